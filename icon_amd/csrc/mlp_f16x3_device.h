// mlp_f16x3_device.h - device side of the 3x f16 split-precision MLP (see mlp_f16x3.hip for the design notes):
// operand image layout, LDS-DMA helpers and the per-chunk MFMA bodies, shared by k_mlp_f16x3 (MLP on
// materialised input rows) and k_fused_f16x3 (fused_f16x3.hip: features computed in the same kernel).
#pragma once
#include "common.h"

namespace icon {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) const void gvoid_t;
typedef __attribute__((address_space(3))) void lvoid_t;

constexpr int kF16Block = 512;                 // 8 waves x 32 points
constexpr int kF16Pts = (kF16Block / 64) * 32; // 256 points per workgroup
constexpr int kBufBytes = 40 * 1024;
constexpr int kW3Stride = 40;                        // w3 per lane group g: 32 hidden weights + 8 raw-input weights
constexpr int kW3Float = 512 + 256 + 128;
constexpr int kZeroFloat = kW3Float + 4 * kW3Stride; // 16 bytes of zeros: the k >= 16 half of the packed [W_lo | 0] operands
constexpr int kSideFloats = kZeroFloat + 4;          // b0 | b1 | b2 | w3 | zeros, staged once per workgroup
constexpr int kW0Off = 2 * kBufBytes;                // layer-0 operands, resident for the whole workgroup
constexpr int kW0Bytes = 32 * 1024;
constexpr int kSideOff = kW0Off + kW0Bytes;
constexpr int kLdsBytes = kSideOff + 4352;           // 80 KiB double buffer + 32 KiB W0 + 4.25 KiB side arrays
constexpr int kZeroFromW0 = kSideOff + kZeroFloat * 4 - kW0Off;   // the zeros, addressed from the W0 region's base
constexpr int kZeroFromBuf0 = kSideOff + kZeroFloat * 4;          // ... and from the first weight buffer = the start of the LDS
static_assert(kSideFloats * 4 <= 4352 && kZeroFromW0 % 16 == 0, "side arrays");

// packed image: [W0: 32 KiB][layer-1 chunks 0..15: 32 KiB each][layer-2 chunks 16: 40 KiB (the raw-input tiles ride on the
// FIRST one: their B operand, the split input row, leaves the registers before the chain is at its widest), 17..19: 32 KiB]
// chunk k: size in KiB and offset in KiB inside the image
__host__ __device__ constexpr int chunk_units(int k) { return k == 16 ? 40 : 32; }
__host__ __device__ constexpr int chunk_offset(int k) { return 32 + 32 * k + (k > 16 ? 8 : 0); }
constexpr size_t kImageBytes = (size_t)(32 + 19 * 32 + 40) * 1024;   // 680 KiB

struct MlpF16Dev {
    const char *image;          // packed f16 hi/lo A operands, chunked
    const float *side;          // f32: b0 [512] | b1 [256] | b2 [128] (bias * weight scale, channel order) | w3 [4][40] | 4 zeros
    float b3;
    float inv0, inv1, inv2;     // 1 / weight scale of layers 0..2
    // LeakyReLU constants 0.505 / scale and 0.495 / scale per layer, from the host: wave-uniform kernel arguments stay in SGPRs
    // (computed in the kernel they took five vector registers of a body that has none to spare: 20 B/lane of scratch)
    float p0, q0, p1, q1, p2, q2;
    int c0;
    int last_op;                // ICON_LASTOP_*
    int *flag;                  // raised when an in-cube result is not finite (operand beyond the f16 range): k_rescue_* redo the point in f32
};

// the in_cube mask as a SELECT (a masked point is 0 whatever the network said - 0 * NaN would not be), and the range flag
__device__ __forceinline__ float masked_result(float y, bool in_cube, int *flag)
{
    if (in_cube && not_finite(y)) *flag = 1;
    return in_cube ? y : 0.0f;
}

// lo halves of a pair: f16(v - hi), the subtraction exact in f32 (hi is a truncation of v), ONE rounding
// (nearest-even) into f16 - v_fma_mixlo/hi_f16 computes fma(f16 hi, -1.0, f32 v) straight into the low / high
// half of the packed result: 2 issue slots where `v - (float)hi` + cvt_pkrtz takes 5 (2 x v_cvt_f32_f16,
// 2 x v_sub_f32, v_cvt_pkrtz).  The activation VALU work is dynamic power the matrix pipe cannot use: the
// kernel is power-bound (tools/mlp_power_probe.py), so every removed VALU instruction is time.
__device__ __forceinline__ fp16x2 residual_pair(fp16x2 hh, float v0, float v1)
{
    const int hb = __builtin_bit_cast(int, hh);
    int lb;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(lb) : "v"(hb), "v"(v0));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lb) : "v"(hb), "v"(v1));
    return __builtin_bit_cast(fp16x2, lb);
}

// x -> (hi, lo) with hi = f16_rtz(x), lo = f16_rne(x - hi); 8 values -> one MFMA operand each
__device__ __forceinline__ void split8(const float *v, half8 &hi, half8 &lo)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const fp16x2 h = __builtin_amdgcn_cvt_pkrtz(v[2 * q], v[2 * q + 1]);
        const fp16x2 l = residual_pair(h, v[2 * q], v[2 * q + 1]);
        hi[2 * q] = (_Float16)h[0]; hi[2 * q + 1] = (_Float16)h[1];
        lo[2 * q] = (_Float16)l[0]; lo[2 * q + 1] = (_Float16)l[1];
    }
}

// LeakyReLU(0.01) of an accumulator value with the weight scale divided out, in TWO VALU operations:
//   max(x, 0.01 x) = 0.505 x + 0.495 |x|,  x = a * inv   ->   fma(|a|, 0.495 inv, (0.505 inv) * a)
// instead of three (a * inv, 0.01 * x, max).  0.505f + 0.495f == 1 exactly; the negative slope comes out as 0.00999999 instead of
// 0.00999999978 (1e-8 of |x| - a twentieth of the 2^-22 the split product carries) and the positive branch takes one more
// rounding.  Round 3: the activation work hides in the MFMA shadow but not its energy - 14.04-14.18 vs 14.14-14.26 ms standalone.
// ICON_ACT_EXACT=1 builds the three-operation form.
#ifndef ICON_ACT_EXACT
#define ICON_ACT_EXACT 0
#endif
struct LeakyK { float inv, p, q; };          // 1 / scale, 0.505 / scale, 0.495 / scale
__device__ __forceinline__ float leaky_scaled(float a, const LeakyK &k)
{
#if ICON_ACT_EXACT
    const float x = a * k.inv;
    return fmaxf(x, 0.01f * x);
#else
    return fmaf(fabsf(a), k.q, k.p * a);
#endif
}

// The MFMA is v_mfma_f32_16x16x32_f16 (16 cycles, K = 32 per instruction).  Lane l = (r = l & 15, g = l >> 4):
//   A (weights, 16 channels x 32 k): row r, halves k = 8g..8g+7;   B (points, 32 k x 16 points): point r, the same k;
//   D: acc[j] = channel 4g + j of point r.
// One wave = 32 points = two 16-point blocks b (point 16b + r).  Two finished 16-channel D tiles Ta, Tb of a block hold
// eight values of the lane's own point: they ARE k-slots 8g..8g+7 of one K = 32 step of the next layer,
//   slot 8g + e  <-  channel 4g + e of Ta (e < 4),  channel 16 + 4g + (e - 4) of Tb (e >= 4)      [sigma() of the packer]
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ half8 lds_op(const char *buf, int slot, int lane)
{
    return *reinterpret_cast<const half8 *>(buf + slot * 1024 + lane * 16);
}
// A lane's LDS address as ONE 32-bit register the optimiser cannot take apart again (base of the LDS map + lane part): what
// the bodies below add to it are immediates of the ds_read.  Left transparent, such an address is re-derived at every use as
// lane part + base + constant - two or three vector instructions in front of the read.
typedef __attribute__((address_space(3))) const char *lds_cptr;
typedef __attribute__((address_space(3))) const half8 *lds_half8;
typedef __attribute__((address_space(3))) const f32x4 *lds_f32x4;
__device__ __forceinline__ lds_cptr lds_lane_address(const void *p)
{
    unsigned a = (unsigned)(size_t)(__attribute__((address_space(3))) const void *)p;
    asm("" : "+v"(a));
    return (lds_cptr)(size_t)a;
}

// (The timing-only variants of round 3 - builds that remove one component of these bodies and give WRONG results by
//  construction - live in tools/probes/exp_r03/, a snapshot of this header with its ICON_EXP_* switches; the product
//  header has no such switch: tests/test_host.py::test_hot_kernels_do_not_spill checks.)
#define ICON_CHUNK_BARRIER() __syncthreads()

// every wave DMAs 1 KiB pieces round-robin: global [piece][lane][16 B] -> LDS, same order

__device__ __forceinline__ void issue_units(const char *src, char *buf, int units, int wave, int lane)
{
    for (int u = wave; u < units; u += kF16Block / 64)
        __builtin_amdgcn_global_load_lds((gvoid_t *)(src + u * 1024 + lane * 16), (lvoid_t *)(buf + u * 1024), 16, 0, 0);
}
__device__ __forceinline__ void issue_chunk(const char *image, char *buf, int k, int wave, int lane)
{
    issue_units(image + (size_t)chunk_offset(k) * 1024, buf, chunk_units(k), wave, lane);
}
// The same pieces in the same order for a unit count known at compile time (the chunks inside the tile loop: 32 units, 40 for
// chunk 16 - 4 or 5 per wave): straight-line, `src` / `dst` = the wave's FIRST piece (wave-uniform: the scalar unit adds the
// 8 KiB between a wave's pieces), the lane's 16 bytes the only vector operand - the run-time form above costs a branch and a
// 64-bit vector add per piece.  (The piece's base goes through an empty asm with a scalar constraint: left to itself the
// compiler folds the lane's offset into a 64-bit VECTOR base outside the chunk loop and adds the piece offsets to that.)
// lane_off: lane * 16, a register of the caller's that passes through an empty asm HERE, in the block of the loads - the
// scalar-base form is only chosen with the 32-bit offset in sight, not with a 64-bit copy of it hoisted out of the chunk loop.
template <int UNITS>
__device__ __forceinline__ void issue_wave_units(const char *src, char *dst, unsigned &lane_off)
{
    constexpr int kWaves = kF16Block / 64;
    static_assert(UNITS % kWaves == 0, "every wave issues the same number of pieces");
    asm volatile("" : "+v"(lane_off));
#pragma unroll
    for (int j = 0; j < UNITS / kWaves; ++j) {
        const char *piece = src + j * kWaves * 1024;
        asm volatile("" : "+s"(piece));
        __builtin_amdgcn_global_load_lds((gvoid_t *)(piece + lane_off), (lvoid_t *)(dst + j * kWaves * 1024), 16, 0, 0);
    }
}
// chunk k (a constant, or one of a run of equally sized chunks: layer 1) -> buf
template <int UNITS>
__device__ __forceinline__ void issue_chunk_units(const char *image, char *buf, int k, int wave, int lane)
{
    unsigned lane_off = (unsigned)lane * 16u;
    issue_wave_units<UNITS>(image + (size_t)(chunk_offset(k) + wave) * 1024, buf + wave * 1024, lane_off);
}

// The per-chunk bodies take the buffer being READ, the buffer being FILLED and the side arrays as
// __restrict__ parameters of a force-inlined function: after inlining, the ds_reads carry alias
// scopes that prove they cannot touch the LDS-DMA destination, so the compiler's waitcnt pass does
// not drain the DMA queue (s_waitcnt vmcnt(0)) in front of every LDS read - the DMA for chunk k+1
// stays in flight for the whole multiplication of chunk k and is only waited for at the barrier.

// 3-term product group of one output tile M of both point blocks: 6 MFMAs (96 cycles), an accumulator comes back
// after two instructions.  Groups are per TILE so that only one tile's operands are held while the next one's are read.
#define GROUP6(ACC, M, AH, AL, BH, BL)                                                              \
    ACC[M][0] = MFMA32(AH, BH[0], ACC[M][0]); ACC[M][1] = MFMA32(AH, BH[1], ACC[M][1]);             \
    ACC[M][0] = MFMA32(AH, BL[0], ACC[M][0]); ACC[M][1] = MFMA32(AH, BL[1], ACC[M][1]);             \
    ACC[M][0] = MFMA32(AL, BH[0], ACC[M][0]); ACC[M][1] = MFMA32(AL, BH[1], ACC[M][1]);

// The raw-input operand of a wave (layer 0 and the tail of layer 2): K = c0 <= 16, so TWO of the three terms share one
// K = 32 instruction:  [W_hi | W_hi] x [x_hi | x_lo]  and  [W_lo | 0] x [x_hi | x_lo]  (the x_lo half meets zeros).
// xb[b]: lanes g < 2 hold x_hi[8g..8g+7] of point 16b + r, lanes g >= 2 hold x_lo[8(g-2)..].  row0 / row1: the f32 rows
// of the lane's two points at input 8 (g & 1).  Returns the lane's share of layer 3's raw-input columns (f32, inputs
// 8 (g & 1) + s of the point of block g >> 1; one fma chain from 0, s ascending): one register across the MFMA body
// where the eight inputs would be eight.
__device__ __forceinline__ float load_x(const float *row0, const float *row1, const float *__restrict__ sw3, int c0, int g, half8 (&xb)[2])
{
    float tail = 0.0f;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const float4 *q = reinterpret_cast<const float4 *>(b ? row1 : row0);
        const float4 u = q[0], v = q[1];
        float x[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
#pragma unroll
        for (int s = 0; s < 8; ++s) x[s] = (s + 8 * (g & 1) < c0) ? x[s] : 0.0f;
        half8 hi, lo;
        split8(x, hi, lo);
        xb[b] = g < 2 ? hi : lo;
        float t = 0.0f;
#pragma unroll
        for (int s = 0; s < 8; ++s) t = fmaf(sw3[g * kW3Stride + 32 + s], x[s], t);
        tail = (g >> 1) == b ? t : tail;
    }
    // (opaque: computed HERE - sunk behind the MFMA body, where its result is used, it would keep the sixteen inputs alive)
    asm volatile("" : "+v"(tail));
    return tail;
}

// A operands of a raw-input tile (1 KiB: [W_hi: 32 lanes][W_lo: 32 lanes], lane (r, g & 1)): a1 = [W_hi | W_hi],
// a2 = [W_lo | 0] - lanes g >= 2 read the 16 zero bytes behind the side arrays; zero_off: their offset from `base`
// (kZeroFromW0 for the W0 region, kZeroFromBuf0 for the first weight buffer).  The zeros meet the x_lo half of
// B = [x_hi | x_lo] - the same as a B of [x_hi | 0] for every finite x_lo; an x_lo that is not (|x| beyond the f16 range)
// gives NaN, which raises the range flag as the hi * lo term always did.
__device__ __forceinline__ void raw_operands(const char *__restrict__ base, int tile, int zero_off, int g, int lane, half8 &a1, half8 &a2)
{
    const int col = (lane & 31) * 16;
    const int lo_off = g < 2 ? 512 + col : zero_off, lo_mul = g < 2 ? 1024 : 0;
    a1 = *reinterpret_cast<const half8 *>(base + tile * 1024 + col);
    a2 = *reinterpret_cast<const half8 *>(base + lo_off + tile * lo_mul);
}

// Where a lane reads the layer-0 operands of the channel tiles not yet multiplied: running LDS addresses, advanced by layer01
// once per PAIR of chunks (the four tiles of a pair are immediates on them) - a tile index times 1024 / 64 re-derived per
// chunk was eight vector instructions of shifts, a multiplication and adds.  Only the [W_lo | 0] operand moves per tile: lanes
// g >= 2 stay on the zeros (step 0), which no immediate can say.  Set up per TILE from the opaque thread index like every
// lane-dependent address (fused_f16x3.hip).
struct L0At { lds_cptr hi, lo, bias; int lo_step; };
__device__ __forceinline__ L0At l0_begin(const char *W0, const float *sb0, int g, int lane)
{
    const int col = (lane & 31) * 16;
    return L0At{lds_lane_address(W0 + col), lds_lane_address(W0 + (g < 2 ? 512 + col : kZeroFromW0)), lds_lane_address(sb0 + 4 * g), g < 2 ? 1024 : 0};
}

// layer 0, 32 hidden channels of both point blocks (h0[b][t]: channel tile T + K + t, T = the tile hi / bias stand at, lo at
// T + K): 8 MFMAs from the resident W0 region; operands as raw_operands() names them.  The addresses are __restrict__
// parameters BY VALUE: the reads stay provably apart from the LDS-DMA destination of the chunk body they are inlined into.
template <int K>
__device__ __forceinline__ void l0_tiles(lds_cptr __restrict__ hi, lds_cptr __restrict__ lo, int lo_step, lds_cptr __restrict__ bias,
                                         const half8 (&xb)[2], f32x4 (&h0)[2][2])
{
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const f32x4 b = *(lds_f32x4)(bias + (K + t) * 64);
        const half8 a1 = *(lds_half8)(hi + (K + t) * 1024);
        const half8 a2 = *(lds_half8)(lo + t * lo_step);
        h0[0][t] = MFMA32(a1, xb[0], b); h0[1][t] = MFMA32(a1, xb[1], b);
        h0[0][t] = MFMA32(a2, xb[0], h0[0][t]); h0[1][t] = MFMA32(a2, xb[1], h0[1][t]);
    }
}

// one eighth of the activation step of two finished tiles Ta, Tb of both blocks: block b = k >> 2, pair q = k & 3 of its
// next B operand (slots 2q, 2q+1: from Ta for q < 2, from Tb otherwise) -> LeakyReLU -> hi/lo halves
__device__ __forceinline__ void act_part(const f32x4 &ta0, const f32x4 &tb0, const f32x4 &ta1, const f32x4 &tb1, int k, const LeakyK &inv,
                                         half8 (&nh)[2], half8 (&nl)[2])
{
    const int b = k >> 2, q = k & 3, j0 = (q & 1) * 2;
    const f32x4 &src = b ? (q >> 1 ? tb1 : ta1) : (q >> 1 ? tb0 : ta0);
    const float v0 = leaky_scaled(src[j0], inv), v1 = leaky_scaled(src[j0 + 1], inv);      // 7 VALU per pair with the split below
    fp16x2 hh = __builtin_amdgcn_cvt_pkrtz(v0, v1);
    fp16x2 ll = residual_pair(hh, v0, v1);
    // the (empty) volatile asm is ordered against the surrounding sched_barriers, which keeps this
    // VALU work in the MFMA group it was written next to instead of being sunk to the end of the chunk
    int hb = __builtin_bit_cast(int, hh), lb = __builtin_bit_cast(int, ll);
    asm volatile("" : "+v"(hb), "+v"(lb));
    hh = __builtin_bit_cast(fp16x2, hb); ll = __builtin_bit_cast(fp16x2, lb);
    nh[b][2 * q] = (_Float16)hh[0]; nh[b][2 * q + 1] = (_Float16)hh[1];
    nl[b][2 * q] = (_Float16)ll[0]; nl[b][2 * q + 1] = (_Float16)ll[1];
}

// activation step of two finished tiles outside the pipelined bodies (the first B operand of a layer)
__device__ __forceinline__ void activate_split(const f32x4 &ta0, const f32x4 &tb0, const f32x4 &ta1, const f32x4 &tb1, const LeakyK &inv,
                                               half8 (&bh)[2], half8 (&bl)[2])
{
#pragma unroll
    for (int k = 0; k < 8; ++k) act_part(ta0, tb0, ta1, tb1, k, inv, bh, bl);
}

// layer 1, one chunk (K = 32 hidden channels = ONE k-step, B operands bh/bl prepared one chunk
// earlier) SOFTWARE-PIPELINED with layer 0 of the next chunk: its eight MFMAs are issued first; its
// LeakyReLU + hi/lo split (pure VALU, 8 parts) is slotted behind every second of the sixteen 6-MFMA groups of this
// chunk, and the LDS reads of group t+1 are issued ahead of the MFMAs of group t.  sched_barrier
// pins that interleave so the matrix pipe and the VALU run side by side instead of alternating.
// The next chunk's B operands are built in nh/nl - registers of their own: the caller swaps the two sets from chunk to chunk
// (layer01), there is no hand-over copy.  The last chunk has no successor: it runs without the layer-0 part and DMAs
// chunk 16 (40 units).  Tile t: hi in slot 2t, lo in 2t + 1.  next_src: the wave's first piece of the next chunk;
// K0: the next chunk's layer-0 tiles as l0_tiles<K0> counts them.  L: the LANE's 16 bytes of slot 0 of the buffer read.
template <bool LAST, int K0>
__device__ __forceinline__ void l01_chunk(lds_cptr __restrict__ L, char *__restrict__ nxt, lds_cptr __restrict__ w_hi,
                                          lds_cptr __restrict__ w_lo, int lo_step, lds_cptr __restrict__ bias, const char *next_src,
                                          f32x4 (&acc1)[16][2], const half8 (&xb)[2], const LeakyK &inv0, unsigned &lane_off, int wave,
                                          const half8 (&bh)[2], const half8 (&bl)[2], half8 (&nh)[2], half8 (&nl)[2])
{
    issue_wave_units<LAST ? 40 : 32>(next_src, nxt + wave * 1024, lane_off);
    f32x4 h0n[2][2];
    if (!LAST) l0_tiles<K0>(w_hi, w_lo, lo_step, bias, xb, h0n);
    half8 a[2][2];
    a[0][0] = *(lds_half8)L; a[0][1] = *(lds_half8)(L + 1024);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        if (t + 1 < 16) { a[(t + 1) & 1][0] = *(lds_half8)(L + (2 * t + 2) * 1024); a[(t + 1) & 1][1] = *(lds_half8)(L + (2 * t + 3) * 1024); }
        GROUP6(acc1, t, a[t & 1][0], a[t & 1][1], bh, bl)
        if (!LAST && (t & 1)) act_part(h0n[0][0], h0n[0][1], h0n[1][0], h0n[1][1], t >> 1, inv0, nh, nl);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// layers 0 + 1 of a tile: layer 0 of hidden tiles 0, 1, then chunks 0..15 TWO per loop iteration, so that the buffer a chunk
// reads and the one it fills are constants (every LDS address of the body is the lane's offset plus an immediate) and the two
// sets of B-operand registers swap roles instead of being copied: the even chunk reads bh/bl from the first buffer and fills
// nh/nl, the odd chunk the reverse.  7 pairs + the pair (14, 15-LAST); chunk 16 lands in the first buffer.  One barrier per
// chunk: all waves done with the buffer AND the next chunk has landed.  bh/bl: scratch registers of the caller (layer 2's).
__device__ __forceinline__ void layer01(char *smem, const float *sb0, const char *image, f32x4 (&acc1)[16][2], const half8 (&xb)[2],
                                        const LeakyK &inv0, int g, int lane, int wave, half8 (&bh)[2], half8 (&bl)[2])
{
    char *const buf0 = smem, *const buf1 = smem + kBufBytes;
    // the lane's column of the two buffers: a register each (the second buffer ends 6 KiB beyond the reach of an immediate)
    const lds_cptr col0 = lds_lane_address(buf0 + lane * 16), col1 = lds_lane_address(buf1 + lane * 16);
    unsigned lane_off = (unsigned)lane * 16u;
    L0At at = l0_begin(smem + kW0Off, sb0, g, lane);
    {
        f32x4 h0[2][2];
        l0_tiles<0>(at.hi, at.lo, at.lo_step, at.bias, xb, h0);
        activate_split(h0[0][0], h0[0][1], h0[1][0], h0[1][1], inv0, bh, bl);
    }
    // `at` stands at tile 0: the even chunk 2p multiplies layer 0 of tiles 4p + 2, 4p + 3, the odd one 4p + 4, 4p + 5
    at.lo += 2 * at.lo_step;
    const char *src = image + (size_t)(chunk_offset(1) + wave) * 1024;      // chunk c + 1, this wave's first piece (scalar)
    half8 nh[2], nl[2];
#pragma nounroll
    for (int p = 0; p < 7; ++p) {
        l01_chunk<false, 2>(col0, buf1, at.hi, at.lo, at.lo_step, at.bias, src, acc1, xb, inv0, lane_off, wave, bh, bl, nh, nl);
        at.lo += 2 * at.lo_step;
        ICON_CHUNK_BARRIER();
        l01_chunk<false, 4>(col1, buf0, at.hi, at.lo, at.lo_step, at.bias, src + 32 * 1024, acc1, xb, inv0, lane_off, wave, nh, nl, bh, bl);
        at.lo += 2 * at.lo_step;
        ICON_CHUNK_BARRIER();
        at.hi += 4 * 1024; at.bias += 4 * 64;
        src += 64 * 1024;
    }
    l01_chunk<false, 2>(col0, buf1, at.hi, at.lo, at.lo_step, at.bias, src, acc1, xb, inv0, lane_off, wave, bh, bl, nh, nl);
    ICON_CHUNK_BARRIER();
    l01_chunk<true, 0>(col1, buf0, at.hi, at.lo, at.lo_step, at.bias, src + 32 * 1024, acc1, xb, inv0, lane_off, wave, nh, nl, bh, bl);
    ICON_CHUNK_BARRIER();
}

// layer 2, chunk 16+Q: k-steps 2Q, 2Q+1 = hidden tiles 4Q..4Q+3 (+ the raw-input k-step in front of the first chunk).
// Same pipelining as layer 1: while the 48 MFMAs of k-step kk run, the activation + split of
// hidden tiles 2kk+2, 2kk+3 (the next B operand) is slotted behind the eight 6-MFMA groups, one part per group.
template <int Q>
__device__ __forceinline__ void l2_chunk(const char *__restrict__ L, char *__restrict__ nxt, const char *image,
                                         f32x4 (&acc1)[16][2], f32x4 (&acc2)[8][2], const half8 (&xb)[2], const LeakyK &inv1,
                                         int g4, int lane, int wave, half8 (&bh)[2], half8 (&bl)[2], bool issue_next = Q < 3)
{
    // the chunk DMA'd into `nxt` while this one is multiplied: 17 + Q; behind Q == 3 the persistent kernel asks for chunk 0
    // of its NEXT tile - issued from inside this body so that it shares the alias scopes
    if (issue_next) issue_chunk_units<32>(image, nxt, Q < 3 ? 17 + Q : 0, wave, lane);
    if (Q == 0) {
        // raw inputs first: tiles of 1 KiB behind the 32 KiB of hidden k-steps (chunk 16 always lands in the FIRST buffer)
#pragma unroll
        for (int m2 = 0; m2 < 8; ++m2) {
            half8 a1, a2;
            raw_operands(L, 32 + m2, kZeroFromBuf0, g4, lane, a1, a2);
            acc2[m2][0] = MFMA32(a1, xb[0], acc2[m2][0]); acc2[m2][1] = MFMA32(a1, xb[1], acc2[m2][1]);
            acc2[m2][0] = MFMA32(a2, xb[0], acc2[m2][0]); acc2[m2][1] = MFMA32(a2, xb[1], acc2[m2][1]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int mm = 0; mm < 2; ++mm) {
        constexpr int kLast = 7;
        const int kk = 2 * Q + mm, n = kk < kLast ? 2 * kk + 2 : 0;
        half8 nh[2], nl[2];
        half8 a[2][2];
        a[0][0] = lds_op(L, mm * 16, lane); a[0][1] = lds_op(L, mm * 16 + 1, lane);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            if (t + 1 < 8) { a[(t + 1) & 1][0] = lds_op(L, mm * 16 + 2 * t + 2, lane); a[(t + 1) & 1][1] = lds_op(L, mm * 16 + 2 * t + 3, lane); }
            GROUP6(acc2, t, a[t & 1][0], a[t & 1][1], bh, bl)
            if (kk < kLast) act_part(acc1[n][0], acc1[n + 1][0], acc1[n][1], acc1[n + 1][1], t, inv1, nh, nl);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (kk < kLast) { bh[0] = nh[0]; bh[1] = nh[1]; bl[0] = nl[0]; bl[1] = nl[1]; }
    }
}

// layer 3 on the VALU (f32) + the cross-lane sum.  Summation order of a point, stated for tools/sim_f16x3.py and the same
// wherever the point sits in its wave (fused and materialising kernels place it differently): per lane group g one fma chain
// H_g over its hidden channels 16 m2 + 4g + j (m2 = 0..7 outer, j = 0..3 inner, starting from 0);
// H = (H_0 + H_1) + (H_2 + H_3) (partners 16, then 32 lanes apart); the raw inputs 8 h + s (s = 0..7, fma chains T_h from 0:
// load_x, carried by lane groups 2 (block) + h) give T = T_0 + T_1;  y = (H + T) + b3.  y[b]: point 16b + r, in every lane.
__device__ __forceinline__ void l3_sum(const float *__restrict__ sw3, const f32x4 (&acc2)[8][2], float tail, const LeakyK &inv2,
                                       float b3, int g, float (&y)[2])
{
    const float *w3 = sw3 + g * kW3Stride;
    float part[2] = {0.0f, 0.0f};
#pragma unroll
    for (int m2 = 0; m2 < 8; ++m2) {
        const f32x4 wv = *reinterpret_cast<const f32x4 *>(w3 + 4 * m2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            part[0] = fmaf(wv[j], leaky_scaled(acc2[m2][0][j], inv2), part[0]);
            part[1] = fmaf(wv[j], leaky_scaled(acc2[m2][1][j], inv2), part[1]);
        }
    }
    const float t = tail + __shfl_xor(tail, 16);        // lane groups 0, 1: T of block 0; 2, 3: T of block 1
    const float t_other = __shfl_xor(t, 32);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        part[b] += __shfl_xor(part[b], 16);
        part[b] += __shfl_xor(part[b], 32);
        y[b] = (part[b] + ((g >> 1) == b ? t : t_other)) + b3;
    }
}

}  // namespace icon

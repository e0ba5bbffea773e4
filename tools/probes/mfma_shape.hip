// timing-only probe: ONE layer-1 chunk body of the f16x3 MLP in the two f16 MFMA shapes, on N(0,1) data.
//
// Question behind it ("MFMA shape"): the fused kernel is power-bound, and bare MFMA loops hold a
// higher clock on v_mfma_f32_16x16x32_f16 than on v_mfma_f32_32x32x16_f16 at equal cycles.  Does the chunk body of
// mlp_f16x3_device.h - MFMAs + ds_read_b128 of every A operand + the 7-VALU-per-pair activation/split of the next
// chunk's B operand + the LDS-DMA of the next chunk + one barrier - keep that advantage?
//
//   shape 0: l01_chunk() as the product had it on 32x32x16 (kept below, verbatim): 48 + 3 MFMAs per chunk and wave
//   shape 1: l01_chunk<false>() of the PRODUCT header, 16x16x32: one wave = 32 points = two 16-point blocks, 16 channel
//            tiles, 96 + 8 MFMAs per chunk and wave (layer 0 as two packed instructions per 16x16 outputs:
//            [W_hi | W_hi] x [x_hi | x_lo] and [W_lo | 0] x [x_hi | x_lo]), the same 32 + 4 A reads, the same 8 activation
//            parts, the same DMA and barrier.  The D tiles of layer 0 are the next B operands in registers.
// Both run 16 chunks per "tile" of 256 points on a persistent grid of one 512-thread workgroup per CU, tile after tile.
// Results are NOT those of the MLP (the operand image is random numbers in slot order); only time, cycles and clock count.
//
// Per shape: >= 2 s of back-to-back launches, then timed launches; the last launch's s_memtime / s_memrealtime stamps
// (one pair around the tile loop, written to a buffer nothing else reads) give the in-kernel clock, median over workgroups.
// Order 0 1 0 1 so that drift shows.
//
// build: hipcc --offload-arch=gfx950 -O3 -I icon_amd/csrc -o mfma_shape tools/probes/mfma_shape.hip
#include "mlp_f16x3_device.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace icon;

// ---- shape 0: the chunk body as the product had it before the change of shape, verbatim ----------------------------------
namespace old32 {
typedef float f32x16 __attribute__((ext_vector_type(16)));
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ f32x16 ld16(const float *p)
{
    const float4 *q = reinterpret_cast<const float4 *>(p);
    const float4 a = q[0], b = q[1], c = q[2], d = q[3];
    f32x16 v;
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w; v[12] = d.x; v[13] = d.y; v[14] = d.z; v[15] = d.w;
    return v;
}

// activation step of a finished tile: undo the weight scale, LeakyReLU(0.01), split for the next GEMM
__device__ __forceinline__ void activate_split(const f32x16 &acc, const LeakyK &inv, half8 hi[2], half8 lo[2])
{
    float v[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) v[t] = leaky_scaled(acc[t], inv);
    split8(v, hi[0], lo[0]);
    split8(v + 8, hi[1], lo[1]);
}

__device__ __forceinline__ half8 lds_op(const char *buf, int slot, int lane)
{
    return *reinterpret_cast<const half8 *>(buf + slot * 1024 + lane * 16);
}

// 3-term product group for 2 output tiles sharing one B operand pair
#define TRIPLE2(ACC, M0, AH, AL, BH, BL)                                     \
    ACC[M0] = MFMA16(AH[0], BH, ACC[M0]); ACC[M0 + 1] = MFMA16(AH[1], BH, ACC[M0 + 1]); \
    ACC[M0] = MFMA16(AH[0], BL, ACC[M0]); ACC[M0 + 1] = MFMA16(AH[1], BL, ACC[M0 + 1]); \
    ACC[M0] = MFMA16(AL[0], BH, ACC[M0]); ACC[M0 + 1] = MFMA16(AL[1], BH, ACC[M0 + 1]);

// layer 0, hidden tile c (32 channels): 3 MFMAs from the resident W0 region
__device__ __forceinline__ f32x16 l0_tile(const char *__restrict__ W0, const float *__restrict__ sb0, int c, half8 xhi, half8 xlo,
                                          int h, int lane)
{
    f32x16 h0 = ld16(sb0 + (c * 2 + h) * 16);
    const half8 a_hi = lds_op(W0, 2 * c, lane), a_lo = lds_op(W0, 2 * c + 1, lane);
    h0 = MFMA16(a_hi, xhi, h0); h0 = MFMA16(a_hi, xlo, h0); h0 = MFMA16(a_lo, xhi, h0);
    return h0;
}

// one eighth of the activation step of a finished layer-0 tile: values 2k, 2k+1 -> LeakyReLU ->
// hi/lo halves -> pair (k&3) of the next B operand (u = k>>2)
__device__ __forceinline__ void act_part(const f32x16 &acc, int k, const LeakyK &inv, half8 (&nh)[2], half8 (&nl)[2])
{

    const float v0 = leaky_scaled(acc[2 * k], inv), v1 = leaky_scaled(acc[2 * k + 1], inv);      // 7 VALU per pair with the split below
    fp16x2 hh = __builtin_amdgcn_cvt_pkrtz(v0, v1);
    fp16x2 ll = residual_pair(hh, v0, v1);
    // the (empty) volatile asm is ordered against the surrounding sched_barriers, which keeps this
    // VALU work in the MFMA group it was written next to instead of being sunk to the end of the chunk
    int hb = __builtin_bit_cast(int, hh), lb = __builtin_bit_cast(int, ll);
    asm volatile("" : "+v"(hb), "+v"(lb));
    hh = __builtin_bit_cast(fp16x2, hb); ll = __builtin_bit_cast(fp16x2, lb);
    const int u = k >> 2, q = k & 3;
    nh[u][2 * q] = (_Float16)hh[0]; nh[u][2 * q + 1] = (_Float16)hh[1];
    nl[u][2 * q] = (_Float16)ll[0]; nl[u][2 * q + 1] = (_Float16)ll[1];
}

// A operands of MFMA group g of a layer-1 chunk: output tiles 2*(g&3), +1 for k-step u = g>>2
__device__ __forceinline__ void load_group(const char *__restrict__ L, int g, int lane, half8 (&a)[4])
{
    const int slot = ((g >> 2) * 8 + (g & 3) * 2) * 2;
    a[0] = lds_op(L, slot, lane); a[1] = lds_op(L, slot + 2, lane);        // hi of tile 0, 1
    a[2] = lds_op(L, slot + 1, lane); a[3] = lds_op(L, slot + 3, lane);    // lo of tile 0, 1
}

// layer 1, chunk c (K = hidden channels 32c..32c+31, B operands bh/bl prepared one iteration
// earlier) SOFTWARE-PIPELINED with layer 0 of chunk c+1: its three MFMAs are issued first; its
// LeakyReLU + hi/lo split (pure VALU, 8 parts) is slotted between the eight 6-MFMA groups of this
// chunk, and the LDS reads of group g+1 are issued ahead of the MFMAs of group g.  sched_barrier
// pins that interleave so the matrix pipe and the VALU run side by side instead of alternating.
__device__ __forceinline__ void l01_chunk(const char *__restrict__ L, char *__restrict__ nxt, const char *__restrict__ W0,
                                          const float *__restrict__ sb0, const char *image, int c, f32x16 (&acc1)[8],
                                          half8 xhi, half8 xlo, const LeakyK &inv0, int h, int lane, int wave,
                                          half8 (&bh)[2], half8 (&bl)[2])
{
    issue_chunk(image, nxt, c + 1, wave, lane);
    const f32x16 h0n = l0_tile(W0, sb0, min(c + 1, 15), xhi, xlo, h, lane);   // c == 15: harmless repeat
    half8 nh[2], nl[2];
    half8 a[2][4];
    load_group(L, 0, lane, a[0]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        if (g + 1 < 8) load_group(L, g + 1, lane, a[(g + 1) & 1]);
        const int u = g >> 2, m0 = (g & 3) * 2;
        const half8 ah[2] = {a[g & 1][0], a[g & 1][1]}, al[2] = {a[g & 1][2], a[g & 1][3]};
        TRIPLE2(acc1, m0, ah, al, bh[u], bl[u])
        if (g >= 1) act_part(h0n, g - 1, inv0, nh, nl);
        __builtin_amdgcn_sched_barrier(0);
    }
    act_part(h0n, 7, inv0, nh, nl);
    bh[0] = nh[0]; bh[1] = nh[1]; bl[0] = nl[0]; bl[1] = nl[1];
}
}  // namespace old32

// ---- the probe kernel -------------------------------------------------------------------------------------------------

struct ProbeArgs {
    const char *image;      // kImageBytes, random operands in slot order
    const float *side;      // kSideFloats
    const float *X;         // [grid * 256][16]
    float *sink;            // [grid * 512]
    unsigned long long *stamps;   // [grid][4]: memtime before, memrealtime before, memtime after, memrealtime after
    int tiles;
    float inv0, p0, q0;
};

template <int SHAPE>
__global__ __launch_bounds__(kF16Block, 2) void k_probe(ProbeArgs w)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const char *chunks = w.image;
    issue_units(w.image, smem + kW0Off, kW0Bytes / 1024, wave, lane);
    float *side = reinterpret_cast<float *>(smem + kSideOff);
    for (int i = threadIdx.x; i < kSideFloats; i += kF16Block) side[i] = w.side[i];
    const float *sb0 = side, *sb1 = side + 512;
    const LeakyK inv0{w.inv0, w.p0, w.q0};

    // B operands of layer 0.  shape 0: point lane & 31, k = 8h..8h+7 of K = 16, hi and lo.
    // shape 1: block b, point lane & 15, lanes g < 2 hold x_hi[8g..], lanes g >= 2 hold x_lo[8(g-2)..]
    const int h = lane >> 5, g4 = lane >> 4;
    half8 xhi, xlo, xb[2];
    if (SHAPE == 0) {
        const float *xp = w.X + ((size_t)(blockIdx.x * 256 + wave * 32 + (lane & 31))) * 16 + 8 * h;
        float xr[8];
        for (int s = 0; s < 8; ++s) xr[s] = (s + 8 * h < 13) ? xp[s] : 0.0f;
        split8(xr, xhi, xlo);
    } else {
        for (int b = 0; b < 2; ++b) {
            const float *xp = w.X + ((size_t)(blockIdx.x * 256 + wave * 32 + b * 16 + (lane & 15))) * 16 + 8 * (g4 & 1);
            float xr[8];
            for (int s = 0; s < 8; ++s) xr[s] = (s + 8 * (g4 & 1) < 13) ? xp[s] : 0.0f;
            half8 hi, lo;
            split8(xr, hi, lo);
            xb[b] = g4 < 2 ? hi : lo;
        }
    }
    issue_chunk(chunks, smem, 0, wave, lane);
    __syncthreads();

    float chk = 0.0f;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int tile = 0; tile < w.tiles; ++tile) {
        half8 bh[2], bl[2];
        if (SHAPE == 0) {
            old32::f32x16 acc1[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) acc1[m] = old32::ld16(sb1 + (m * 2 + h) * 16);
            old32::activate_split(old32::l0_tile(smem + kW0Off, sb0, 0, xhi, xlo, h, lane), inv0, bh, bl);
            for (int c = 0; c < 16; ++c) {
                old32::l01_chunk(smem + (c & 1) * kBufBytes, smem + ((c + 1) & 1) * kBufBytes, smem + kW0Off, sb0, chunks, c, acc1, xhi, xlo,
                          inv0, h, lane, wave, bh, bl);
                ICON_CHUNK_BARRIER();
            }
#pragma unroll
            for (int m = 0; m < 8; ++m)
#pragma unroll
                for (int t = 0; t < 16; ++t) chk += acc1[m][t];
        } else {
            f32x4 acc1[16][2];
#pragma unroll
            for (int m = 0; m < 16; ++m) acc1[m][0] = acc1[m][1] = *reinterpret_cast<const f32x4 *>(sb1 + m * 16 + 4 * g4);
            // the product's layers 0 + 1 as they are (the last chunk runs without the layer-0 part and DMAs chunk 16)
            layer01(smem, sb0, chunks, acc1, xb, inv0, g4, lane, wave, bh, bl);
#pragma unroll
            for (int m = 0; m < 16; ++m)
#pragma unroll
                for (int t = 0; t < 4; ++t) chk += acc1[m][0][t] + acc1[m][1][t];
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    w.sink[blockIdx.x * kF16Block + threadIdx.x] = chk;
    if (threadIdx.x == 0) {
        unsigned long long *s = w.stamps + (size_t)blockIdx.x * 4;
        s[0] = t0; s[1] = r0; s[2] = t1; s[3] = r1;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static uint16_t f16_bits(_Float16 v) { uint16_t b; memcpy(&b, &v, 2); return b; }
// hi = f16 truncation of v, lo = f16(v - hi): what mlp_pack_f16x3 stores
static void split_host(float v, uint16_t &hi, uint16_t &lo)
{
    _Float16 hh = (_Float16)v;
    if (fabsf((float)hh) > fabsf(v)) { uint16_t b = f16_bits(hh); --b; memcpy(&hh, &b, 2); }
    hi = f16_bits(hh);
    lo = f16_bits((_Float16)(v - (float)hh));
}

struct Result { double ms, mhz, cycles; };

template <int SHAPE>
static int run(const ProbeArgs &base, int grid, int tiles, double warm_s, int timed, Result &res)
{
    ProbeArgs a = base;
    a.tiles = tiles;
    const int lds = kLdsBytes;
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_probe<SHAPE>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    const auto w0 = std::chrono::steady_clock::now();
    int warm = 0;
    do {
        for (int i = 0; i < 8; ++i) hipLaunchKernelGGL(k_probe<SHAPE>, dim3(grid), dim3(kF16Block), lds, 0, a);
        CK(hipDeviceSynchronize());
        warm += 8;
    } while (std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() < warm_s);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    CK(hipEventRecord(e0));
    for (int i = 0; i < timed; ++i) hipLaunchKernelGGL(k_probe<SHAPE>, dim3(grid), dim3(kF16Block), lds, 0, a);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> st((size_t)grid * 4);
    CK(hipMemcpy(st.data(), a.stamps, st.size() * 8, hipMemcpyDeviceToHost));
    std::vector<double> mhz, cyc;
    for (int b = 0; b < grid; ++b) {
        const double dc = (double)(st[b * 4 + 2] - st[b * 4]), dr = (double)(st[b * 4 + 3] - st[b * 4 + 1]);
        if (dr > 0) { mhz.push_back(dc / dr * 100.0); cyc.push_back(dc); }
    }
    std::sort(mhz.begin(), mhz.end()); std::sort(cyc.begin(), cyc.end());
    res.ms = ms / timed;
    res.mhz = mhz.empty() ? 0 : mhz[mhz.size() / 2];
    res.cycles = cyc.empty() ? 0 : cyc[cyc.size() / 2];
    // layer-1 MACs of the three terms, the same in both shapes: 256 channels x 32 points x 32 k x 3 per chunk and wave
    const double macs = (double)grid * 8 * tiles * 16 * 256.0 * 32 * 32 * 3;
    printf("shape %s  warm %4d launches  %8.4f ms/launch  %7.3f fs/MAC  %7.1f cycles/chunk  in-kernel clock %6.0f MHz\n",
           SHAPE ? "16x16x32" : "32x32x16", warm, res.ms, res.ms * 1e12 / macs, res.cycles / (tiles * 16.0), res.mhz);
    fflush(stdout);
    return 0;
}

int main(int argc, char **argv)
{
    const int tiles = argc > 1 ? atoi(argv[1]) : 260;          // 66,000 tiles of the 257^3 step / 256 CUs
    const double warm_s = argc > 2 ? atof(argv[2]) : 2.0;
    const int zero = argc > 3 ? atoi(argv[3]) : 0;             // 1: all-zero operands (ranks the shapes by cycles alone)
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int grid = prop.multiProcessorCount;
    printf("%s  %d CUs  tiles/workgroup %d  data %s\n", prop.gcnArchName, grid, tiles, zero ? "zeros" : "N(0,1)");

    std::mt19937 rng(12345);
    std::normal_distribution<float> nd(0.0f, 1.0f);
    // operand image: [W0][chunks], every 1 KiB slot pair (hi, lo) the split of N(0,1) numbers.  (The 16x16x32 body reads its
    // layer-0 tiles as [hi 512 B][lo 512 B] from the same bytes: hi and lo pieces alternate at 512 B there - random either way.)
    char *d_img;
    {
        std::vector<uint16_t> img(kImageBytes / 2, 0);
        for (size_t p = 0; p + 1 < kImageBytes / 1024; p += 2)
            for (int e = 0; e < 512; ++e) {
                uint16_t hi, lo;
                split_host(zero ? 0.0f : nd(rng), hi, lo);
                img[p * 512 + e] = hi; img[(p + 1) * 512 + e] = lo;
            }
        CK(hipMalloc(&d_img, kImageBytes));
        CK(hipMemcpy(d_img, img.data(), kImageBytes, hipMemcpyHostToDevice));
    }
    std::vector<float> side(kSideFloats), X((size_t)grid * 256 * 16);
    for (auto &v : side) v = zero ? 0.0f : 0.1f * nd(rng);
    for (int i = 0; i < 4; ++i) side[kZeroFloat + i] = 0.0f;
    for (auto &v : X) v = zero ? 0.0f : nd(rng);
    ProbeArgs a{};
    float *d_side, *d_x;
    CK(hipMalloc(&d_side, side.size() * 4)); CK(hipMemcpy(d_side, side.data(), side.size() * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&d_x, X.size() * 4)); CK(hipMemcpy(d_x, X.data(), X.size() * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&a.sink, (size_t)grid * kF16Block * 4));
    CK(hipMalloc(&a.stamps, (size_t)grid * 4 * 8));
    a.side = d_side; a.X = d_x;
    // 13 inputs of N(0,1) x N(0,1) weights: hidden values of N(0, 13); 1/4 brings them back to O(1) like the product's scales
    a.inv0 = 0.25f; a.p0 = 0.505f * a.inv0; a.q0 = 0.495f * a.inv0;

    Result r[2][2];
    for (int rep = 0; rep < 2; ++rep) {
        a.image = d_img; if (run<0>(a, grid, tiles, warm_s, 60, r[rep][0])) return 1;
        if (run<1>(a, grid, tiles, warm_s, 60, r[rep][1])) return 1;
    }
    for (int rep = 0; rep < 2; ++rep)
        printf("rep %d: time per MAC 16x16x32 / 32x32x16 = %.4f   cycles %.4f   clock %.4f\n", rep, r[rep][1].ms / r[rep][0].ms,
               r[rep][1].cycles / r[rep][0].cycles, r[rep][1].mhz / r[rep][0].mhz);
    return 0;
}

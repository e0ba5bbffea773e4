// mlp_f16x3.hip - the occupancy MLP on the f16 matrix cores with float32-class accuracy.
//
// Same contract and the same register-chained layer structure as mlp_kernels.hip (see there for
// the reference citations: lib/net/MLP.py:49-72, lib/net/HGPIFuNet.py:128-133,363), but every
// float32 product a*b is evaluated as three f16 MFMA products with f32 accumulation,
//       a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi,   x_hi = f16(x), x_lo = f16(x - x_hi),
// so both operands carry 22 significant bits and the dropped a_lo*b_lo term is 2^-22 relative:
// the result differs from the exact-f32 path by ~1e-6 of the activations' magnitude (measured in
// tests/test_gpu_parity.py against the float64 oracle; the north-star tolerance is 1e-4).
// v_mfma_f32_16x16x32_f16 retires 16 x 16 x 32 MACs in 16 cycles - the rate of v_mfma_f32_32x32x16_f16, which the chain
// used until the kernel was found power-bound: on real data the chip holds a higher clock on the small shape (DESIGN.md
// 4.4, tools/probes/mfma_shape.hip) - where v_mfma_f32_32x32x2_f32 needs 8 x 64 for a 32 x 32 x 16 block, so three of
// them are 5.3x faster than the exact-f32 MFMA chain.
//
// What changes structurally at that rate:
//  * weights can no longer stream from L2 per wavefront (85 B/clk/CU): a 512-thread workgroup
//    (8 waves x 32 points) shares them through LDS.  The packed hi/lo operand image (680 KB) is cut
//    into 20 chunks of 32-40 KB that are DMA'd global->LDS with global_load_lds_dwordx4 into a
//    double buffer; chunk k+1 lands while chunk k is being multiplied, one barrier per chunk.
//  * A operands are read with ds_read_b128 in [..][lane][16 B] order (conflict-free);
//    B operands are the previous layer's accumulators, LeakyReLU'd and split to hi/lo in
//    registers (v_cvt_pkrtz_f16_f32) - still no activation ever touches LDS or HBM.  One wave = 32 points =
//    two 16-point blocks; two finished 16-channel D tiles are the eight k-slots a lane holds of one K = 32
//    step, in the order sigma() below gives the packer.
//  * the raw inputs (layer 0, the input columns of layer 2: K = c0 <= 16) use half of an instruction's K, so two of
//    the three terms share one: [W_hi | W_hi] x [x_hi | x_lo], then [W_lo | 0] x [x_hi | x_lo] - two MFMAs, not three.
//  * per-layer power-of-two weight scales keep the lo parts out of the f16 subnormal range; they are
//    divided out (exactly) in the activation step.
#include "mlp_f16x3_device.h"

#include <cmath>
#include <cstring>

namespace icon {

template <bool MASK>
__global__ __launch_bounds__(kF16Block, 2) void k_mlp_f16x3(const float *__restrict__ X, int64_t N, float *__restrict__ out, MlpF16Dev w)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int64_t base = ((int64_t)blockIdx.x * (kF16Block / 64) + wave) * 32;
    // waves past the end still help with the DMA + barriers
    const int64_t pi0 = min(base + r, N - 1), pi1 = min(base + 16 + r, N - 1);
    const int64_t po = (g & 1) ? pi1 : pi0;      // the point this lane writes (lanes g < 2)

    // side arrays -> LDS once: no ordinary global load may sit between an LDS-DMA and its consumer
    // (vmcnt retires in order, so waiting for such a load would drain the DMA queue as well)
    issue_units(w.image, smem + kW0Off, kW0Bytes / 1024, wave, lane);     // resident layer-0 operands
    float *side = reinterpret_cast<float *>(smem + kSideOff);
    for (int i = threadIdx.x; i < kSideFloats; i += kF16Block) side[i] = w.side[i];
    const float *sb0 = side, *sb1 = side + 512, *sb2 = side + 768, *sw3 = side + kW3Float;

    float maskf = 1.0f;
    if (MASK) {
        const uint32_t code = (uint32_t)__float_as_int(X[po * kXRow + kCodeSlot]);
        maskf = (code & kCodeInCube) ? 1.0f : 0.0f;
        asm volatile("" : "+v"(maskf));
    }
    issue_chunk(w.image, smem, 0, wave, lane);
    __syncthreads();   // side arrays visible, chunk 0 landed (the barrier's release waits for the LDS-DMA)
    half8 xb[2];
    const float tail = load_x(X + pi0 * kXRow + 8 * (g & 1), X + pi1 * kXRow + 8 * (g & 1), sw3, w.c0, g, xb);

    f32x4 acc1[16][2];
#pragma unroll
    for (int m = 0; m < 16; ++m) acc1[m][0] = acc1[m][1] = *reinterpret_cast<const f32x4 *>(sb1 + m * 16 + 4 * g);

    // ---- layers 0 + 1: one chunk = 32 hidden channels ------------------------------------------
    half8 bh[2], bl[2];
    const LeakyK k0{w.inv0, w.p0, w.q0}, k1{w.inv1, w.p1, w.q1};
    layer01(smem, sb0, w.image, acc1, xb, k0, g, lane, wave, bh, bl);

    // ---- layer 2: K = 256 (registers) + 16 (raw input) ---------------------------------------------
    f32x4 acc2[8][2];
#pragma unroll
    for (int m2 = 0; m2 < 8; ++m2) acc2[m2][0] = acc2[m2][1] = *reinterpret_cast<const f32x4 *>(sb2 + m2 * 16 + 4 * g);
    activate_split(acc1[0][0], acc1[1][0], acc1[0][1], acc1[1][1], k1, bh, bl);
    l2_chunk<0>(smem, smem + kBufBytes, w.image, acc1, acc2, xb, k1, g, lane, wave, bh, bl);
    ICON_CHUNK_BARRIER();
    l2_chunk<1>(smem + kBufBytes, smem, w.image, acc1, acc2, xb, k1, g, lane, wave, bh, bl);
    ICON_CHUNK_BARRIER();
    l2_chunk<2>(smem, smem + kBufBytes, w.image, acc1, acc2, xb, k1, g, lane, wave, bh, bl);
    ICON_CHUNK_BARRIER();
    l2_chunk<3>(smem + kBufBytes, smem, w.image, acc1, acc2, xb, k1, g, lane, wave, bh, bl);

    // ---- layer 3 on the VALU (f32) ----------------------------------------------------------------
    float y2[2];
    {
        int tid_3 = threadIdx.x;
        asm volatile("" : "+v"(tid_3), "+v"(acc2[0][0]));     // layer 3's lane group, re-derived behind layer 2
        l3_sum(sw3, acc2, tail, LeakyK{w.inv2, w.p2, w.q2}, w.b3, (tid_3 >> 4) & 3, y2);
    }
    // the output index is re-derived behind the result: no 64-bit lane value lives across the MFMA body
    int tid_o = threadIdx.x;
    asm volatile("" : "+v"(tid_o), "+v"(y2[0]), "+v"(y2[1]));
    const int g_o = (tid_o >> 4) & 3;
    const int64_t o = ((int64_t)blockIdx.x * (kF16Block / 64) + (tid_o >> 6)) * 32 + 16 * g_o + (tid_o & 15);
    const float y = apply_last_op(g_o == 0 ? y2[0] : y2[1], w.last_op);
    if (g_o < 2 && o < N) out[o] = masked_result(y, MASK ? maskf != 0.0f : true, w.flag);
}

// ---------------------------------------------------------------------------------------------
// host side: operand image
// ---------------------------------------------------------------------------------------------
uint16_t f32_to_f16_rtn(float f)
{
    uint32_t x; memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (x > 0x7f800000u ? 0x200u : 0));
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                  // rounds to inf
    if (x < 0x33000001u) return (uint16_t)sign;                               // rounds to zero
    int e = (int)(x >> 23) - 127;
    uint32_t m = (x & 0x7fffffu) | 0x800000u;
    int shift;
    if (e < -14) { shift = 13 + (-14 - e); e = -15; } else shift = 13;
    uint32_t r = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (r & 1))) ++r;
    uint32_t out = (e == -15) ? r : (((uint32_t)(e + 15) << 10) + (r - 0x400u));  // carry propagates into exponent
    return (uint16_t)(sign | out);
}

float f16_to_f32(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const int e = (h >> 10) & 31;
    const uint32_t m = h & 0x3ffu;
    float v;
    if (e == 0) v = std::ldexp((float)m, -24);
    else if (e == 31) v = m ? NAN : INFINITY;
    else v = std::ldexp((float)(m | 0x400u), e - 25);
    return sign ? -v : v;
}

float pick_scale(const std::vector<float> &W)
{
    float mx = 0.f;
    for (float v : W) mx = std::max(mx, std::fabs(v));
    if (!(mx > 0.f) || !std::isfinite(mx)) return 1.0f;
    int e = (int)std::floor(std::log2(8192.0 / (double)mx));
    e = std::min(std::max(e, -60), 60);
    return std::ldexp(1.0f, e);
}

// Activation scale of a hidden layer (a power of two): the hidden activations are SPLIT into f16 pieces for the next
// GEMM, so the path has f16's range there - beyond 65504 the point is redone in f32 (k_rescue_*), but BELOW 2^-14 the
// pieces are f16 subnormals and lose their bits silently: a checkpoint whose BatchNorm gamma is 1e-4 with a next layer
// that compensates (the same function!) would come out with a few significant bits.  LeakyReLU is positively
// homogeneous, so a layer's activations may carry any factor A > 0 as long as the next layer's weights carry 1 / A:
// A is chosen from the weights alone so that the TYPICAL activation (RMS over the channels of the RMS pre-activation
// for inputs of the given mean squares) becomes 16 - 12 binades below the overflow point, 7 above the point where the
// lo piece starts to lose bits.  Exact (powers of two): for activations that were in range all along the results do
// not change by a bit.  out_ms[c] = mean square of channel c's pre-activation under that model.
float activation_scale(const std::vector<float> &W, const std::vector<float> &B, int cout, int cin, int n_used, const std::vector<double> &in_ms,
                       std::vector<double> &out_ms)
{
    out_ms.assign(cout, 0.0);
    double acc = 0.0;
    for (int c = 0; c < cout; ++c) {
        double s = (double)B[c] * B[c];
        for (int k = 0; k < n_used; ++k) s += (double)W[(size_t)c * cin + k] * W[(size_t)c * cin + k] * in_ms[k];
        out_ms[c] = s; acc += s;
    }
    const double typical = std::sqrt(acc / std::max(cout, 1));
    if (!(typical > 0.0) || !std::isfinite(typical)) return 1.0f;
    int e = (int)std::lround(std::log2(16.0 / typical));
    e = std::min(std::max(e, -60), 60);
    return std::ldexp(1.0f, e);
}

// W: folded float32 weights of the four layers (row-major [cout][cin]), B: folded biases.  Host only: the operand image
// (kImageBytes), the side arrays (kSideFloats), inv[3] = what an accumulator of layers 0..2 is multiplied by before
// LeakyReLU, scales[5] = weight scales s0, s1, s2 and activation scales A0, A1.
void mlp_pack_f16x3_host(int c0, const std::vector<std::vector<float>> &W, const std::vector<std::vector<float>> &B,
                         std::vector<uint16_t> &img, std::vector<float> &side, float inv[3], float scales[5])
{
    // activation scales A0, A1 of the two hidden layers whose outputs are split (layer 2's go to the f32 VALU layer as they
    // are); inputs of layer 0 taken as unit mean square.  The next layer's weights carry 1 / A (exact).
    std::vector<double> ms_in(c0, 1.0), ms0, ms1;
    const float A0 = activation_scale(W[0], B[0], 512, c0, c0, ms_in, ms0);
    std::vector<float> W1(W[1]);
    for (float &v : W1) v /= A0;
    const float A1 = activation_scale(W[1], B[1], 256, 512, 512, ms0, ms1);
    const int ci2_ = 256 + c0;
    std::vector<float> W2(W[2]);
    for (int c = 0; c < 128; ++c)
        for (int k = 0; k < 256; ++k) W2[(size_t)c * ci2_ + k] /= A1;           // the raw-input columns [256, 256 + c0) are not activations
    const float s0 = pick_scale(W[0]), s1 = pick_scale(W1), s2 = pick_scale(W2);
    img.assign(kImageBytes / 2, 0);
    // K permutation: k-slot k = 8g + e of a K = 32 step is, of the 32 channels of the two D tiles it is built from,
    // channel 4g + e of the first (e < 4) or 16 + 4g + (e - 4) of the second (mlp_f16x3_device.h)
    auto sigma = [](int k) { const int g = k >> 3, e = k & 7; return e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4); };
    // hi into half index `at`, lo into `at + lo_step`
    auto put = [&](size_t at, size_t lo_step, float wv, float scale) {
        const float ws = wv * scale;
        const uint16_t hi = f32_to_f16_rtn(ws);
        img[at] = hi;
        img[at + lo_step] = f32_to_f16_rtn(ws - f16_to_f32(hi));
    };
    const int ci2 = 256 + c0;
    // hidden k-steps: one 1-KiB slot = [lane 64][8 halves], lane (r, g) = row r, halves k = 8g..8g+7; hi in slot 2m, lo in 2m + 1
    parallel_for(64, [&](int lane) {       // every lane owns its own 16-byte column of each slot
        const int r = lane & 15, g = lane >> 4;
        for (int e = 0; e < 8; ++e) {
            const int ch = sigma(8 * g + e);
            const size_t col = (size_t)lane * 8 + e;
            for (int c = 0; c < 16; ++c)                 // layer 1, chunk c = k-step c: output tiles m = 0..15
                for (int mm = 0; mm < 16; ++mm)
                    put(((size_t)chunk_offset(c) + 2 * mm) * 512 + col, 512, W1[(size_t)(16 * mm + r) * 512 + 32 * c + ch], s1);
            for (int q = 0; q < 4; ++q)                  // layer 2, chunk 16+q = k-steps 2q, 2q+1: output tiles m2 = 0..7
                for (int mm = 0; mm < 2; ++mm)
                    for (int m2 = 0; m2 < 8; ++m2)
                        put(((size_t)chunk_offset(16 + q) + (mm * 8 + m2) * 2) * 512 + col, 512,
                            W2[(size_t)(16 * m2 + r) * ci2 + 32 * (2 * q + mm) + ch], s2);
        }
    });
    // raw-input tiles: 1 KiB = [W_hi: lane (r, g1) x 8 halves][W_lo: the same], k = 8 g1 + e < c0.  The kernel reads
    // [W_hi | W_hi] and [W_lo | 0] from them (two of the three terms per instruction): layer 0 (W0 region, tile = 16
    // hidden channels) and the raw-input columns of layer 2 (behind the hidden k-steps of chunk 16)
    for (int g1 = 0; g1 < 2; ++g1)
        for (int r = 0; r < 16; ++r)
            for (int e = 0; e < 8; ++e) {
                const int k = 8 * g1 + e;
                const size_t col = (size_t)(g1 * 16 + r) * 8 + e;
                for (int ct = 0; ct < 32; ++ct)
                    put((size_t)ct * 512 + col, 256, k < c0 ? W[0][(size_t)(16 * ct + r) * c0 + k] : 0.f, s0);
                for (int m2 = 0; m2 < 8; ++m2)
                    put(((size_t)chunk_offset(16) + 32 + m2) * 512 + col, 256, k < c0 ? W2[(size_t)(16 * m2 + r) * ci2 + 256 + k] : 0.f, s2);
            }
    // f32 side arrays: scaled biases in channel order (accumulator initial values: a lane reads channels 4g..4g+3 of a tile),
    // the last layer per lane group, 16 bytes of zeros
    side.assign(kSideFloats, 0.f);
    float *b0 = side.data(), *b1 = b0 + 512, *b2 = b1 + 256, *w3 = side.data() + kW3Float;
    for (int c = 0; c < 512; ++c) b0[c] = B[0][c] * s0;
    for (int c = 0; c < 256; ++c) b1[c] = B[1][c] * s1;
    for (int c = 0; c < 128; ++c) b2[c] = B[2][c] * s2;
    for (int g = 0; g < 4; ++g) {
        for (int m2 = 0; m2 < 8; ++m2)
            for (int j = 0; j < 4; ++j) w3[g * kW3Stride + 4 * m2 + j] = W[3][16 * m2 + 4 * g + j];
        for (int s = 0; s < 8; ++s) w3[g * kW3Stride + 32 + s] = (s + 8 * (g & 1) < c0) ? W[3][128 + s + 8 * (g & 1)] : 0.f;
    }
    // what an accumulator is multiplied by before LeakyReLU: 1 / weight scale, times the activation scale of the layer
    inv[0] = A0 / s0; inv[1] = A1 / s1; inv[2] = 1.0f / s2;
    scales[0] = s0; scales[1] = s1; scales[2] = s2; scales[3] = A0; scales[4] = A1;
}

int mlp_pack_f16x3(icon_mlp *m, const std::vector<std::vector<float>> &W, const std::vector<std::vector<float>> &B,
                   hipStream_t st)
{
    std::vector<uint16_t> img;
    std::vector<float> side;
    float scales[5];
    mlp_pack_f16x3_host(m->c0, W, B, img, side, m->f16_inv, scales);
    const size_t side_bytes = side.size() * sizeof(float);
    ICON_HIP(hipMalloc((void **)&m->d_f16, kImageBytes + side_bytes));
    ICON_HIP(hipMemcpyAsync(m->d_f16, img.data(), kImageBytes, hipMemcpyHostToDevice, st));
    ICON_HIP(hipMemcpyAsync(m->d_f16 + kImageBytes, side.data(), side_bytes, hipMemcpyHostToDevice, st));
    ICON_HIP(hipStreamSynchronize(st));
    return ICON_OK;
}

int mlp_launch_f16x3(const icon_mlp *mlp, const float *d_x, int64_t N, float *d_out, bool mask, hipStream_t st)
{
    if (N <= 0) return ICON_OK;
    MlpF16Dev w;
    w.image = mlp->d_f16;
    w.side = reinterpret_cast<const float *>(mlp->d_f16 + kImageBytes);
    w.b3 = mlp->b3; w.inv0 = mlp->f16_inv[0]; w.inv1 = mlp->f16_inv[1]; w.inv2 = mlp->f16_inv[2]; w.c0 = mlp->c0; w.last_op = mlp->last_op;
    w.flag = reinterpret_cast<int *>(mlp->d_blob + mlp->off_flag);
    w.p0 = 0.505f * w.inv0; w.q0 = 0.495f * w.inv0; w.p1 = 0.505f * w.inv1; w.q1 = 0.495f * w.inv1; w.p2 = 0.505f * w.inv2; w.q2 = 0.495f * w.inv2;
    const int64_t nb = (N + kF16Pts - 1) / kF16Pts;
    ICON_ARG(nb < (1ll << 31), "mlp: N too large for one launch");
    int rc = once_per_device(6, [] {       // per device: a process may drive several (common.h)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_mlp_f16x3<true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
        return e != hipSuccess ? e : hipFuncSetAttribute(reinterpret_cast<const void *>(k_mlp_f16x3<false>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    });
    if (rc) return rc;
    rc = mlp_flag_reset(mlp, st);
    if (rc) return rc;
    if (mask) hipLaunchKernelGGL(k_mlp_f16x3<true>, dim3((unsigned)nb), dim3(kF16Block), kLdsBytes, st, d_x, N, d_out, w);
    else      hipLaunchKernelGGL(k_mlp_f16x3<false>, dim3((unsigned)nb), dim3(kF16Block), kLdsBytes, st, d_x, N, d_out, w);
    ICON_HIP(hipGetLastError());
    return mlp_rescue_rows(mlp, d_x, N, d_out, st);
}

}  // namespace icon

// host only (no device is touched): the packed operand image of a folded network of input width c0 <= 16, for tests that
// read it back in MFMA order.  h_W / h_b: the four layers, [cout][cin] row-major with cin = c0, 512, 256 + c0, 128 + c0.
extern "C" int icon_debug_mlp_pack_f16x3(int c0, const float *const *h_W, const float *const *h_b, uint16_t *img, float *side,
                                         float *inv, float *scales)
{
    ICON_ARG(h_W && h_b && img && side && inv && scales && c0 >= 1 && c0 <= 16, "icon_debug_mlp_pack_f16x3: bad argument");
    const int cin[4] = {c0, 512, 256 + c0, 128 + c0}, cout[4] = {512, 256, 128, 1};
    std::vector<std::vector<float>> W(4), B(4);
    for (int l = 0; l < 4; ++l) {
        ICON_ARG(h_W[l] && h_b[l], "icon_debug_mlp_pack_f16x3: null layer");
        W[l].assign(h_W[l], h_W[l] + (size_t)cout[l] * cin[l]);
        B[l].assign(h_b[l], h_b[l] + cout[l]);
    }
    std::vector<uint16_t> im;
    std::vector<float> sd;
    icon::mlp_pack_f16x3_host(c0, W, B, im, sd, inv, scales);
    memcpy(img, im.data(), icon::kImageBytes);
    memcpy(side, sd.data(), sd.size() * sizeof(float));
    return ICON_OK;
}

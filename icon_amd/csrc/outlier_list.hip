// outlier_list.hip - the outlier sign list of a call in reference cmap mode (lib/net/HGPIFuNet.py:298-305): its kernels
// (count -> scan -> compact in the linear point order of the call, the packed message of the multi-GPU exchange and the
// prefix of the gathered messages' headers, the cmap patch of the materialising paths) and its host side.  The rule itself -
// where the list lives, how a sign is decoded, cmap[j][k] = s[(3j + k) mod K] - is sign_list_device.h, shared with the
// fused kernel.
#pragma clang fp contract(off)

#include "sign_list_device.h"
#include "scan_device.h"

#include <algorithm>

namespace icon {

__global__ __launch_bounds__(kScanBlock) void k_outlier_count(const uint8_t *__restrict__ code8, int64_t N, int32_t *block_counts)
{
    __shared__ int wsum[kScanBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kScanBlock + threadIdx.x;
    const bool o = (i < N) && (code8[i] & kCodeOutlier);
    const unsigned long long b = __ballot(o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kScanBlock / 64; ++w) s += wsum[w];
        block_counts[blockIdx.x] = s;
    }
}

// Exclusive scan of the per-tile outlier counts (66,308 entries for a 257^3 call; int64 offsets: a 513^3
// lattice has 1.35e8 points) in two coalesced passes: k_scan_local scans 1,024 consecutive counts per
// workgroup (scan_device.h: wave shuffles + one LDS hop) and records the chunk total, k_scan_apply adds the sum of the
// preceding chunk totals.  (A single workgroup walking 65 strided entries per thread was latency-bound:
// 0.12 ms - more than k_sign, the count and the compaction together.)
// n_points_dev (adaptive levels): the call's size lives on the device - n = its number of 256-point blocks
__global__ __launch_bounds__(1024) void k_scan_local(const int32_t *__restrict__ counts, int64_t n, int32_t *__restrict__ local, int64_t *__restrict__ part,
                                                     const int *__restrict__ n_points_dev)
{
    __shared__ int64_t wtot[16];
    if (n_points_dev) n = ((int64_t)*n_points_dev + kScanBlock - 1) / kScanBlock;
    const int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    const int64_t v = (i < n) ? counts[i] : 0;
    int64_t total;
    const int64_t ex = block_excl_scan<16>(v, wtot, total);
    if (i < n) local[i] = (int32_t)ex;
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void k_scan_apply(const int32_t *__restrict__ local, const int64_t *__restrict__ part, int64_t nchunks, int64_t n,
                                                     int64_t *__restrict__ offsets, int64_t *__restrict__ total, const int *__restrict__ n_points_dev)
{
    __shared__ int64_t wtot[16];
    if (n_points_dev) n = ((int64_t)*n_points_dev + kScanBlock - 1) / kScanBlock;
    // sum of the chunk totals before this chunk (and of all chunks, for *total): nchunks <= a few hundred
    int64_t before = 0, all = 0;
    for (int64_t k = threadIdx.x; k < nchunks; k += 1024) { const int64_t t = part[k]; all += t; if (k < blockIdx.x) before += t; }
    int64_t sum_all, sum_before;
    (void)block_excl_scan<16>(all, wtot, sum_all);
    __syncthreads();
    (void)block_excl_scan<16>(before, wtot, sum_before);
    const int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    if (i < n) offsets[i] = sum_before + local[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) *total = sum_all;
}

__device__ __forceinline__ int64_t outlier_rank(bool o, const int64_t *block_offsets, int *wsum)
{
    // exclusive rank of this thread's outlier among the outliers of the call (linear order)
    const unsigned long long b = __ballot(o);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wsum[w] = __popcll(b);
    __syncthreads();
    int before = 0;
    for (int k = 0; k < w; ++k) before += wsum[k];
    before += __popcll(b & ((1ull << lane) - 1ull));
    return block_offsets[blockIdx.x] + before;
}

__global__ __launch_bounds__(kScanBlock) void k_outlier_compact(const uint8_t *__restrict__ code8, int64_t N,
                                                                const int64_t *block_offsets, int8_t *signs, const int *__restrict__ n_dev)
{
    __shared__ int wsum[kScanBlock / 64];
    if (n_dev) { N = *n_dev; if ((int64_t)blockIdx.x * kScanBlock >= N) return; }
    const int64_t i = (int64_t)blockIdx.x * kScanBlock + threadIdx.x;
    const uint32_t code = (i < N) ? code8[i] : 0u;
    const bool o = code & kCodeOutlier;
    const int64_t r = outlier_rank(o, block_offsets, wsum);
    if (o) signs[r] = (int8_t)code_sign(code);
}

// scan + compact in ONE launch for calls of few blocks (the levels of the reference's schedule: 20,000 - 60,000 points, 80 - 250
// blocks): every workgroup sums the counts before its own block itself (a few hundred ints from L2) instead of waiting for two
// scan launches - three launches of ~5 us each were the launch floor, not work.  O(blocks^2) reads: the host picks it by size.
__global__ __launch_bounds__(kScanBlock) void k_outlier_small(const int32_t *__restrict__ counts, const uint8_t *__restrict__ code8, int64_t N,
                                                              int64_t *__restrict__ block_offsets, int64_t *__restrict__ total, int8_t *__restrict__ signs,
                                                              const int *__restrict__ n_dev)
{
    __shared__ int wsum[kScanBlock / 64];
    __shared__ int64_t red[2][kScanBlock / 64];
    if (n_dev) N = *n_dev;
    const int64_t nblk = (N + kScanBlock - 1) / kScanBlock;
    if (blockIdx.x == 0 && threadIdx.x == 0 && nblk == 0) *total = 0;
    if ((int64_t)blockIdx.x >= nblk) return;
    int64_t before = 0, all = 0;
    const bool want_all = blockIdx.x == 0;                       // block 0 also publishes the call's total
    for (int64_t k = threadIdx.x; k < (want_all ? nblk : (int64_t)blockIdx.x); k += kScanBlock) { const int64_t t = counts[k]; all += t; if (k < blockIdx.x) before += t; }
    for (int d = 32; d >= 1; d >>= 1) { before += __shfl_xor(before, d); all += __shfl_xor(all, d); }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { red[0][w] = before; red[1][w] = all; }
    __syncthreads();
    before = 0; all = 0;
    for (int k = 0; k < kScanBlock / 64; ++k) { before += red[0][k]; all += red[1][k]; }
    if (threadIdx.x == 0) { block_offsets[blockIdx.x] = before; if (want_all) *total = all; }
    const int64_t i = (int64_t)blockIdx.x * kScanBlock + threadIdx.x;
    const uint32_t code = (i < N) ? code8[i] : 0u;
    const bool o = code & kCodeOutlier;
    const unsigned long long b = __ballot(o);
    if (lane == 0) wsum[w] = __popcll(b);
    __syncthreads();
    int64_t r = before + __popcll(b & ((1ull << lane) - 1ull));
    for (int k = 0; k < w; ++k) r += wsum[k];
    if (o) signs[r] = (int8_t)code_sign(code);
}
constexpr int64_t kSmallListBlocks = 16384;      // up to this many blocks (4.2 M points) the one-launch list; worst case 1 GB of L2 reads

// the cmap of every outlier row of the materialising paths: outlier_cmap of its rank among the call's outliers, wherever the
// call's sign list is (SEG: resolve_signs ran k_seg_offsets first).  K, the rank offset and the mode are wave-uniform.
__global__ __launch_bounds__(kScanBlock) void k_outlier_patch(float *__restrict__ X, const uint8_t *__restrict__ code8, int64_t N, int cmap_slot,
                                                              const int64_t *block_offsets, SignSrc sg)
{
    __shared__ int wsum[kScanBlock / 64];
    int64_t K, rank0;
    sign_list_extent(sg, K, rank0);
    const int64_t i = (int64_t)blockIdx.x * kScanBlock + threadIdx.x;
    const uint32_t code = (i < N) ? code8[i] : 0u;
    const bool o = code & kCodeOutlier;
    const int64_t j = rank0 + outlier_rank(o, block_offsets, wsum);
    if (o && K > 0) {
        float c[3];
        outlier_cmap(sg, K, j, c);
        float *row = X + i * kXRow + cmap_slot;
        row[0] = c[0]; row[1] = c[1]; row[2] = c[2];
    }
}

// sign message of the multi-GPU exchange: [int64 K][K signs, 2 bits each (sign + 1), four to a byte, zero padded]
__global__ __launch_bounds__(256) void k_pack_signs(const int8_t *__restrict__ signs, const int64_t *__restrict__ k_dev, uint8_t *__restrict__ msg, int64_t cap_bytes)
{
    const int64_t K = *k_dev;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) *reinterpret_cast<int64_t *>(msg) = K;
    if (t >= cap_bytes || 4 * t >= K) return;
    uint32_t b = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * t + j < K) b |= (uint32_t)(signs[4 * t + j] + 1) << (2 * j);
    msg[8 + t] = (uint8_t)b;
}

// exclusive prefix of the per-rank outlier counts found in the headers of the gathered messages
__global__ void k_seg_offsets(const int8_t *__restrict__ gathered, int64_t stride, int world, int64_t *__restrict__ seg)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t a = 0;
    for (int r = 0; r < world; ++r) { seg[r] = a; a += *reinterpret_cast<const int64_t *>(gathered + (int64_t)r * stride); }
    seg[world] = a;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// count + scan + compact over the codes of points [0, N): fills w->d_block_offsets, w->d_total, and `signs`.
// `counted`: k_sign already left the outlier count of every 256-point block in d_block_counts.
// n_dev (adaptive levels; counted): the call's size lives on the device, *n_dev <= N - a few percent of N, so the one-launch
// list serves up to kSmallListBlocks blocks (see k_outlier_small) where a call of host-known size takes it up to 1,024.
int outlier_list(icon_work *w, int64_t N, const int *n_dev, int8_t *signs, bool counted, hipStream_t st)
{
    const int64_t nblk = (N + kScanBlock - 1) / kScanBlock;
    if (!counted) hipLaunchKernelGGL(k_outlier_count, dim3((unsigned)nblk), dim3(kScanBlock), 0, st, w->d_code8, N, w->d_block_counts);
    const bool one = nblk <= (n_dev ? kSmallListBlocks : 1024);
    if (one) {
        hipLaunchKernelGGL(k_outlier_small, dim3((unsigned)std::max<int64_t>(nblk, 1)), dim3(kScanBlock), 0, st, w->d_block_counts, w->d_code8, N, w->d_block_offsets, w->d_total,
                           signs, n_dev);
    } else {
        const int64_t nchunks = (nblk + 1023) / 1024;
        hipLaunchKernelGGL(k_scan_local, dim3((unsigned)nchunks), dim3(1024), 0, st, w->d_block_counts, nblk, w->d_scan_local, w->d_scan_part, n_dev);
        hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nchunks), dim3(1024), 0, st, w->d_scan_local, w->d_scan_part, nchunks, nblk, w->d_block_offsets, w->d_total, n_dev);
        hipLaunchKernelGGL(k_outlier_compact, dim3((unsigned)nblk), dim3(kScanBlock), 0, st, w->d_code8, N, w->d_block_offsets, signs, n_dev);
    }
    ICON_HIP(hipGetLastError());
    if (!n_dev) debug_sync(one ? "outlier list (one launch)" : "outlier scan + compact", st);
    return ICON_OK;
}

// this call's own list is the whole list (`needs`: the call is in reference cmap mode with a cmap channel)
SignSrc self_signs(const icon_work *work, bool needs)
{
    SignSrc sg{};
    sg.mode = needs ? kSignSelf : kSignNone;
    sg.list = work->d_signs; sg.k_dev = work->d_total;
    return sg;
}

// what a launch that reads `sg` needs on the device first.  SEG: the prefix of the gathered messages' counts in work->d_seg
int resolve_signs(const icon_work *work, SignSrc *sg, hipStream_t st)
{
    if (sg->mode != kSignSeg) return ICON_OK;
    if (!work->d_seg) return fail(ICON_ERR_STATE, "sign list: segment offsets buffer missing");
    hipLaunchKernelGGL(k_seg_offsets, dim3(1), dim3(64), 0, st, sg->gathered, sg->stride, sg->world, work->d_seg);
    sg->seg = work->d_seg;
    return ICON_OK;
}

// the reference-mode cmap of the outlier rows among w->d_x[0, N) (slots cmap_slot .. cmap_slot + 2), behind outlier_list
int outlier_patch(icon_work *w, int64_t N, int cmap_slot, const SignSrc &sg, hipStream_t st)
{
    if (sg.mode == kSignNone || (sg.mode == kSignGlobal && sg.k_host <= 0)) return ICON_OK;
    SignSrc s = sg;
    const int rc = resolve_signs(w, &s, st);
    if (rc) return rc;
    const int64_t nblk = (N + kScanBlock - 1) / kScanBlock;
    hipLaunchKernelGGL(k_outlier_patch, dim3((unsigned)nblk), dim3(kScanBlock), 0, st, w->d_x, w->d_code8, N, cmap_slot, w->d_block_offsets, s);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

// the call's message of the multi-GPU exchange (k_pack_signs writes it, sign_at reads it): `signs` and w->d_total -> d_msg,
// which holds `cap` packed bytes behind its header
int pack_sign_message(const icon_work *w, const int8_t *signs, void *d_msg, int64_t cap, hipStream_t st)
{
    const int64_t nb = (std::max<int64_t>(cap, 1) + 255) / 256;
    hipLaunchKernelGGL(k_pack_signs, dim3((unsigned)nb), dim3(256), 0, st, signs, w->d_total, (uint8_t *)d_msg, cap);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

}  // namespace icon

// compact_device.h - the order-preserving compaction of a submesh, as clean_mesh.hip and garment.hip emit theirs: the caller's
// own rule writes a flag per face and per vertex (a kept face names existing vertices only, and flags all three) and the faces'
// count per kCompactBlock entries (compact_count); then, here: the vertices' counts, one scan of both count arrays, the kept
// vertices in their order with their new indices in `remap`, the kept faces in their order, renumbered.  No atomics: equal
// bytes from run to run.  Workgroups of kCompactBlock threads throughout, one entry per thread.  Everything lives in the
// including file's anonymous namespace.
#pragma once

#include "scan_device.h"

namespace icon {
namespace {

constexpr int kCompactBlock = 256;        // entries per count / offset
constexpr int kCompactRound = 8192;       // counts per round of k_compact_scan (1,024 threads x 8): more than that many blocks carry a total over

// blk[this workgroup] = the number of its threads with `keep` set
__device__ __forceinline__ void compact_count(bool keep, int *blk)
{
    __shared__ int ws[kCompactBlock / 64];
    const unsigned long long b = __ballot(keep);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// the number of threads with `keep` set before this one in the workgroup
__device__ __forceinline__ int compact_rank(bool keep)
{
    __shared__ int ws[kCompactBlock / 64];
    const unsigned long long b = __ballot(keep);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) ws[w] = __popcll(b);
    __syncthreads();
    int k = __popcll(b & ((1ull << lane) - 1ull));
    for (int q = 0; q < w; ++q) k += ws[q];
    return k;
}

__global__ __launch_bounds__(kCompactBlock) void k_compact_count_v(const uint8_t *__restrict__ flag_v, int64_t V, int *__restrict__ blk_v)
{
    const int64_t v = (int64_t)blockIdx.x * kCompactBlock + threadIdx.x;
    compact_count(v < V && flag_v[v], blk_v);
}

// exclusive scan of the block counts, in place (one workgroup per array; eight counts per thread and round); workgroup 0: the
// vertices, 1: the faces; totals[0], totals[1]: how many are kept
template <class TT>
__global__ __launch_bounds__(1024) void k_compact_scan(int *blk_v, int64_t V, int *blk_f, int64_t F, TT *totals)
{
    __shared__ int wtot[16];
    int *cnt = blockIdx.x == 0 ? blk_v : blk_f;
    const int nb = (int)(((blockIdx.x == 0 ? V : F) + kCompactBlock - 1) / kCompactBlock);
    int carry = 0;
    for (int base = 0; base < nb; base += kCompactRound) {
        __syncthreads();                                        // (the previous round's wtot has been read)
        carry += block_scan_tile<16, 8>(cnt, cnt, base + (int)threadIdx.x * 8, nb, carry, wtot);
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// out_ids: the old index of every emitted vertex, or null
__global__ __launch_bounds__(kCompactBlock) void k_compact_emit_v(const float *__restrict__ verts, const uint8_t *__restrict__ flag_v, int64_t V,
                                                                  const int *__restrict__ blk_v, int *__restrict__ remap,
                                                                  float *__restrict__ out_verts, int32_t *__restrict__ out_ids)
{
    const int64_t v = (int64_t)blockIdx.x * kCompactBlock + threadIdx.x;
    const bool keep = v < V && flag_v[v];
    const int64_t k = blk_v[blockIdx.x] + compact_rank(keep);
    if (!keep) return;
    remap[v] = (int)k;
    out_verts[3 * k] = verts[3 * v]; out_verts[3 * k + 1] = verts[3 * v + 1]; out_verts[3 * k + 2] = verts[3 * v + 2];
    if (out_ids) out_ids[k] = (int32_t)v;
}

template <class IT>
__device__ __forceinline__ void compact_emit_faces(const IT *faces, const uint8_t *flag_f, int64_t F, const int *blk_f, const int *remap,
                                                   int32_t *out_faces)
{
    const int64_t f = (int64_t)blockIdx.x * kCompactBlock + threadIdx.x;
    const bool keep = f < F && flag_f[f];
    const int64_t k = blk_f[blockIdx.x] + compact_rank(keep);
    if (!keep) return;
    out_faces[3 * k] = remap[faces[3 * f]]; out_faces[3 * k + 1] = remap[faces[3 * f + 1]]; out_faces[3 * k + 2] = remap[faces[3 * f + 2]];
}
template <class IT>
__global__ __launch_bounds__(kCompactBlock) void k_compact_emit_f(const IT *__restrict__ faces, const uint8_t *__restrict__ flag_f, int64_t F,
                                                                  const int *__restrict__ blk_f, const int *__restrict__ remap,
                                                                  int32_t *__restrict__ out_faces)
{
    compact_emit_faces(faces, flag_f, F, blk_f, remap, out_faces);
}

}  // namespace
}  // namespace icon

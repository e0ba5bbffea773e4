// scan_device.h - the workgroup exclusive scan every count -> offset pass of the library uses, stated once: a wave inclusive scan
// through __shfl_up, one LDS word per wave, a sum over the waves before.  T is any type with + and - that __shfl_up moves: int,
// int64_t, and the unsigned 64-bit word in which marching cubes packs two 32-bit counts (nothing here assumes a sign).
//
// The barrier contract: block_excl_scan holds ONE barrier, between the waves' stores to s_w and the loads of them.  Nothing
// orders those loads against the NEXT stores to s_w: a caller that scans again over the same words - a loop over rounds, two
// scans in a row - places a __syncthreads() of its own before the next call; a caller that scans once needs none.
#pragma once

#include "common.h"

namespace icon {

template <class T>
__device__ __forceinline__ T wave_incl_scan(T v)
{
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) { const T up = __shfl_up(v, d); if (lane >= d) v += up; }
    return v;
}

// exclusive prefix of v over the workgroup's NW wavefronts; s_w: NW words of LDS; total: the workgroup's sum
template <int NW, class T>
__device__ __forceinline__ T block_excl_scan(T v, T *s_w, T &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T incl = wave_incl_scan(v);
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    T ex = incl - v, all = 0;                                   // the prefix inside the wave, then the waves before
#pragma unroll
    for (int q = 0; q < NW; ++q) { const T t = s_w[q]; ex += q < w ? t : T(0); all += t; }
    total = all;
    return ex;
}

// one tile of N consecutive items per thread: out[i] = carry + the sum of the tile's items before i, for the thread's items
// i0 .. i0 + N - 1 below n (in == out is fine: a thread reads its items before it writes them); returns the tile's sum
template <int NW, int N, class T>
__device__ __forceinline__ T block_scan_tile(const T *in, T *out, int64_t i0, int64_t n, T carry, T *s_w)
{
    T v[N], sum = 0, total;
#pragma unroll
    for (int k = 0; k < N; ++k) { v[k] = i0 + k < n ? in[i0 + k] : T(0); sum += v[k]; }
    T run = carry + block_excl_scan<NW>(sum, s_w, total);
#pragma unroll
    for (int k = 0; k < N; ++k) { if (i0 + k < n) out[i0 + k] = run; run += v[k]; }
    return total;
}

}  // namespace icon

// sign_list_device.h - the outlier sign list of a call in reference cmap mode (lib/net/HGPIFuNet.py:298-305), stated once:
// where the list lives (SignSrc), how a sign is decoded from a code byte and from a packed message, and the rule that
// couples every outlier of the call to it - outlier j of the call's K outliers gets cmap[j][k] = s[(3j + k) mod K].
// Read by the fused kernel (fused_f16x3.hip: icon_row) and by the patch kernel of the materialising paths
// (outlier_list.hip, which also holds the list's kernels and the one writer of the packed message, k_pack_signs).
#pragma once

#include "common.h"

namespace icon {

// where the outlier signs of the whole call are
enum { kSignNone = 0, kSignSelf = 1, kSignGlobal = 2, kSignSeg = 3 };
// (part of the kernel argument FusedGeom: the layout is device code)
struct SignSrc {
    int mode;
    const int8_t *list;          // SELF / GLOBAL: the outlier signs of the call in point order
    const int64_t *k_dev;        // SELF: device scalar K
    int64_t k_host, rank_offset; // GLOBAL: K and the number of outliers in lower slabs
    const int8_t *gathered;      // SEG: all_gather output, message r = [int64 count][signs, 2 bits each: sign + 1]
    int64_t stride;
    int world, rank;
    const int64_t *seg;          // SEG: [world + 1] exclusive prefix of the counts (k_seg_offsets; set by resolve_signs)
};

// sign(sdf) of an outlier, -1 / 0 / +1, from its code byte
__device__ __forceinline__ int code_sign(uint32_t code)
{
    return (int)((code >> kCodeSignShift) & 3u) - 1;
}

// the sign-list geometry of a launch: K outliers in the call, rank0 = rank of this launch's first
__device__ __forceinline__ void sign_list_extent(const SignSrc &sg, int64_t &K, int64_t &rank0)
{
    K = 0; rank0 = 0;
    if (sg.mode == kSignSelf) K = *sg.k_dev;
    else if (sg.mode == kSignGlobal) { K = sg.k_host; rank0 = sg.rank_offset; }
    else if (sg.mode == kSignSeg) { K = sg.seg[sg.world]; rank0 = sg.seg[sg.rank]; }
}

// entry mm of the list.  SEG mode: `seg` = exclusive prefix of the per-rank counts (world + 1 entries, global memory written by
// k_seg_offsets, read here through wave-uniform scalar loads): segment of mm = number of boundaries <= mm
__device__ __forceinline__ float sign_at(const SignSrc &sg, int64_t mm)
{
    if (sg.mode == kSignSeg) {
        int r = 0;
        int64_t base = 0;
        for (int q = 1; q < sg.world; ++q) {
            const int64_t o = sg.seg[q];
            const bool ge = mm >= o;
            r += ge ? 1 : 0;
            base = ge ? o : base;
        }
        const int64_t e = mm - base;                             // 2 bits per sign (sign + 1), four to a byte
        const uint32_t byte = (uint8_t)sg.gathered[(int64_t)r * sg.stride + 8 + (e >> 2)];
        return (float)((int)((byte >> (2 * (int)(e & 3))) & 3u) - 1);
    }
    return (float)sg.list[mm];
}

// the cmap of outlier j (its rank among the K > 0 outliers of the call): c[k] = s[(3j + k) mod K]
__device__ __forceinline__ void outlier_cmap(const SignSrc &sg, int64_t K, int64_t j, float c[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int64_t mm = 3 * j + k;             // j < K  =>  mm < 3K
        if (mm >= K) mm -= K;
        if (mm >= K) mm -= K;
        c[k] = sign_at(sg, mm);
    }
}

}  // namespace icon

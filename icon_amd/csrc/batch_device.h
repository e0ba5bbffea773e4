// batch_device.h - per-subject lookups of a batched point-mode call (icon_query_points_batch): point i of the call belongs to
// subject b = i / n; its calibration, mesh and feature planes come from the BatchDev descriptor (common.h).  The one place that
// says how: read by the batched instantiations of the point-mode kernel templates (query_device.h: k_nearest_coop, k_features;
// fused_f16x3.hip: k_sign_wide, build_row of k_fused_f16x3 / k_rescue_fused) and by k_nearest_batch (batch_query.hip).
#pragma once
#pragma clang fp contract(off)

#include "geom_device.h"

namespace icon {

// per lane (subjects may differ within a wave: tiles straddle subject boundaries when n is not a multiple of the tile)
__device__ __forceinline__ Calib batch_calib(const BatchDev &bd, int64_t b)
{
    Calib c;
    const float *q = bd.calibs + 12 * b;
#pragma unroll
    for (int k = 0; k < 12; ++k) c.m[k] = q[k];
    c.d = nullptr;
    return c;
}

__device__ __forceinline__ FeatDev batch_feat(const FeatDev &f, const BatchDev &bd, int64_t b)
{
    FeatDev g = f;
    g.planes = f.planes + b * bd.plane_stride;
    g.vol = f.vol + b * bd.vol_stride;        // (no volume: null, stride 0)
    return g;
}

// wave-uniform subject (the search kernels: every wave holds points of one subject): scalar loads, the descriptors in SGPRs
// as the unbatched kernels have them
__device__ __forceinline__ MeshDev batch_mesh_uniform(const BatchDev &bd, int b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(4))) const MeshDev cmesh;
    return *(cmesh *)(uintptr_t)(bd.meshes + b);
#else
    return bd.meshes[b];
#endif
}

__device__ __forceinline__ Calib batch_calib_uniform(const BatchDev &bd, int b)
{
    Calib c;
    cfloat *q = as_const(bd.calibs + 12 * (int64_t)b);
#pragma unroll
    for (int k = 0; k < 12; ++k) c.m[k] = q[k];
    c.d = nullptr;
    return c;
}

}  // namespace icon

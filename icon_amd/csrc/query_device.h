// query_device.h - the point-mode kernels of query_kernels.hip that the batched call (batch_query.hip) instantiates too: "batched
// or not" is a template parameter.  The unbatched instantiations take the mesh, the planes and the calibration as launch-uniform
// kernel arguments (scalar registers) and never read the trailing BatchDev; the batched ones look the subject up (batch_device.h).
#pragma once
#pragma clang fp contract(off)

#include "batch_device.h"
#include "sign_list_device.h"

namespace icon {

constexpr int kBlock = 256;

// point mode, one wavefront per point (see nearest_coop).  BATCH: the wave's point belongs to subject i / n of a batched call
// (wave-uniform: that subject's descriptors by scalar loads, in SGPRs as the unbatched call's kernel arguments are)
template <bool BATCH>
__global__ __launch_bounds__(kCoopWaves * 64) void k_nearest_coop(MeshDev m, Calib cal, const float *__restrict__ pts, int64_t N,
                                                                 NearRef near, int cap, float sdf_clip, BatchDev bd)
{
    extern __shared__ __attribute__((aligned(16))) char coop_smem[];
    const int wave = BATCH ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (int)(threadIdx.x >> 6);
    const int64_t i = (int64_t)blockIdx.x * kCoopWaves + wave;
    if (i >= N) return;
    if (BATCH) {
        const int b = __builtin_amdgcn_readfirstlane((int)(i / bd.n));
        m = batch_mesh_uniform(bd, b); cal = batch_calib_uniform(bd, b);
    }
    const f3 p = project(resolve_calib(cal), mk3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
    const Nearest nr = nearest_coop(m, p, coop_lds(coop_smem, wave, cap));
    if ((threadIdx.x & 63) == 0) store_near(near, i, nr, sdf_clip);
}

// Feature assembly: one 16-float row per point,
//   icon : [img(csel) | sdf | cmap r g b | norm x y z | 0.. | code]
//   pamir: [img(C) | vol(Cv) | 0.. | code]      pifu: [img(C) | z | 0.. | code]
// Rows are indexed by the point's linear index (lattice: (z*R + y)*R + x relative to plane z0).
// Src::Batch: point i of the B*n points of a batched call - calibration, planes, volume and mesh of subject i / n, per lane.
template <int PRIOR, Src SRC, bool BRUTE>
__global__ __launch_bounds__(kBlock) void k_features(MeshDev m, FeatDev f, Calib cal, LatticeMap L,
                                                     const float *__restrict__ pts, int64_t N,
                                                     float sdf_clip, int cmap_local,
                                                     const int32_t *__restrict__ row_count, const int32_t *__restrict__ row_slots,
                                                     NearRef near,
                                                     float *__restrict__ X, uint8_t *__restrict__ code8, int skip_shell, BatchDev bd)
{
    __shared__ int lds[(PRIOR == ICON_PRIOR_ICON && BRUTE) ? kBruteTile * 24 : 1];
    int64_t i; bool live; f3 p;
    if (SRC == Src::Lattice) {
        // L tiles the WHOLE slab here (every point gets a row); skip_shell: the geometry pre-pass left the shell out
        int ix, iy, iz, cx, cy, cz;
        live = lattice_point(L, ix, iy, iz);
        lattice_clamp(L, ix, iy, iz, cx, cy, cz);
        p = lattice_world(L.res, cx, cy, cz + L.z0);
        i = ((int64_t)cz * L.res + cy) * L.res + cx;
        if (skip_shell && !in_cube_bit(p)) {
            // a shell point: multiplied by 0 whatever its row holds (in_cube, HGPIFuNet.py:363) - a zero row and the code
            // byte k_sign wrote (icon) / in_cube = 0, without touching the search results that do not exist for it
            if (live) {
                float z[kXRow];
#pragma unroll
                for (int k = 0; k < kXRow; ++k) z[k] = 0.0f;
                uint32_t c = 0;
                if (PRIOR == ICON_PRIOR_ICON) c = code8[i];
                z[kCodeSlot] = __int_as_float((int)c);
                store_row(X, i, z);
                if (PRIOR != ICON_PRIOR_ICON) code8[i] = (uint8_t)c;
            }
            return;
        }
    } else {
        i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        live = i < N;
        if (!live) i = N - 1;
        if (SRC == Src::Batch) {              // the point's subject: its calibration, planes, volume and mesh replace the call's
            const int64_t b = i / bd.n;
            cal = batch_calib(bd, b);
            f = batch_feat(f, bd, b);
            if (PRIOR == ICON_PRIOR_ICON) m = bd.meshes[b];
        }
        p = project(resolve_calib(cal), mk3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
    }
    float row[kXRow];
#pragma unroll
    for (int k = 0; k < kXRow; ++k) row[k] = 0.0f;
    uint32_t code = in_cube_bit(p);
    if (PRIOR == ICON_PRIOR_ICON) {
        Nearest nr;
        bool ins;
        float s;
        f3 cmv;
        SdfOut o;
        if (BRUTE) {
            nr = nearest_brute<kBlock>(m, p, reinterpret_cast<float *>(lds)); ins = inside_brute(m, p);
            o = sdf_attrs(m, p, nr, ins);
            code = sign_code(p, nr.d2, ins, sdf_clip);
        } else {
            // the geometry pre-pass ran on the same stream just before: slot of the nearest triangle, the code byte
            // (outlier / sign / inside / in_cube) and, for points inside the clip band only, d^2
            code = code8[i];
            nr.slot = near_slot_of(near, i); nr.face = 0;
            nr.d2 = (code & kCodeOutlier) ? 0.0f : near_d2(near, i);
            ins = (code & kCodeInside) != 0;
            o = sdf_attrs(m, p, nr, ins);
        }
        s = o.sdf;
        cmv = o.cm;
        if (code & kCodeOutlier) {            // HGPIFuNet.py:298-305
            s = (float)code_sign(code);
            if (cmap_local) cmv = mk3(s, s, s);   // reference mode: patched later from the sign list
        }
        float g[16];
        gather_planes_dyn(f, (f.n_select == 2 && o.vis == 0.0f) ? 1 : 0, p.x, p.y, g);   // feat_select: vis==1 -> front half; no 'vis': all channels
        const int h = f.csel;
        for (int k = 0; k < h; ++k) row[k] = g[k];
        int hh = h;                                       // [img | sdf | cmap (if) | norm (if)], HGPIFuNet.py:301-311
        row[hh++] = s;
        if (f.smpl_mask & kSmplCmap) { row[hh] = cmv.x; row[hh + 1] = cmv.y; row[hh + 2] = cmv.z; hh += 3; }
        if (f.smpl_mask & kSmplNorm) { row[hh] = o.nrm.x; row[hh + 1] = o.nrm.y; row[hh + 2] = o.nrm.z; }
    } else {
        float g[16];
        gather_planes_dyn(f, 0, p.x, p.y, g);
        const int h = f.csel;
        for (int k = 0; k < h; ++k) row[k] = g[k];
        if (PRIOR == ICON_PRIOR_PAMIR) {
            float v[8];
            if (f.vpad == 8) gather_volume<2>(f, p.x, p.y, p.z, v); else gather_volume<1>(f, p.x, p.y, p.z, v);
            for (int k = 0; k < f.Cv; ++k) row[h + k] = v[k];
        } else {
            row[h] = p.z;
        }
    }
    row[kCodeSlot] = __int_as_float((int)code);
    if (live) { store_row(X, i, row); code8[i] = (uint8_t)code; }   // byte copy of the code word: the outlier passes stream 1 B/pt
}

// X rows + codes of the call's work items (the materialising path): k_features, reading the search results unless the search is
// brute force.  A template of the source so that each unit instantiates the kernels of the sources it serves (query_kernels.hip:
// lattice and points, batch_query.hip: batch).
template <Src SRC>
int launch_features(const QueryCall &c, icon_work *work, hipStream_t st)
{
    // every point of the slab gets a row: tile the whole slab, whatever region the geometry pre-pass covered
    LatticeMap Lf = c.L;
    if (SRC == Src::Lattice) {
        Lf.sx0 = Lf.sy0 = Lf.sz0 = 0; Lf.sx1 = Lf.sy1 = c.L.res; Lf.sz1 = c.L.nz;
        Lf.tx = (c.L.res + 15) / 16; Lf.ty = (c.L.res + 3) / 4; Lf.tz = (c.L.nz + 3) / 4; Lf.pk = 4; Lf.trim = 0;
    }
    const int64_t nb = SRC == Src::Lattice ? (int64_t)Lf.tx * Lf.ty * Lf.tz : (c.N + kBlock - 1) / kBlock;
    ICON_ARG(nb > 0 && nb < (1ll << 31), "too many workgroups for one launch");
    const dim3 grid((unsigned)nb), block(kBlock);
    constexpr bool batch = SRC == Src::Batch;    // mesh and calibration per subject, through c.bd
    const MeshDev md = (c.mesh && !batch) ? c.mesh->dev : MeshDev{};
    const int32_t *row_count = batch ? nullptr : work->d_row_count, *row_slots = batch ? nullptr : work->d_row_slots;
    const int local = (c.cmap_mode == ICON_CMAP_LOCAL) ? 1 : 0;
#define ICON_LAUNCH(P, B) hipLaunchKernelGGL((k_features<P, SRC, B>), grid, block, 0, st, md, c.feat->dev, c.cal, Lf, c.points, c.N, c.sdf_clip, local, row_count, row_slots, work_near(work, c), work->d_x, work->d_code8, c.L.off, c.bd)
    if constexpr (!batch) {                      // (a batched call refuses the brute-force search: no such instantiation)
        if (c.prior == ICON_PRIOR_ICON && c.search == ICON_SEARCH_BRUTE) { ICON_LAUNCH(ICON_PRIOR_ICON, true); ICON_HIP(hipGetLastError()); return ICON_OK; }
    }
    if (c.prior == ICON_PRIOR_ICON) ICON_LAUNCH(ICON_PRIOR_ICON, false);
    else if (c.prior == ICON_PRIOR_PAMIR) ICON_LAUNCH(ICON_PRIOR_PAMIR, false);
    else ICON_LAUNCH(ICON_PRIOR_PIFU, false);
#undef ICON_LAUNCH
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}
extern template int launch_features<Src::Batch>(const QueryCall &, icon_work *, hipStream_t);     // batch_query.hip

}  // namespace icon

// batch_query.hip - HGPIFuNet.query for B subjects in ONE call (icon_query_points_batch), as the reference's own query takes
// them: points [B,3,N], calibs [B,4,4], feature stacks [B,C,H,W], smpl_feat_dict [B,...] (lib/net/HGPIFuNet.py:268-367,
// lib/dataset/mesh_util.py:357-396).
//
// The batch is one point-mode call over the B*N points in subject-major order: point i belongs to subject b = i / N.  Everything
// that runs over the linear order of a call's points - the 1-byte codes, the outlier count / scan / compaction, the reference-mode
// cmap patch, the steal pool of the fused kernel, the MLP - applies unchanged, and the outlier list over the B*N points in that
// order IS the reference's batch-global list (smpl_sdf[outlier].repeat(1,1,3) flattens [B,N,.] subject-major, :303-305).  What
// differs per subject - mesh, feature planes, calibration - is looked up through a BatchDev descriptor (batch_device.h).
//
// Launches per call and feature stack do not depend on B:
//   icon, N*B < kPacketMinPoints : k_nearest_coop<true>, k_sign_wide<true>, [outlier list], fused kernel + rescue
//   icon, larger calls           : Morton keys + radix sort, k_nearest_batch, k_sign_wide<true>, [outlier list], fused + rescue
//   pamir / pifu                 : fused kernel + rescue (pamir: subject b's packed volume, icon_feat_batch_set_volume)
// (f32 / ICON_AMD_UNFUSED=1: k_features<prior, Src::Batch>, [patch], the MLP kernels over the materialised rows instead of the fused kernel.)
// These are the kernels of the unbatched point-mode call, instantiated for the batched source (query_device.h, fused_f16x3.hip):
// this file holds the batched C ABI, the face check and the one search kernel that has no unbatched twin (k_nearest_batch).
//
// The packet search needs every wavefront's 64 points to belong to one subject (it walks that subject's BVH with scalar loads):
// the Morton key carries the subject above the Morton bits, and the search grid pads every subject's sorted segment to whole
// wavefronts (padding lanes are parked, as the last wave of an unbatched call is).  Kernels that take one point per lane
// (k_sign_wide, k_features, the fused kernel's feature phase) look the subject up per lane: their tiles may straddle two.
#pragma clang fp contract(off)

#include "query_device.h"

#include <algorithm>

namespace icon {

constexpr int kBatchChecked = 0x100;          // status word: the face check has run (pinned host mirror only)

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
// check_sign(verts, faces[0], points) (mesh_util.py:393) tests every subject against subject 0's faces: flag a subject whose face
// f names other vertices than subject 0's face f (the vertex ids the device build stored with the triangle record)
__global__ __launch_bounds__(kBlock) void k_faces_match(const MeshDev *__restrict__ tab, int B, int64_t F, int *__restrict__ status)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (int64_t)(B - 1) * F) return;
    const int b = 1 + (int)(t / F);
    const int f = (int)(t - (int64_t)(b - 1) * F);
    const TriRec &r0 = tab[0].tris[tab[0].face2slot[f]];
    const TriRec &rb = tab[b].tris[tab[b].face2slot[f]];
    if (r0.ia != rb.ia || r0.ib != rb.ib || r0.ic != rb.ic) atomicOr(status, ICON_MESH_BATCH_FACES_DIFFER);
}

// nearest triangle, 64-point packets over the Morton order: position k of the PADDED order holds sorted position b n + r of
// subject b = k / npad (npad = n rounded up to whole wavefronts, so a wave never mixes subjects); r >= n: a parked lane
__global__ __launch_bounds__(kBlock) void k_nearest_batch(BatchDev bd, const float *__restrict__ pts, int64_t npad, NearRef near,
                                                          const int32_t *__restrict__ perm, float sdf_clip)
{
    __shared__ int lds[(kBlock / 64) * kStackDepth];
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int b = __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * kBlock + (threadIdx.x & ~63u)) / npad));
    if (b >= bd.B) return;                                       // (wave-uniform: the tail of the last workgroup)
    const int64_t r = k - (int64_t)b * npad;
    const bool live = r < bd.n;
    const int64_t i = perm[(int64_t)b * bd.n + (live ? r : bd.n - 1)];
    const MeshDev m = batch_mesh_uniform(bd, b);
    const f3 p = project(batch_calib_uniform(bd, b), mk3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
    const Nearest nr = nearest_packet(m, p, live, lds + (threadIdx.x >> 6) * kStackDepth, {mesh_root(m)});
    if (live) store_near(near, i, nr, sdf_clip);
}

// the geometry half of a batched icon call over the B*N points: nearest triangle (cooperative or Morton packets), the sign pass
// (code bytes + block counts) and, for the reference cmap rule, the batch-global outlier sign list.  Shared by
// icon_query_points_batch and icon_train_rows_forward (train_rows.hip): the search runs once per call, whoever consumes it.
int batch_geometry(const icon_mesh_batch *mb, const BatchDev &bd, const float *d_points, int64_t N, int B, float sdf_clip,
                   bool needs_patch, icon_work *work, hipStream_t st)
{
    const icon_mesh *mesh0 = mb->subj[0];
    const float *d_calibs = bd.calibs;
    const int64_t NB = N * (int64_t)B;
    int rc;
    if (mb->F > kNearLoSlots && work->cap_points_hi < work->cap_points) {      // big meshes: the byte of higher slot bits
        (void)hipFree(work->d_near_hi); work->d_near_hi = nullptr; work->cap_points_hi = 0;
        ICON_HIP(hipMalloc((void **)&work->d_near_hi, (size_t)work->cap_points));
        work->cap_points_hi = work->cap_points;
    }
    const NearRef near = work_near(work, mesh0);
    static const int mode = getenv("ICON_AMD_POINT_SEARCH") ? atoi(getenv("ICON_AMD_POINT_SEARCH")) : 0;   // 0 auto, 2 coop, 3 packets
    if (mode != 3 && (NB < kPacketMinPoints || mode == 2)) {
        const int cap = coop_cap(mb->depth_bound);
        hipLaunchKernelGGL(k_nearest_coop<true>, dim3((unsigned)((NB + kCoopWaves - 1) / kCoopWaves)), dim3(kCoopWaves * 64),
                           kCoopWaves * coop_wave_bytes(cap), st, MeshDev{}, Calib{}, d_points, NB, near, cap, sdf_clip, bd);
    } else {
        const int32_t *perm = nullptr;
        if ((rc = morton_order_batch(work, d_points, d_calibs, N, B, st, &perm))) return rc;
        const int64_t npad = (N + 63) / 64 * 64;
        const int64_t nb = (npad * B + kBlock - 1) / kBlock;
        ICON_ARG(nb < (1ll << 31), "icon_query_points_batch: too many workgroups for one launch");
        if (work->prof) (void)hipEventRecord(work->ev[4], st);
        hipLaunchKernelGGL(k_nearest_batch, dim3((unsigned)nb), dim3(kBlock), 0, st, bd, d_points, npad, near, perm, sdf_clip);
        if (work->prof) { (void)hipEventRecord(work->ev[5], st); work->ev_search = true; }
    }
    ICON_HIP(hipGetLastError());
    debug_sync("nearest (batch)", st);
    if ((rc = launch_sign(mesh0, Calib{}, 0, 0, d_points, NB, sdf_clip, work, false, st, &bd))) return rc;
    debug_sync("k_sign_wide<batch>", st);
    if (needs_patch && (rc = outlier_list(work, NB, nullptr, work->d_signs, true, st))) return rc;
    return ICON_OK;
}

}  // namespace icon

// =============================================================================================
// C ABI
// =============================================================================================
using namespace icon;

extern "C" int icon_mesh_batch_destroy(icon_mesh_batch_t *mb)
{
    if (!mb) return ICON_OK;
    if (mb->done) (void)hipEventDestroy(mb->done);
    (void)hipFree(mb->d_table);
    if (mb->h_table) (void)hipHostFree(mb->h_table);
    if (mb->h_status) (void)hipHostFree(mb->h_status);
    delete mb;
    return ICON_OK;
}

extern "C" int icon_mesh_batch_create(const icon_mesh_t *const *meshes, int B, void *stream, icon_mesh_batch_t **out)
{
    ICON_ARG(out != nullptr, "icon_mesh_batch_create: out is null");
    *out = nullptr;
    ICON_ARG(meshes != nullptr && B >= 1, "icon_mesh_batch_create: no meshes");
    for (int b = 0; b < B; ++b) {
        ICON_ARG(meshes[b] != nullptr, "icon_mesh_batch_create: a mesh is null");
        ICON_ARG(meshes[b]->V == meshes[0]->V && meshes[b]->F == meshes[0]->F,
                 "icon_mesh_batch_create: the subjects' vertex / face counts differ (check_sign takes subject 0's faces for every subject, "
                 "lib/dataset/mesh_util.py:393)");
    }
    hipStream_t st = (hipStream_t)stream;
    icon_mesh_batch *mb = new icon_mesh_batch();
    mb->B = B; mb->V = meshes[0]->V; mb->F = meshes[0]->F;
    for (int b = 0; b < B; ++b) { mb->subj.push_back(meshes[b]); mb->depth_bound = std::max(mb->depth_bound, meshes[b]->depth_bound); }
    // device table: B descriptors followed by the status word (initialised to kBatchChecked by the same upload)
    const size_t tab_bytes = (size_t)B * sizeof(MeshDev), bytes = tab_bytes + sizeof(int);
    hipError_t e = hipMalloc((void **)&mb->d_table, bytes);
    if (e == hipSuccess) e = hipHostMalloc((void **)&mb->h_table, bytes, hipHostMallocPortable);
    if (e == hipSuccess) e = hipHostMalloc((void **)&mb->h_status, sizeof(int), hipHostMallocPortable);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&mb->done, hipEventDisableTiming);
    if (e != hipSuccess) { icon_mesh_batch_destroy(mb); return fail(ICON_ERR_HIP, std::string("icon_mesh_batch_create: ") + hipGetErrorString(e)); }
    for (int b = 0; b < B; ++b) mb->h_table[b] = meshes[b]->dev;
    int *h_word = reinterpret_cast<int *>(reinterpret_cast<char *>(mb->h_table) + tab_bytes);
    int *d_word = reinterpret_cast<int *>(reinterpret_cast<char *>(mb->d_table) + tab_bytes);
    *h_word = kBatchChecked;
    *(volatile int *)mb->h_status = 0;
    e = hipMemcpyAsync(mb->d_table, mb->h_table, bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && B > 1 && mb->F > 0) {
        const int64_t n = (int64_t)(B - 1) * mb->F;
        hipLaunchKernelGGL(k_faces_match, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, mb->d_table, B, mb->F, d_word);
        e = hipGetLastError();
    }
    // the verdict lands in pinned memory without a synchronisation (icon_mesh_batch_status reads it, as icon_mesh_status does)
    if (e == hipSuccess) e = hipMemcpyAsync(mb->h_status, d_word, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventRecord(mb->done, st);
    if (e != hipSuccess) { icon_mesh_batch_destroy(mb); return fail(ICON_ERR_HIP, std::string("icon_mesh_batch_create: ") + hipGetErrorString(e)); }
    *out = mb;
    return ICON_OK;
}

extern "C" int icon_mesh_batch_status(const icon_mesh_batch_t *mb, int wait, int *bits)
{
    ICON_ARG(mb != nullptr, "icon_mesh_batch_status: batch is null");
    if (wait) ICON_HIP(hipEventSynchronize(mb->done));
    const int st = *reinterpret_cast<const volatile int *>(mb->h_status);
    if (!(st & kBatchChecked)) { if (bits) *bits = -1; return ICON_OK; }
    if (bits) *bits = st & ~kBatchChecked;
    if (st & ICON_MESH_BATCH_FACES_DIFFER)
        return fail(ICON_ERR_ARG, "icon_mesh_batch: the subjects' faces differ - check_sign(verts, faces[0], points) (lib/dataset/mesh_util.py:393) "
                                  "tests every subject against subject 0's faces; bind subjects of one topology");
    return ICON_OK;
}

extern "C" int icon_query_points_batch(const icon_mesh_batch_t *mb, const icon_feat_t *feat, const icon_mlp_t *mlp,
                                       int prior_type, float sdf_clip, int cmap_mode, const float *d_calibs,
                                       const float *d_points, int64_t N, int B, float *d_occ,
                                       int search, int precision, icon_work_t *work, void *stream)
{
    ICON_ARG(mlp && work && feat && d_points && d_occ && d_calibs, "icon_query_points_batch: null argument");
    ICON_ARG(N >= 0 && B >= 1, "icon_query_points_batch: bad N / B");
    ICON_ARG(N * (int64_t)B < (1ll << 31), "icon_query_points_batch: B * N must be below 2^31");
    if (search == ICON_SEARCH_BRUTE) return fail(ICON_ERR_UNSUPPORTED, "icon_query_points_batch: search 'brute' is evaluated at batch size 1 only");
    if (work->tie_rule != 0) return fail(ICON_ERR_UNSUPPORTED, "icon_query_points_batch: tie rules are evaluated at batch size 1 only");
    ICON_ARG(prior_type == ICON_PRIOR_ICON || prior_type == ICON_PRIOR_PAMIR || prior_type == ICON_PRIOR_PIFU, "icon_query_points_batch: unknown prior_type");
    ICON_ARG(feat->batch == B, "icon_query_points_batch: the feature handle holds another number of subjects");
    const FeatDev &f = feat->dev;
    int c0 = 0;
    if (prior_type == ICON_PRIOR_ICON) {
        ICON_ARG(mb != nullptr, "icon_query_points_batch: the icon prior needs a mesh batch");
        ICON_ARG(mb->B == B, "icon_query_points_batch: the mesh batch holds another number of subjects");
        c0 = f.csel + 1 + ((f.smpl_mask & kSmplCmap) ? 3 : 0) + ((f.smpl_mask & kSmplNorm) ? 3 : 0);
    } else if (prior_type == ICON_PRIOR_PAMIR) {
        // [index(im_feat, xy) | index(vol_feat, xyz)] per subject (lib/net/HGPIFuNet.py:346-353): no mesh, no search, no sign pass
        ICON_ARG(f.n_select == 1, "icon_query_points_batch: pamir prior needs n_select = 1");
        ICON_ARG(f.vol != nullptr, "icon_query_points_batch: the pamir prior needs a feature handle with a volume (icon_feat_batch_set_volume)");
        c0 = f.csel + f.Cv;
    } else {
        ICON_ARG(f.n_select == 1, "icon_query_points_batch: pifu prior needs n_select = 1");
        c0 = f.csel + 1;
    }
    if (c0 > kCodeSlot) return fail(ICON_ERR_UNSUPPORTED, "icon_query_points_batch: more than 15 MLP input channels");
    ICON_ARG(c0 == mlp->c0, "icon_query_points_batch: MLP input width does not match the feature layout");
    if (N == 0) return ICON_OK;
    const int64_t NB = N * (int64_t)B;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = ensure_work(work, NB, false))) return rc;
    work->slab_ready = false;
    work->q_rows_ready = false; work->slab_patched = false;
    const icon_mesh *mesh0 = (prior_type == ICON_PRIOR_ICON) ? mb->subj[0] : nullptr;
    BatchDev bd{};
    bd.meshes = mesh0 ? mb->d_table : nullptr; bd.calibs = d_calibs; bd.n = N; bd.plane_stride = feat->plane_stride; bd.B = B;
    bd.vol_stride = feat->vol_stride;
    const bool needs_patch = prior_type == ICON_PRIOR_ICON && cmap_mode == ICON_CMAP_REFERENCE && (f.smpl_mask & kSmplCmap);
    const int local = (cmap_mode == ICON_CMAP_LOCAL) ? 1 : 0;
    mark(work, 0, st);
    if (prior_type == ICON_PRIOR_ICON && (rc = batch_geometry(mb, bd, d_points, N, B, sdf_clip, needs_patch, work, st))) return rc;
    mark(work, 1, st);
    const SignSrc fs = self_signs(work, needs_patch);
    if (want_fused(precision, search)) {
        mark(work, 2, st);
        rc = launch_fused_f16x3(mesh0, feat, mlp, prior_type, Calib{}, LatticeMap{}, 0, 0, d_points, NB, sdf_clip, local, work, fs, d_occ,
                                false, st, &bd);
        mark(work, 3, st);
        return rc;
    }
    if ((rc = ensure_work(work, NB, true))) return rc;
    const NearRef near = work_near(work, mesh0);
    const unsigned nb = (unsigned)((NB + kBlock - 1) / kBlock);
#define ICON_LAUNCH(P) hipLaunchKernelGGL((k_features<P, Src::Batch, false>), dim3(nb), dim3(kBlock), 0, st, MeshDev{}, f, Calib{}, LatticeMap{}, d_points, NB, sdf_clip, local, (const int32_t *)nullptr, (const int32_t *)nullptr, near, work->d_x, work->d_code8, 0, bd)
    if (prior_type == ICON_PRIOR_ICON) ICON_LAUNCH(ICON_PRIOR_ICON);
    else if (prior_type == ICON_PRIOR_PAMIR) ICON_LAUNCH(ICON_PRIOR_PAMIR);
    else ICON_LAUNCH(ICON_PRIOR_PIFU);
#undef ICON_LAUNCH
    ICON_HIP(hipGetLastError());
    if ((rc = outlier_patch(work, NB, f.csel + 1, fs, st))) return rc;
    mark(work, 2, st);
    rc = mlp_launch(mlp, work->d_x, NB, d_occ, precision, st);
    mark(work, 3, st);
    return rc;
}

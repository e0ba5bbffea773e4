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

// the search of a batched icon call over its B*n points: cooperative, or Morton packets.  The sign pass and the batch-global outlier
// list behind it are the common ones (call_geometry), for icon_query_points_batch and icon_train_rows_forward (train_rows.hip) alike.
int launch_nearest_batch(const QueryCall &c, icon_work *work, hipStream_t st)
{
    const BatchDev &bd = c.bd;
    const int64_t NB = c.N;
    const NearRef near = work_near(work, c);
    if (coop_search(NB, work)) {
        const int cap = coop_cap(c.mb->depth_bound);
        hipLaunchKernelGGL(k_nearest_coop<true>, dim3((unsigned)((NB + kCoopWaves - 1) / kCoopWaves)), dim3(kCoopWaves * 64),
                           kCoopWaves * coop_wave_bytes(cap), st, MeshDev{}, Calib{}, c.points, NB, near, cap, c.sdf_clip, bd);
    } else {
        const int32_t *perm = nullptr;
        const int rc = morton_order_batch(work, c.points, bd.calibs, bd.n, bd.B, st, &perm);
        if (rc) return rc;
        const int64_t npad = (bd.n + 63) / 64 * 64;
        const int64_t nb = (npad * bd.B + kBlock - 1) / kBlock;
        ICON_ARG(nb < (1ll << 31), std::string(c.who) + ": too many workgroups for one launch");
        if (work->prof) (void)hipEventRecord(work->ev[4], st);
        hipLaunchKernelGGL(k_nearest_batch, dim3((unsigned)nb), dim3(kBlock), 0, st, bd, c.points, npad, near, perm, c.sdf_clip);
        if (work->prof) { (void)hipEventRecord(work->ev[5], st); work->ev_search = true; }
    }
    ICON_HIP(hipGetLastError());
    debug_sync("nearest (batch)", st);
    return ICON_OK;
}

template int launch_features<Src::Batch>(const QueryCall &, icon_work *, hipStream_t);     // k_features<prior, Src::Batch> live in this unit

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
    QueryCall c = query_call("icon_query_points_batch", Src::Batch, feat, prior_type, sdf_clip, cmap_mode, search);
    c.mb = mb; c.points = d_points; c.N = N * (int64_t)B;
    c.bd.calibs = d_calibs; c.bd.n = N; c.bd.B = B; c.bd.plane_stride = feat->plane_stride; c.bd.vol_stride = feat->vol_stride;
    int rc = describe_call(c);
    if (rc) return rc;
    ICON_ARG(c.c0 == mlp->c0, "icon_query_points_batch: MLP input width does not match the feature layout");
    if (N == 0) return ICON_OK;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = begin_call(work, c))) return rc;
    mark(work, 0, st);
    if ((rc = call_geometry(c, nullptr, work, st))) return rc;
    mark(work, 1, st);
    return call_finish(c, mlp, self_signs(work, c.needs_patch), d_occ, precision, work, st);
}

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
//   icon, N*B < kPacketMinPoints : k_nearest_coop_batch, k_sign_batch, [outlier list], fused kernel + rescue
//   icon, larger calls           : Morton keys + radix sort, k_nearest_batch, k_sign_batch, [outlier list], fused + rescue
//   pamir / pifu                 : fused kernel + rescue (pamir: subject b's packed volume, icon_feat_batch_set_volume)
// (f32 / ICON_AMD_UNFUSED=1: k_features_batch, [patch], the MLP kernels over the materialised rows instead of the fused kernel.)
//
// The packet search needs every wavefront's 64 points to belong to one subject (it walks that subject's BVH with scalar loads):
// the Morton key carries the subject above the Morton bits, and the search grid pads every subject's sorted segment to whole
// wavefronts (padding lanes are parked, as the last wave of an unbatched call is).  Kernels that take one point per lane
// (k_sign_batch, k_features_batch, the fused kernel's feature phase) look the subject up per lane: their tiles may straddle two.
#pragma clang fp contract(off)

#include "batch_device.h"

#include <algorithm>

namespace icon {

constexpr int kBatchBlock = 256;
constexpr int kBatchChecked = 0x100;          // status word: the face check has run (pinned host mirror only)

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
// B feature stacks [B][C][H][W] -> B plane sets [n_select][H][W][cpad], `stride` floats apart (grid z = subject)
__global__ void k_pack_planes_batch(const float *__restrict__ src, int C, int H, int W, int n_select, int csel, int cpad, int64_t stride,
                                    float *__restrict__ dst)
{
    const int64_t n = (int64_t)n_select * H * W * cpad;
    const float *s = src + (int64_t)blockIdx.z * C * H * W;
    float *d = dst + (int64_t)blockIdx.z * stride;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % cpad);
        const int64_t pix = (i / cpad) % ((int64_t)H * W);
        const int sel = (int)(i / ((int64_t)cpad * H * W));
        d[i] = (c < csel) ? s[((int64_t)(sel * csel + c)) * H * W + pix] : 0.0f;
    }
}

// check_sign(verts, faces[0], points) (mesh_util.py:393) tests every subject against subject 0's faces: flag a subject whose face
// f names other vertices than subject 0's face f (the vertex ids the device build stored with the triangle record)
__global__ __launch_bounds__(kBatchBlock) void k_faces_match(const MeshDev *__restrict__ tab, int B, int64_t F, int *__restrict__ status)
{
    const int64_t t = (int64_t)blockIdx.x * kBatchBlock + threadIdx.x;
    if (t >= (int64_t)(B - 1) * F) return;
    const int b = 1 + (int)(t / F);
    const int f = (int)(t - (int64_t)(b - 1) * F);
    const TriRec &r0 = tab[0].tris[tab[0].face2slot[f]];
    const TriRec &rb = tab[b].tris[tab[b].face2slot[f]];
    if (r0.ia != rb.ia || r0.ib != rb.ib || r0.ic != rb.ic) atomicOr(status, ICON_MESH_BATCH_FACES_DIFFER);
}

// nearest triangle, one wavefront per point (calls of few points, see nearest_coop): the wave's subject is uniform
__global__ __launch_bounds__(kCoopWaves * 64) void k_nearest_coop_batch(BatchDev bd, const float *__restrict__ pts, int64_t N, NearRef near,
                                                                       int cap, float sdf_clip)
{
    extern __shared__ __attribute__((aligned(16))) char coop_smem[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t i = (int64_t)blockIdx.x * kCoopWaves + wave;
    if (i >= N) return;
    const int b = __builtin_amdgcn_readfirstlane((int)(i / bd.n));
    const MeshDev m = batch_mesh_uniform(bd, b);
    const f3 p = project(batch_calib_uniform(bd, b), mk3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
    const Nearest nr = nearest_coop(m, p, coop_lds(coop_smem, wave, cap));
    if ((threadIdx.x & 63) == 0) store_near(near, i, nr, sdf_clip);
}

// nearest triangle, 64-point packets over the Morton order: position k of the PADDED order holds sorted position b n + r of
// subject b = k / npad (npad = n rounded up to whole wavefronts, so a wave never mixes subjects); r >= n: a parked lane
__global__ __launch_bounds__(kBatchBlock) void k_nearest_batch(BatchDev bd, const float *__restrict__ pts, int64_t npad, NearRef near,
                                                          const int32_t *__restrict__ perm, float sdf_clip)
{
    __shared__ int lds[(kBatchBlock / 64) * kStackDepth];
    const int64_t k = (int64_t)blockIdx.x * kBatchBlock + threadIdx.x;
    const int b = __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * kBatchBlock + (threadIdx.x & ~63u)) / npad));
    if (b >= bd.B) return;                                       // (wave-uniform: the tail of the last workgroup)
    const int64_t r = k - (int64_t)b * npad;
    const bool live = r < bd.n;
    const int64_t i = perm[(int64_t)b * bd.n + (live ? r : bd.n - 1)];
    const MeshDev m = batch_mesh_uniform(bd, b);
    const f3 p = project(batch_calib_uniform(bd, b), mk3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
    const Nearest nr = nearest_packet(m, p, live, lds + (threadIdx.x >> 6) * kStackDepth);
    if (live) store_near(near, i, nr, sdf_clip);
}

// k_sign_wide (fused_f16x3.hip) per subject: four lanes per point walk the point's ray-bin list in ITS subject's mesh; a workgroup
// is one 256-point block of the outlier scan / one tile of the fused kernel, in the linear order of the B*n points
__global__ __launch_bounds__(1024) void k_sign_batch(BatchDev bd, const float *__restrict__ pts, int64_t N, float sdf_clip, NearRef near,
                                                     uint8_t *__restrict__ code8, int32_t *__restrict__ block_counts,
                                                     unsigned long long *__restrict__ grp_mask, float far_box2, int *__restrict__ range_flag)
{
    __shared__ unsigned long long gm[4];
    if (range_flag && blockIdx.x == 0 && threadIdx.x == 0) *range_flag = 0;
    if (threadIdx.x < 4) gm[threadIdx.x] = 0ull;
    __syncthreads();
    const int s = threadIdx.x & 3, pt = threadIdx.x >> 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + pt;
    const bool live = i < N;
    const int64_t ic = live ? i : N - 1;
    const int64_t b = ic / bd.n;
    const MeshDev m = bd.meshes[b];
    uint32_t code = 0;
    const MeshDyn &d = *m.dyn;
    f3 p = mk3(0.f, 0.f, 0.f);
    int beg = 0, end = 0;
    bool brute = false;
    if (live) {
        p = project(batch_calib(bd, b), mk3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
        if (d.gy == 0) brute = true;
        else if (p.y >= d.bin_y0 && p.y <= d.bin_y1 && p.z >= d.bin_z0 && p.z <= d.bin_z1) {
            const int cy = bin_cell(p.y, d.bin_y0, d.bin_inv_y, d.gy);
            const int cz = bin_cell(p.z, d.bin_z0, d.bin_inv_z, d.gz);
            const int cell = cz * d.gy + cy;
            beg = m.bin_start[cell]; end = m.bin_start[cell + 1];
        }
    }
    int cnt = 0;
    for (int k = beg + s; k < end; k += 4) {
        f3 a, bb, c; int ia, ib, icc;
        load_tri_full(m.tris + m.bin_slots[k], a, bb, c, ia, ib, icc);
        cnt += ray_hit(p, a, bb, c, ia, ib, icc);
    }
    cnt += __shfl_xor(cnt, 1);
    cnt += __shfl_xor(cnt, 2);
    if (live) {
        const bool ins = brute ? inside_brute(m, p) : ((cnt & 1) != 0);
        const bool far = box_dist2(d.box_lo[0], d.box_lo[1], d.box_lo[2], d.box_hi[0], d.box_hi[1], d.box_hi[2], p) > far_box2 || near_is_far(near, i);
        code = far ? sign_code_far(p, ins) : sign_code(p, near_d2(near, i), ins, sdf_clip);
        if (s == 0) code8[i] = (uint8_t)code;
    }
    unsigned long long x = __ballot(live && s == 0 && (code & kCodeOutlier));      // bit 4 j = point j of this wave's 16
    x = (x | (x >> 3)) & 0x0303030303030303ull;
    x = (x | (x >> 6)) & 0x000f000f000f000full;
    x = (x | (x >> 12)) & 0x000000ff000000ffull;
    x = (x | (x >> 24)) & 0xffffull;
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0 && x) atomicOr(&gm[wave >> 2], x << (16 * (wave & 3)));
    __syncthreads();
    if (threadIdx.x < 4) grp_mask[(int64_t)blockIdx.x * 4 + threadIdx.x] = gm[threadIdx.x];
    if (threadIdx.x == 0) block_counts[blockIdx.x] = __popcll(gm[0]) + __popcll(gm[1]) + __popcll(gm[2]) + __popcll(gm[3]);
}

// the materialising path (precision f32, ICON_AMD_UNFUSED=1): k_features' point mode per subject, one 16-float row per point
template <int PRIOR>
__global__ __launch_bounds__(kBatchBlock) void k_features_batch(BatchDev bd, FeatDev f0, const float *__restrict__ pts, int64_t N, int cmap_local,
                                                           NearRef near, float *__restrict__ X, uint8_t *__restrict__ code8)
{
    int64_t i = (int64_t)blockIdx.x * kBatchBlock + threadIdx.x;
    const bool live = i < N;
    if (!live) i = N - 1;
    const int64_t b = i / bd.n;
    const f3 p = project(batch_calib(bd, b), mk3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
    const FeatDev f = batch_feat(f0, bd, b);
    float row[kXRow];
#pragma unroll
    for (int k = 0; k < kXRow; ++k) row[k] = 0.0f;
    uint32_t code = in_cube_bit(p);
    float g[16];
    if (PRIOR == ICON_PRIOR_ICON) {
        const MeshDev m = bd.meshes[b];
        code = code8[i];
        Nearest nr;
        nr.slot = near_slot_of(near, i); nr.face = 0;
        nr.d2 = (code & kCodeOutlier) ? 0.0f : near_d2(near, i);
        const SdfOut o = sdf_attrs(m, p, nr, (code & kCodeInside) != 0);
        float s = o.sdf;
        f3 cmv = o.cm;
        if (code & kCodeOutlier) {            // HGPIFuNet.py:298-305
            s = (float)((int)((code >> kCodeSignShift) & 3u) - 1);
            if (cmap_local) cmv = mk3(s, s, s);   // reference mode: patched later from the batch-global sign list
        }
        gather_planes_dyn(f, (f.n_select == 2 && o.vis == 0.0f) ? 1 : 0, p.x, p.y, g);
        const int h = f.csel;
        for (int k = 0; k < h; ++k) row[k] = g[k];
        int hh = h;
        row[hh++] = s;
        if (f.smpl_mask & kSmplCmap) { row[hh] = cmv.x; row[hh + 1] = cmv.y; row[hh + 2] = cmv.z; hh += 3; }
        if (f.smpl_mask & kSmplNorm) { row[hh] = o.nrm.x; row[hh + 1] = o.nrm.y; row[hh + 2] = o.nrm.z; }
    } else {                                  // pamir / pifu
        gather_planes_dyn(f, 0, p.x, p.y, g);
        const int h = f.csel;
        for (int k = 0; k < h; ++k) row[k] = g[k];
        if (PRIOR == ICON_PRIOR_PAMIR) {      // subject b's volume (batch_feat), as k_features
            float v[8];
            if (f.vpad == 8) gather_volume<2>(f, p.x, p.y, p.z, v); else gather_volume<1>(f, p.x, p.y, p.z, v);
            for (int k = 0; k < f.Cv; ++k) row[h + k] = v[k];
        } else {
            row[h] = p.z;
        }
    }
    row[kCodeSlot] = __int_as_float((int)code);
    if (live) { store_row(X, i, row); code8[i] = (uint8_t)code; }
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
        hipLaunchKernelGGL(k_faces_match, dim3((unsigned)((n + kBatchBlock - 1) / kBatchBlock)), dim3(kBatchBlock), 0, st, mb->d_table, B, mb->F, d_word);
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

extern "C" int icon_feat_create_batch(const float *d_planes, int B, int C, int H, int W, int n_select, void *stream, icon_feat_t **out)
{
    ICON_ARG(out != nullptr, "icon_feat_create_batch: out is null");
    *out = nullptr;
    ICON_ARG(d_planes && B >= 1 && C > 0 && H > 1 && W > 1, "icon_feat_create_batch: bad planes");
    ICON_ARG(n_select == 1 || n_select == 2, "icon_feat_create_batch: n_select must be 1 or 2");
    ICON_ARG(C % n_select == 0, "icon_feat_create_batch: C not divisible by n_select");
    ICON_ARG(B <= 65535, "icon_feat_create_batch: more than 65,535 subjects");
    const int csel = C / n_select;
    const int cpad = (csel + 3) & ~3;
    if (cpad > 16) return fail(ICON_ERR_UNSUPPORTED, "icon_feat_create_batch: more than 16 channels per tap");
    hipStream_t st = (hipStream_t)stream;
    icon_feat *f = new icon_feat();
    const int64_t stride = (int64_t)n_select * H * W * cpad;
    hipError_t e = hipMalloc((void **)&f->d_planes, (size_t)stride * B * sizeof(float));
    if (e != hipSuccess) { delete f; return fail(ICON_ERR_HIP, std::string("hipMalloc planes: ") + hipGetErrorString(e)); }
    hipLaunchKernelGGL(k_pack_planes_batch, dim3((unsigned)std::max(1, 1024 / B), 1, (unsigned)B), dim3(256), 0, st, d_planes, C, H, W, n_select,
                       csel, cpad, stride, f->d_planes);
    FeatDev &d = f->dev;
    d.planes = f->d_planes; d.C = C; d.H = H; d.W = W; d.n_select = n_select; d.csel = csel; d.cpad = cpad;
    d.smpl_mask = kSmplCmap | kSmplNorm;
    d.vol = nullptr; d.Cv = 0; d.Dv = d.Hv = d.Wv = 0; d.vpad = 0;
    f->batch = B; f->plane_stride = stride;
    e = hipGetLastError();
    if (e != hipSuccess) { icon_feat_destroy(f); return fail(ICON_ERR_HIP, std::string("pack planes: ") + hipGetErrorString(e)); }
    *out = f;
    return ICON_OK;
}

extern "C" int icon_feat_batch_set_volume(icon_feat_t *feat, const float *d_vol, int B, int Cv, int Dv, int Hv, int Wv, void *stream)
{
    ICON_ARG(feat != nullptr && d_vol != nullptr, "icon_feat_batch_set_volume: null argument");
    ICON_ARG(B == feat->batch, "icon_feat_batch_set_volume: the volume holds another number of subjects than the feature handle");
    ICON_ARG(feat->dev.vol == nullptr, "icon_feat_batch_set_volume: the handle already holds a volume");
    ICON_ARG(Cv > 0 && Dv > 1 && Hv > 1 && Wv > 1, "icon_feat_batch_set_volume: bad volume");
    if (Cv > 8) return fail(ICON_ERR_UNSUPPORTED, "icon_feat_batch_set_volume: more than 8 volume channels");
    hipStream_t st = (hipStream_t)stream;
    // icon_feat_create's layout per subject: a volume is a "plane" of D*H rows, channel-last, zero padded to vpad
    const int vpad = (Cv + 3) & ~3;
    const int64_t stride = (int64_t)Dv * Hv * Wv * vpad;
    float *d = nullptr;
    hipError_t e = hipMalloc((void **)&d, (size_t)stride * B * sizeof(float));
    if (e != hipSuccess) return fail(ICON_ERR_HIP, std::string("hipMalloc vol: ") + hipGetErrorString(e));
    hipLaunchKernelGGL(k_pack_planes_batch, dim3((unsigned)std::max(1, 1024 / B), 1, (unsigned)B), dim3(256), 0, st, d_vol, Cv, Dv * Hv, Wv, 1,
                       Cv, vpad, stride, d);
    e = hipGetLastError();
    if (e != hipSuccess) { (void)hipFree(d); return fail(ICON_ERR_HIP, std::string("pack volume: ") + hipGetErrorString(e)); }
    feat->d_vol = d; feat->vol_stride = stride;
    FeatDev &f = feat->dev;
    f.vol = d; f.Cv = Cv; f.Dv = Dv; f.Hv = Hv; f.Wv = Wv; f.vpad = vpad;
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
    if ((rc = ensure_work_rows(work, NB, false))) return rc;
    work->slab_ready = false;
    work->q_rows_ready = false; work->slab_patched = false;
    const icon_mesh *mesh0 = (prior_type == ICON_PRIOR_ICON) ? mb->subj[0] : nullptr;
    BatchDev bd{};
    bd.meshes = mesh0 ? mb->d_table : nullptr; bd.calibs = d_calibs; bd.n = N; bd.plane_stride = feat->plane_stride; bd.B = B;
    bd.vol_stride = feat->vol_stride;
    const bool needs_patch = prior_type == ICON_PRIOR_ICON && cmap_mode == ICON_CMAP_REFERENCE && (f.smpl_mask & kSmplCmap);
    const int local = (cmap_mode == ICON_CMAP_LOCAL) ? 1 : 0;
    work_mark(work, 0, st);
    if (prior_type == ICON_PRIOR_ICON) {
        if (mb->F > kNearLoSlots && work->cap_points_hi < work->cap_points) {      // big meshes: the byte of higher slot bits
            (void)hipFree(work->d_near_hi); work->d_near_hi = nullptr; work->cap_points_hi = 0;
            ICON_HIP(hipMalloc((void **)&work->d_near_hi, (size_t)work->cap_points));
            work->cap_points_hi = work->cap_points;
        }
        const NearRef near = work_near(work, mesh0);
        static const int mode = getenv("ICON_AMD_POINT_SEARCH") ? atoi(getenv("ICON_AMD_POINT_SEARCH")) : 0;   // 0 auto, 2 coop, 3 packets
        if (mode != 3 && (NB < kPacketMinPoints || mode == 2)) {
            const int cap = coop_cap(mb->depth_bound);
            hipLaunchKernelGGL(k_nearest_coop_batch, dim3((unsigned)((NB + kCoopWaves - 1) / kCoopWaves)), dim3(kCoopWaves * 64),
                               kCoopWaves * coop_wave_bytes(cap), st, bd, d_points, NB, near, cap, sdf_clip);
        } else {
            const int32_t *perm = nullptr;
            if ((rc = morton_order_batch(work, d_points, d_calibs, N, B, st, &perm))) return rc;
            const int64_t npad = (N + 63) / 64 * 64;
            const int64_t nb = (npad * B + kBatchBlock - 1) / kBatchBlock;
            ICON_ARG(nb < (1ll << 31), "icon_query_points_batch: too many workgroups for one launch");
            if (work->prof) (void)hipEventRecord(work->ev[4], st);
            hipLaunchKernelGGL(k_nearest_batch, dim3((unsigned)nb), dim3(kBatchBlock), 0, st, bd, d_points, npad, near, perm, sdf_clip);
            if (work->prof) { (void)hipEventRecord(work->ev[5], st); work->ev_search = true; }
        }
        ICON_HIP(hipGetLastError());
        debug_sync("nearest (batch)", st);
        const int64_t nblk = (NB + 255) / 256;
        hipLaunchKernelGGL(k_sign_batch, dim3((unsigned)nblk), dim3(1024), 0, st, bd, d_points, NB, sdf_clip, near, work->d_code8,
                           work->d_block_counts, (unsigned long long *)work->d_grp_mask, far_box_dist2(sdf_clip), work->d_flag);
        ICON_HIP(hipGetLastError());
        work->flag_clean = work->d_flag != nullptr;
        debug_sync("k_sign_batch", st);
        if (needs_patch && (rc = outlier_list_counted(work, NB, st))) return rc;
    }
    work_mark(work, 1, st);
    FusedSigns fs{};
    fs.mode = needs_patch ? kSignSelf : kSignNone;
    fs.list = work->d_signs; fs.k_dev = work->d_total;
    if (fused_path(precision, search)) {
        work_mark(work, 2, st);
        rc = launch_fused_f16x3(mesh0, feat, mlp, prior_type, Calib{}, LatticeMap{}, 0, 0, d_points, NB, sdf_clip, local, work, fs, d_occ,
                                false, st, &bd);
        work_mark(work, 3, st);
        return rc;
    }
    if ((rc = ensure_work_rows(work, NB, true))) return rc;
    const NearRef near = work_near(work, mesh0);
    const unsigned nb = (unsigned)((NB + kBatchBlock - 1) / kBatchBlock);
    if (prior_type == ICON_PRIOR_ICON)
        hipLaunchKernelGGL(k_features_batch<ICON_PRIOR_ICON>, dim3(nb), dim3(kBatchBlock), 0, st, bd, f, d_points, NB, local, near, work->d_x, work->d_code8);
    else if (prior_type == ICON_PRIOR_PAMIR)
        hipLaunchKernelGGL(k_features_batch<ICON_PRIOR_PAMIR>, dim3(nb), dim3(kBatchBlock), 0, st, bd, f, d_points, NB, local, near, work->d_x, work->d_code8);
    else
        hipLaunchKernelGGL(k_features_batch<ICON_PRIOR_PIFU>, dim3(nb), dim3(kBatchBlock), 0, st, bd, f, d_points, NB, local, near, work->d_x, work->d_code8);
    ICON_HIP(hipGetLastError());
    if (needs_patch && (rc = patch_self_rows(work, NB, f.csel + 1, st))) return rc;
    work_mark(work, 2, st);
    rc = mlp_launch(mlp, work->d_x, NB, d_occ, precision, st);
    work_mark(work, 3, st);
    return rc;
}

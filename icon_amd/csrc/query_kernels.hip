// query_kernels.hip - gfx950 kernels for the per-point geometry/feature half of HGPIFuNet.query:
//   nearest triangle (BVH2, per-lane LDS stack, or LDS-tiled brute force), +x ray parity over
//   (y,z) bins, Heidrich barycentric interpolation, outlier clipping, bilinear / trilinear
//   feature gather + front/back select, and assembly of the 16-float MLP input rows.
//
// Reference being replaced (paths relative to the reference root):
//   lib/dataset/mesh_util.py:357-396 (cal_sdf_batch), :319-354 (barycentrics), :266-277 (feat_select)
//   lib/net/HGPIFuNet.py:268-365 (query), lib/net/geometry.py:21-61 (index, orthogonal)
//
// Arithmetic spec: float32, the only fused operations are the explicit fmaf() calls,
// IEEE division / sqrt (hipcc default: correctly rounded).  This file is compiled with
// -ffp-contract=off; the pragma below is a second line of defence.
#pragma clang fp contract(off)

#include "query_device.h"
#include "sign_list_device.h"

namespace icon {

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
// cal_sdf_batch for explicit points (API parity with the reference function; also the unit-test
// surface for the geometry kernels)
template <bool BRUTE>
__global__ __launch_bounds__(kBlock) void k_sdf_query(MeshDev m, const float *__restrict__ pts, int64_t N,
                                                      float *sdf, float *nrm, float *cm, float *vis,
                                                      int64_t *face, uint8_t *inside_out, const int32_t *__restrict__ perm)
{
    __shared__ int lds[kBruteTile * 24];   // brute: TriPre tile; packet: 4 wave stacks
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < N;
    if (live && perm) i = perm[i];           // Morton order (sort_points.hip): a wave's 64 points are neighbours
    const int64_t ic = live ? i : (N - 1);
    const f3 p = clamp_raw(mk3(pts[3 * ic], pts[3 * ic + 1], pts[3 * ic + 2]));
    Nearest nr;
    bool ins;
    if (BRUTE) { nr = nearest_brute<kBlock>(m, p, reinterpret_cast<float *>(lds)); ins = inside_brute(m, p); }
    else       { nr = nearest_packet(m, p, live, lds + (threadIdx.x >> 6) * kStackDepth, {mesh_root(m)}); ins = inside_bins(m, p); }
    if (!live) return;
    const SdfOut o = sdf_attrs(m, p, nr, ins);
    sdf[i] = o.sdf;
    nrm[3 * i] = o.nrm.x; nrm[3 * i + 1] = o.nrm.y; nrm[3 * i + 2] = o.nrm.z;
    cm[3 * i] = o.cm.x; cm[3 * i + 1] = o.cm.y; cm[3 * i + 2] = o.cm.z;
    vis[i] = o.vis;
    if (face) face[i] = nr.face;
    if (inside_out) inside_out[i] = ins ? 1 : 0;
}

__global__ __launch_bounds__(kCoopWaves * 64) void k_sdf_query_coop(MeshDev m, const float *__restrict__ pts, int64_t N,
                                                                   float *sdf, float *nrm, float *cm, float *vis,
                                                                   int64_t *face, uint8_t *inside_out, int cap)
{
    extern __shared__ __attribute__((aligned(16))) char coop_smem[];
    const int64_t i = (int64_t)blockIdx.x * kCoopWaves + (threadIdx.x >> 6);
    if (i >= N) return;
    const f3 p = clamp_raw(mk3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
    const Nearest nr = nearest_coop(m, p, coop_lds(coop_smem, threadIdx.x >> 6, cap));
    if ((threadIdx.x & 63) != 0) return;
    const bool ins = inside_bins(m, p);
    const SdfOut o = sdf_attrs(m, p, nr, ins);
    sdf[i] = o.sdf;
    nrm[3 * i] = o.nrm.x; nrm[3 * i + 1] = o.nrm.y; nrm[3 * i + 2] = o.nrm.z;
    cm[3 * i] = o.cm.x; cm[3 * i + 1] = o.cm.y; cm[3 * i + 2] = o.cm.z;
    vis[i] = o.vis;
    if (face) face[i] = nr.face;
    if (inside_out) inside_out[i] = ins ? 1 : 0;
}

// Nearest-triangle search as its own launch: the packet traversal needs ~50 VGPRs, so it runs at
// full occupancy (8 waves / SIMD hide the dependent scalar-load chain), which the register-heavier
// attribute / gather code would cap at 5.  Output per point, structure of arrays: the slot of the nearest
// triangle with the "outside the clip band" flag, and - inside the band only - its squared distance (store_near).
// ALT (diagnostics, icon_work_set_tie_rule): the alternative tie rule - highest face index among the faces within
// `tie_ulps` float32 ulps of the minimum d^2 (nearest_packet_alt) - for measuring how much of the output hangs on
// the unpinned tie behaviour of the kaolin leaf (lib/dataset/mesh_util.py:374-390).
// CLAMP: the half-unit, clamped evaluation of the oriented boxes (nearest_packet; "box_clamp"), lattice launches only.
// The host launches it only for a mesh that holds pair boxes AND node boxes (the default), so what the walk would otherwise ask the
// mesh record at every visit is settled when the kernel is compiled (nearest_packet's BOXES).
// <true, false, false> is the same lattice launch on pair_box_bound and on whatever tables the mesh has, for meshes created with
// one of the three options off (A/B, tests): bit-identical results.
template <bool LATTICE, bool ALT, bool CLAMP>
__global__ __launch_bounds__(kBlock) void k_nearest(MeshDev m, Calib cal, LatticeMap L, const float *__restrict__ pts, int64_t N,
                                                    NearRef near, const int32_t *__restrict__ perm,
                                                    float sdf_clip, int tie_ulps, const LatticeFast *lf)
{
    __shared__ int lds[(kBlock / 64) * kStackDepth];
    int64_t i; bool live; f3 p;
    int root = 0;
    if (LATTICE) {
        int cx, cy, cz;
        if (lf) {                                                // 4^3 packets, default block order: the set-up precomputed per call
            const LatticeFast F = lattice_fast_load(lf);
            if ((int)blockIdx.x >= F.nb) return;                 // beyond the trimmed tiling (the host tiled the whole slab)
            live = lattice_point_fast(F, blockIdx.x, threadIdx.x >> 6, threadIdx.x & 63, cx, cy, cz);
            p = lattice_world_fast(lf, cx, cy, cz + L.z0);
            root = F.root;
        } else {
            PacketPoint pt;
            if (!packet_point(L, m, (int)blockIdx.x, threadIdx.x >> 6, threadIdx.x & 63, pt)) return;
            live = pt.live; p = pt.p; cx = pt.cx; cy = pt.cy; cz = pt.cz;
            root = mesh_root(m);
        }
        i = ((int64_t)cz * L.res + cy) * L.res + cx;
    } else {
        i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        live = i < N;
        if (!live) i = N - 1;
        if (perm) i = perm[i];          // Morton order: the wave's 64 points are neighbours (sort_points.hip)
        p = project(resolve_calib(cal), mk3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
        root = mesh_root(m);
    }
    Nearest nr = nearest_packet<false, false, CLAMP, CLAMP>(m, p, live, lds + (threadIdx.x >> 6) * kStackDepth, {root, LATTICE ? packet_center_lane(L) : 21});
    if (ALT) nr = nearest_packet_alt(m, p, live, lds + (threadIdx.x >> 6) * kStackDepth, (uint32_t)__float_as_int(nr.d2), (uint32_t)tie_ulps);
    // (staging the 16 x 4 x 4 block through LDS so that 16 threads store one 64-byte run removes the partial-line
    //  writes but the block-wide barrier costs 0.14 ms; not kept)
    if (live) store_near(near, i, nr, sdf_clip);
}

// Lattices of few packets (33^3 .. 65^3 slabs: the first level of the reference's schedule): one PACKET per workgroup, its walk
// shared by the NW wavefronts (nearest_shared) - such a launch lasts as long as its longest walk, and this divides the walk.
// Workgroup b serves packet b & 3 of tile b >> 2 of k_nearest's tiling.
template <int NW>
__global__ __launch_bounds__(NW * 64) void k_nearest_shared(MeshDev m, LatticeMap L, NearRef near, float sdf_clip, ShareDbg dbg)
{
    __shared__ int lds[NW * kStackDepth];
    __shared__ __attribute__((aligned(16))) char smem[share_lds_bytes(NW)];
    // (the prologue written out, not packet_point: with the bound check inside an inlined helper this kernel compiles to other
    //  registers - SGPRs 94 -> 86 / 88, VGPRs 60 -> 62 - and its listing is kept as it was)
    L = lattice_trim(L, m);
    if ((int)(blockIdx.x >> 2) >= L.tx * L.ty * L.tz) return;
    int ix, iy, iz, cx, cy, cz;
    const bool live = lattice_point_at(L, (int)(blockIdx.x >> 2), (int)(blockIdx.x & 3), threadIdx.x & 63, ix, iy, iz);
    lattice_clamp(L, ix, iy, iz, cx, cy, cz);
    const f3 p = lattice_world(L.res, cx, cy, cz + L.z0);
    const Nearest nr = nearest_shared<NW>(m, p, live, lds + (threadIdx.x >> 6) * kStackDepth, smem, packet_center_lane(L), dbg);
    if (live && threadIdx.x < 64) store_near(near, ((int64_t)cz * L.res + cy) * L.res + cx, nr, sdf_clip);
}

// Diagnostics (icon_sdf_query_ties): winner, runner-up and the ulp gap between their squared distances
__global__ __launch_bounds__(kBlock) void k_nearest_ties(MeshDev m, const float *__restrict__ pts, int64_t N, const int32_t *__restrict__ perm,
                                                         int32_t *__restrict__ face, int32_t *__restrict__ face2, uint8_t *__restrict__ ulps)
{
    __shared__ int lds[(kBlock / 64) * kStackDepth];
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < N;
    if (!live) i = N - 1;
    if (perm) i = perm[i];
    const f3 p = clamp_raw(mk3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
    unsigned long long k2 = 0;
    WalkArgs wa{mesh_root(m)};
    wa.runner_up = &k2;
    const Nearest nr = nearest_packet<false, true>(m, p, live, lds + (threadIdx.x >> 6) * kStackDepth, wa);
    if (!live) return;
    const uint32_t b1 = (uint32_t)__float_as_int(nr.d2), b2 = (uint32_t)(k2 >> 32);
    const int f2 = (int)(k2 & 0xffffffffu);
    const bool has2 = f2 != 0x7fffffff && b2 >= b1;
    face[i] = nr.face;
    face2[i] = has2 ? f2 : -1;
    ulps[i] = (uint8_t)(has2 ? min(b2 - b1, 255u) : 255u);
}

// diagnostics: the work of the lattice walk, summed over the packets of a slab (icon_debug_traversal_stats / _pair_stats /
// _walk_stats; DESIGN.md reports visited nodes / point, tools/pair_box_model.py predicts the pairs offered and tested on the CPU).
// out = [packets, inner nodes, leaf pairs offered, pairs tested, leaves, oriented parents, triangles of the visited leaves,
// longest walk (nodes + triangles of one packet: what a latency-bound launch waits for)].
// The children are ordered by packet_center_lane(L) as in k_nearest: lane 21 for the default 4^3 packets, lane 0 under a
// non-default ICON_AMD_PACKET (where traversal_stats used to keep lane 21).
template <bool CLAMP>
__global__ __launch_bounds__(kBlock) void k_walk_stats(MeshDev m, LatticeMap L, unsigned long long *out /* [8] */)
{
    __shared__ int lds[(kBlock / 64) * kStackDepth];
    PacketPoint pt;
    if (!packet_point(L, m, (int)blockIdx.x, threadIdx.x >> 6, threadIdx.x & 63, pt)) return;
    WalkStats ws = {};
    nearest_packet<true, false, CLAMP>(m, pt.p, pt.live, lds + (threadIdx.x >> 6) * kStackDepth,
                                       {mesh_root(m), packet_center_lane(L), &ws});
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out[0], 1ull); atomicAdd(&out[1], (unsigned long long)ws.nodes);
        atomicAdd(&out[2], (unsigned long long)ws.offered); atomicAdd(&out[3], (unsigned long long)ws.tested);
        atomicAdd(&out[4], (unsigned long long)ws.leaves); atomicAdd(&out[5], (unsigned long long)ws.obox);
        atomicAdd(&out[6], (unsigned long long)ws.tris);
        atomicMax(&out[7], (unsigned long long)(ws.nodes + ws.tris));
    }
}

// one thread per (y, z) row of the slab: triangles whose (y,z) projection covers the row
__global__ __launch_bounds__(kBlock) void k_row_crossings(MeshDev m, LatticeMap L, int32_t *row_count, int32_t *row_slots, LatticeFast *lf)
{
    if (lf && blockIdx.x == 0 && threadIdx.x == 0) lattice_fast_write(lf, L, m);      // the search's per-packet set-up, once per call
    if (lf) lattice_fast_coords(lf, L.res, (int64_t)blockIdx.x * kBlock + threadIdx.x);
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= (int64_t)L.nz * L.res) return;
    const int iy = (int)(row % L.res), iz = (int)(row / L.res);
    const f3 p = lattice_world(L.res, 0, iy, iz + L.z0);
    int n = 0;
    const MeshDyn &d = *m.dyn;
    if (d.gy == 0) { row_count[row] = -1; return; }          // no bin lists (kMeshBinOverflow): every point takes inside_bins' brute-force branch
    if (p.y >= d.bin_y0 && p.y <= d.bin_y1 && p.z >= d.bin_z0 && p.z <= d.bin_z1) {
        const int cy = bin_cell(p.y, d.bin_y0, d.bin_inv_y, d.gy);
        const int cz = bin_cell(p.z, d.bin_z0, d.bin_inv_z, d.gz);
        const int cell = cz * d.gy + cy;
        const int beg = m.bin_start[cell], end = m.bin_start[cell + 1];
        for (int k = beg; k < end; ++k) {
            const int slot = m.bin_slots[k];
            f3 a, b, c; int ia, ib, ic;
            load_tri_full(m.tris + slot, a, b, c, ia, ib, ic);
            if (ray_covers(p, a, b, c, ia, ib, ic)) {
                if (n < kRowCap) row_slots[row * kRowCap + n] = slot;
                ++n;
            }
        }
    }
    row_count[row] = (n <= kRowCap) ? n : -1;
}

// The same with 16 lanes per row (slabs of few rows - the coarse lattices: 33^2 = 1,089 threads walking ~100-entry bin lists one
// after the other were a 28 us launch of pure latency): the lanes of a group take every 16th entry of the bin list, the hits are
// appended in list order through a ballot (the same row_slots as the one-thread version, entry for entry).
__global__ __launch_bounds__(kBlock) void k_row_crossings_wide(MeshDev m, LatticeMap L, int32_t *row_count, int32_t *row_slots, LatticeFast *lf)
{
    if (lf && blockIdx.x == 0 && threadIdx.x == 0) lattice_fast_write(lf, L, m);
    if (lf) lattice_fast_coords(lf, L.res, (int64_t)blockIdx.x * kBlock + threadIdx.x);
    const int lane = threadIdx.x & 63, g = lane >> 4, s = lane & 15;
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 4;
    const bool have = row < (int64_t)L.nz * L.res;
    const MeshDyn &d = *m.dyn;
    if (d.gy == 0) { if (have && s == 0) row_count[row] = -1; return; }
    const int iy = have ? (int)(row % L.res) : 0, iz = have ? (int)(row / L.res) : 0;
    const f3 p = lattice_world(L.res, 0, iy, iz + L.z0);
    int beg = 0, end = 0;
    if (have && p.y >= d.bin_y0 && p.y <= d.bin_y1 && p.z >= d.bin_z0 && p.z <= d.bin_z1) {
        const int cy = bin_cell(p.y, d.bin_y0, d.bin_inv_y, d.gy);
        const int cz = bin_cell(p.z, d.bin_z0, d.bin_inv_z, d.gz);
        const int cell = cz * d.gy + cy;
        beg = m.bin_start[cell]; end = m.bin_start[cell + 1];
    }
    int n = 0;
    for (int k = beg + s; __any(k - s < end); k += 16) {
        bool hit = false;
        int slot = 0;
        if (k < end) {
            slot = m.bin_slots[k];
            f3 a, b, c; int ia, ib, ic;
            load_tri_full(m.tris + slot, a, b, c, ia, ib, ic);
            hit = ray_covers(p, a, b, c, ia, ib, ic);
        }
        const unsigned grp = (unsigned)(__ballot(hit) >> (16 * g)) & 0xffffu;
        const int at = n + __popc(grp & ((1u << s) - 1u));
        if (hit && at < kRowCap) row_slots[row * kRowCap + at] = slot;
        n += __popc(grp);
    }
    if (have && s == 0) row_count[row] = (n <= kRowCap) ? n : -1;
}

// The f16x3 precision (the default) with the BVH search runs FUSED: no input rows in HBM (fused_f16x3.hip).
// ICON_AMD_UNFUSED=1 forces the materialising path (tests compare the two bit for bit).
bool want_fused(int precision, int search)
{
    return !option(kOptUnfused) && precision == ICON_PRECISION_F16X3 && search != ICON_SEARCH_BRUTE;
}

}  // namespace icon

// =============================================================================================
// C ABI
// =============================================================================================
using namespace icon;


extern "C" int icon_sdf_query(const icon_mesh_t *mesh, const float *d_points, int64_t N,
                              float *d_sdf, float *d_norm, float *d_cmap, float *d_vis,
                              int64_t *d_face, uint8_t *d_inside, int search, void *stream)
{
    ICON_ARG(mesh && d_points && d_sdf && d_norm && d_cmap && d_vis, "icon_sdf_query: null argument");
    ICON_ARG(N >= 0, "icon_sdf_query: negative N");
    if (N == 0) return ICON_OK;
    const int64_t nb = (N + kBlock - 1) / kBlock;
    ICON_ARG(nb < (1ll << 31), "icon_sdf_query: N too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    if (search == ICON_SEARCH_BRUTE) {
        hipLaunchKernelGGL(k_sdf_query<true>, dim3((unsigned)nb), dim3(kBlock), 0, st, mesh->dev, d_points, N, d_sdf, d_norm,
                           d_cmap, d_vis, d_face, d_inside, nullptr);
    } else if (N < kPacketMinPoints) {    // sparse / unordered points: one wavefront per point (see nearest_coop)
        const int cap = coop_cap(mesh->depth_bound);
        hipLaunchKernelGGL(k_sdf_query_coop, dim3((unsigned)((N + kCoopWaves - 1) / kCoopWaves)), dim3(kCoopWaves * 64), kCoopWaves * coop_wave_bytes(cap), st,
                           mesh->dev, d_points, N, d_sdf, d_norm, d_cmap, d_vis, d_face, d_inside, cap);
    } else {                              // large batches: packets over the Morton order (scratch freed after a stream sync)
        icon_work tmp;
        const int32_t *perm = nullptr;
        int rc = morton_order(&tmp, d_points, kIdentCalib, nullptr, N, st, &perm);
        if (!rc) {
            hipLaunchKernelGGL(k_sdf_query<false>, dim3((unsigned)nb), dim3(kBlock), 0, st, mesh->dev, d_points, N, d_sdf, d_norm,
                               d_cmap, d_vis, d_face, d_inside, perm);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = fail(ICON_ERR_HIP, "icon_sdf_query: launch failed");
        }
        (void)hipFree(tmp.d_sort_keys); (void)hipFree(tmp.d_sort_idx); (void)hipFree(tmp.d_sort_tmp);
        return rc;
    }
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

namespace icon {

int describe_call(QueryCall &c)
{
    ICON_ARG(c.feat != nullptr, std::string(c.who) + ": feature handle is null");
    if (c.src == Src::Batch) ICON_ARG(c.feat->batch == c.bd.B, std::string(c.who) + ": the feature handle holds another number of subjects");
    return describe_call(c, c.feat->dev);
}

// the same for a call whose rows have the layout f without a feature handle behind it (the training rows: train_rows.hip)
int describe_call(QueryCall &c, const FeatDev &f)
{
    const auto say = [&c](const char *what) { return std::string(c.who) + ": " + what; };      // (evaluated by a refusal only)
    ICON_ARG(c.prior == ICON_PRIOR_ICON || c.prior == ICON_PRIOR_PAMIR || c.prior == ICON_PRIOR_PIFU, say("unknown prior_type"));
    if (c.prior == ICON_PRIOR_ICON) {
        if (c.src == Src::Batch) {
            ICON_ARG(c.mb != nullptr, say("the icon prior needs a mesh batch"));
            ICON_ARG(c.mb->B == c.bd.B, say("the mesh batch holds another number of subjects"));
            c.mesh = c.mb->subj[0]; c.bd.meshes = c.mb->d_table;
        }
        ICON_ARG(c.mesh != nullptr, say("the icon prior needs a mesh handle"));
        // n_select = 2: smpl_vis picks the front or back half (HGPIFuNet.py:334-336); 1: smpl_feats without 'vis', every channel is an input (:345-346)
        c.c0 = f.csel + 1 + ((f.smpl_mask & kSmplCmap) ? 3 : 0) + ((f.smpl_mask & kSmplNorm) ? 3 : 0);
    } else if (c.prior == ICON_PRIOR_PAMIR) {
        // [index(im_feat, xy) | index(vol_feat, xyz)] (lib/net/HGPIFuNet.py:346-353): no mesh, no search, no sign pass
        ICON_ARG(f.n_select == 1, say("the pamir prior needs n_select = 1"));
        ICON_ARG(f.vol != nullptr, say("the pamir prior needs a feature handle with a volume (icon_feat_batch_set_volume for a batch)"));
        c.c0 = f.csel + f.Cv;
    } else {
        ICON_ARG(f.n_select == 1, say("the pifu prior needs n_select = 1"));
        c.c0 = f.csel + 1;
    }
    if (c.c0 > kCodeSlot) return fail(ICON_ERR_UNSUPPORTED, say("more than 15 MLP input channels"));
    c.needs_patch = c.prior == ICON_PRIOR_ICON && c.cmap_mode == ICON_CMAP_REFERENCE && (f.smpl_mask & kSmplCmap);
    c.cmap_slot = f.csel + 1;
    return ICON_OK;
}

// point mode: sparse calls walk the tree one wavefront per point; a call dense enough for a wave's 64 Morton neighbours to be
// close together goes through the packet kernels (the alternative tie rule - diagnostics - lives in the packet kernel only)
bool coop_search(int64_t N, const icon_work *work)
{
    static const int mode = getenv("ICON_AMD_POINT_SEARCH") ? atoi(getenv("ICON_AMD_POINT_SEARCH")) : 0;   // 0 auto, 2 coop, 3 packets
    return work->tie_rule == 0 && mode != 3 && (N < kPacketMinPoints || mode == 2);
}

namespace {

// the search of a lattice / points call (icon prior, BVH): per-row crossing lists (lattice), nearest triangle -> work_near
template <bool LATTICE>
int launch_nearest(const QueryCall &c, icon_work *work, hipStream_t st)
{
    const icon_mesh *mesh = c.mesh;
    const LatticeMap &L = c.L;
    const int64_t N = c.N;
    LatticeFast *lf = nullptr;
    if (LATTICE) {
        const int64_t rows = (int64_t)L.nz * L.res;
        if (rows > work->cap_rows) {
            (void)hipFree(work->d_row_count); (void)hipFree(work->d_row_slots);
            work->d_row_count = nullptr; work->d_row_slots = nullptr; work->cap_rows = 0;
            ICON_HIP(hipMalloc((void **)&work->d_row_count, (size_t)rows * sizeof(int32_t)));
            ICON_HIP(hipMalloc((void **)&work->d_row_slots, (size_t)rows * kRowCap * sizeof(int32_t)));
            work->cap_rows = rows;
        }
        // the record of the search's per-packet set-up (LatticeFast): 4^3 packets in the default block order only
        if (option(kOptLatticeFast) && (L.pk == 0 || L.pk == 4) && L.remap == 0 && L.res <= kLatticeFastMaxRes) {
            if (!work->d_lfast) ICON_HIP(hipMalloc((void **)&work->d_lfast, kLatticeFastBytes));
            lf = work->d_lfast;
        }
        if (rows <= 20000)                       // up to 129^2 rows: 16 lanes per row
            hipLaunchKernelGGL(k_row_crossings_wide, dim3((unsigned)((rows * 16 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, mesh->dev, L,
                               work->d_row_count, work->d_row_slots, lf);
        else
            hipLaunchKernelGGL(k_row_crossings, dim3((unsigned)((rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, mesh->dev, L,
                               work->d_row_count, work->d_row_slots, lf);
    }
    int64_t nb;
    if (LATTICE) nb = (int64_t)L.tx * L.ty * L.tz; else nb = (N + kBlock - 1) / kBlock;
    ICON_ARG(nb >= 0 && nb < (1ll << 31), "too many workgroups for one launch");
    const NearRef near = work_near(work, c);
    const int32_t *perm = nullptr;
    const bool alt = work->tie_rule != 0;
    if (!LATTICE && coop_search(N, work)) {
        const int cap = coop_cap(mesh->depth_bound);
        hipLaunchKernelGGL(k_nearest_coop<false>, dim3((unsigned)((N + kCoopWaves - 1) / kCoopWaves)), dim3(kCoopWaves * 64),
                           kCoopWaves * coop_wave_bytes(cap), st, mesh->dev, c.cal, c.points, N, near, cap, c.sdf_clip, BatchDev{});
    } else if (nb > 0) {                         // nb == 0: a slab that is all shell (nothing to search)
        if (!LATTICE) {
            const int rc = morton_order(work, c.points, c.cal.m, c.cal.d, N, st, &perm);
            if (rc) return rc;
        }
        const int share_env = option(kOptShareWaves);            // diagnostics: 1 = never, 8 / 16
        const int nw = (!LATTICE || alt) ? 1 : ((share_env == 1 || share_env == 8 || share_env == 16) ? share_env : share_waves(nb * 4));
        ShareDbg dbg{};
        if (nw > 1) { const int rc = work_share_dbg(work, &dbg); if (rc) return rc; }
        if (work->prof) (void)hipEventRecord(work->ev[4], st);
        if (nw == 16) hipLaunchKernelGGL(k_nearest_shared<16>, dim3((unsigned)nb * 4), dim3(16 * 64), 0, st, mesh->dev, L, near, c.sdf_clip, dbg);
        else if (nw == 8) hipLaunchKernelGGL(k_nearest_shared<8>, dim3((unsigned)nb * 4), dim3(8 * 64), 0, st, mesh->dev, L, near, c.sdf_clip, dbg);
        else if (alt) hipLaunchKernelGGL((k_nearest<LATTICE, true, false>), dim3((unsigned)nb), dim3(kBlock), 0, st, mesh->dev, c.cal, L, c.points, N, near, perm, c.sdf_clip, work->tie_ulps, lf);
        else if (LATTICE && !(mesh->dev.box_clamp && mesh->dev.pbox_off && mesh->dev.nbox_off)) hipLaunchKernelGGL((k_nearest<true, false, false>), dim3((unsigned)nb), dim3(kBlock), 0, st, mesh->dev, c.cal, L, c.points, N, near, perm, c.sdf_clip, 0, lf);
        else hipLaunchKernelGGL((k_nearest<LATTICE, false, LATTICE>), dim3((unsigned)nb), dim3(kBlock), 0, st, mesh->dev, c.cal, L, c.points, N, near, perm, c.sdf_clip, 0, lf);
        if (work->prof) { (void)hipEventRecord(work->ev[5], st); work->ev_search = true; }
    }
    ICON_HIP(hipGetLastError());
    debug_sync(LATTICE ? "k_row_crossings + k_nearest<lattice>" : "nearest (points)", st);
    return ICON_OK;
}

// The MLP input rows of the call in work->d_x ([N, kXRow], reference channel order, slot kCodeSlot = code word) ...
int feature_rows(QueryCall &c, icon_work *work, hipStream_t st)
{
    if (c.rows_ready) return ICON_OK;
    int rc;
    if ((rc = ensure_work(work, c.N, true))) return rc;
    rc = c.src == Src::Lattice ? launch_features<Src::Lattice>(c, work, st)
       : c.src == Src::Points ? launch_features<Src::Points>(c, work, st) : launch_features<Src::Batch>(c, work, st);
    c.rows_ready = rc == ICON_OK;
    return rc;
}

// ... with the reference-mode outlier cmap patched in from wherever the call's sign list is.  Idempotent per call.
int materialise_rows(QueryCall &c, icon_work *work, const SignSrc &fs, hipStream_t st)
{
    int rc;
    if ((rc = feature_rows(c, work, st))) return rc;
    if (c.needs_patch && !c.patched) {
        if ((rc = outlier_patch(work, c.N, c.cmap_slot, fs, st))) return rc;
        c.patched = true;
    }
    return ICON_OK;
}

}  // namespace

int sign_and_list(const QueryCall &c, int8_t *d_signs_out, icon_work *work, hipStream_t st)
{
    int rc;
    if ((rc = launch_sign(c, work, st))) return rc;
    if (!c.n_dev) debug_sync(c.src == Src::Batch ? "k_sign_wide<batch>" : "k_sign", st);      // (a schedule level names its whole tail: adaptive.hip)
    if (c.needs_patch && (rc = outlier_list(work, c.N, c.n_dev, d_signs_out ? d_signs_out : work->d_signs, true, st))) return rc;
    return ICON_OK;
}

int call_geometry(QueryCall &c, int8_t *d_signs_out, icon_work *work, hipStream_t st)
{
    int rc;
    if (c.prior != ICON_PRIOR_ICON) return ICON_OK;
    if (c.search == ICON_SEARCH_BRUTE) {         // the rows themselves (k_features<.., BRUTE> searches and signs), then the list from their code bytes
        if ((rc = feature_rows(c, work, st))) return rc;
        return c.needs_patch ? outlier_list(work, c.N, nullptr, d_signs_out ? d_signs_out : work->d_signs, false, st) : ICON_OK;
    }
    rc = c.src == Src::Points ? launch_nearest<false>(c, work, st) : c.src == Src::Lattice ? launch_nearest<true>(c, work, st) : launch_nearest_batch(c, work, st);
    if (rc) return rc;
    return sign_and_list(c, d_signs_out, work, st);
}

int call_finish(QueryCall &c, const icon_mlp *mlp, const SignSrc &fs, float *d_occ, int precision, icon_work *work, hipStream_t st, int za, int zb)
{
    int rc;
    const LatticeMap &L = c.L;
    const bool lattice = c.src == Src::Lattice;
    const bool first = !lattice || za == L.z0;
    if (want_fused(precision, c.search)) {
        if (first) mark(work, 2, st);
        rc = launch_fused_f16x3(c, mlp, work, za, zb, fs, d_occ, st);
        mark(work, 3, st);
        return rc;
    }
    if ((rc = materialise_rows(c, work, fs, st))) return rc;
    if (first) mark(work, 2, st);
    if (lattice) {
        const int64_t o = (int64_t)(za - L.z0) * L.res * L.res, n = (int64_t)(zb - za) * L.res * L.res;
        rc = mlp_launch(mlp, work->d_x + o * kXRow, n, d_occ + o, precision, st);
    } else {
        rc = mlp_launch(mlp, work->d_x, c.N, d_occ, precision, st);
    }
    mark(work, 3, st);
    return rc;
}

}  // namespace icon

// a point-mode call's calibration: h_calib (host, null = identity) or d_calib (device, read by the kernels themselves)
static Calib points_calib(const float *h_calib, const float *d_calib)
{
    Calib cal;
    memcpy(cal.m, h_calib ? h_calib : kIdentCalib, sizeof(cal.m));
    cal.d = d_calib;
    return cal;
}

static int query_points_impl(const icon_mesh_t *mesh, const icon_feat_t *feat, const icon_mlp_t *mlp,
                             int prior_type, float sdf_clip, int cmap_mode, const float *h_calib, const float *d_calib,
                             const float *d_points, int64_t N, float *d_occ,
                             int search, int precision, icon_work_t *work, void *stream)
{
    ICON_ARG(mlp && work && d_points && d_occ, "icon_query_points: null argument");
    ICON_ARG(N >= 0, "icon_query_points: negative N");
    QueryCall c = query_call("icon_query_points", Src::Points, feat, prior_type, sdf_clip, cmap_mode, search);
    c.mesh = mesh; c.cal = points_calib(h_calib, d_calib); c.points = d_points; c.N = N;
    int rc = describe_call(c);
    if (rc) return rc;
    ICON_ARG(c.c0 == mlp->c0, "icon_query_points: MLP input width does not match the feature layout");
    if (N == 0) return ICON_OK;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = begin_call(work, c))) return rc;
    mark(work, 0, st);
    if ((rc = call_geometry(c, nullptr, work, st))) return rc;
    mark(work, 1, st);
    return call_finish(c, mlp, self_signs(work, c.needs_patch), d_occ, precision, work, st);
}

extern "C" int icon_query_points(const icon_mesh_t *mesh, const icon_feat_t *feat, const icon_mlp_t *mlp,
                                 int prior_type, float sdf_clip, int cmap_mode, const float *h_calib,
                                 const float *d_points, int64_t N, float *d_occ,
                                 int search, int precision, icon_work_t *work, void *stream)
{
    return query_points_impl(mesh, feat, mlp, prior_type, sdf_clip, cmap_mode, h_calib, nullptr, d_points, N, d_occ, search,
                             precision, work, stream);
}

extern "C" int icon_query_points_dcalib(const icon_mesh_t *mesh, const icon_feat_t *feat, const icon_mlp_t *mlp,
                                        int prior_type, float sdf_clip, int cmap_mode, const float *d_calib,
                                        const float *d_points, int64_t N, float *d_occ,
                                        int search, int precision, icon_work_t *work, void *stream)
{
    ICON_ARG(d_calib != nullptr, "icon_query_points_dcalib: d_calib is null");
    return query_points_impl(mesh, feat, mlp, prior_type, sdf_clip, cmap_mode, nullptr, d_calib, d_points, N, d_occ, search,
                             precision, work, stream);
}

// Lattice geometry of a slab.  `shell_ok`: the caller allows the shell skip (everything but the brute-force search,
// which computes its own rows for every point).  The MLP then never sees the shell (in_cube alone makes it 0); the
// SEARCH leaves out every face of the cube that is provably all "outside" outliers without looking at the mesh -
// farther from the body's bounding box than the clip band is wide, k_sign's own far test - and keeps the others: a
// shell point is an entry of the call's outlier sign list and its code byte must be right.
static int lattice_map(int res, int z0, int z1, const icon_mesh_t *mesh, float sdf_clip, bool shell_ok, LatticeMap *L)
{
    ICON_ARG(res >= 3 && (res & 1) == 1, "lattice resolution must be odd and >= 3 (seg3d_lossless.py:84-86)");
    ICON_ARG(z0 >= 0 && z1 > z0 && z1 <= res, "bad z range");
    L->res = res; L->z0 = z0; L->nz = z1 - z0;
    const int off = (shell_ok && option(kOptShellSkip)) ? 1 : 0;
    L->off = off;
    L->zs = std::max(z0, off); L->nzi = std::min(z1, res - off) - L->zs;
    if (L->nzi < 0) L->nzi = 0;
    // search region: the whole slab here - the kernel itself leaves out the far faces (lattice_trim: the body's box is
    // known on the device only) and workgroups beyond the trimmed tiling exit at once
    L->sx0 = 0; L->sx1 = res; L->sy0 = 0; L->sy1 = res; L->sz0 = 0; L->sz1 = z1 - z0;
    // points per wavefront of the search: 4^3 blocks (common.h: lattice_packet)
    L->pk = lattice_packet();
    L->tx = (L->sx1 - L->sx0 + 4 * L->pk - 1) / (4 * L->pk); L->ty = (L->sy1 - L->sy0 + L->pk - 1) / L->pk; L->tz = (L->sz1 - L->sz0 + L->pk - 1) / L->pk;
    L->trim = (off && mesh) ? 1 : 0;
    L->trim_need = std::sqrt(far_box_dist2(sdf_clip)) * 1.001f + 1e-5f;
    const char *e = getenv("ICON_AMD_XCD_REMAP");
    // 0: single blocks alternate over the XCDs (default, fastest); 2: whole x-rows of blocks per XCD - 14 % fewer HBM
    // write bytes (partial lines meet in one L2) but 1.5 % slower; 1: contiguous XCD bands, 1.6x slower
    L->remap = e ? atoi(e) : 0;
    return ICON_OK;
}

static int slab_features_impl(const icon_mesh_t *mesh, const icon_feat_t *feat, int prior_type, float sdf_clip, int cmap_mode,
                              int res, int z0, int z1, int8_t *d_signs_local, int64_t *d_count_local, void *d_msg, int64_t msg_bytes,
                              int search, icon_work_t *work, void *stream)
{
    ICON_ARG(work != nullptr, "icon_grid_slab_features: work is null");
    QueryCall c = query_call("icon_grid_slab_features", Src::Lattice, feat, prior_type, sdf_clip, cmap_mode, search);
    c.mesh = mesh;
    int rc = describe_call(c);
    if (rc) return rc;
    // the brute-force path computes rows for every point itself; everything else may skip the shell
    if ((rc = lattice_map(res, z0, z1, prior_type == ICON_PRIOR_ICON ? mesh : nullptr, sdf_clip, search != ICON_SEARCH_BRUTE, &c.L))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = c.N = (int64_t)c.L.nz * res * res;
    ICON_ARG(N < (1ll << 31), "icon_grid_slab_features: more than 2^31 points in one slab");
    if ((rc = begin_call(work, c))) return rc;
    mark(work, 0, st);
    if ((rc = call_geometry(c, d_signs_local, work, st))) return rc;
    if (d_count_local) {
        if (c.needs_patch) ICON_HIP(hipMemcpyAsync(d_count_local, work->d_total, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        else ICON_HIP(hipMemsetAsync(d_count_local, 0, sizeof(int64_t), st));
    }
    if (d_msg) {
        const int64_t cap = msg_bytes - 8;                 // packed bytes available
        ICON_ARG(msg_bytes >= 8 && cap * 4 >= N, "icon_grid_slab_features_msg: message buffer too small (8 + ceil(points / 4) bytes)");
        if (c.needs_patch) {
            if ((rc = pack_sign_message(work, d_signs_local ? d_signs_local : work->d_signs, d_msg, cap, st))) return rc;
        } else {
            ICON_HIP(hipMemsetAsync(d_msg, 0, sizeof(int64_t), st));
        }
    }
    mark(work, 1, st);
    work->slab = c; work->slab_ready = true;
    return ICON_OK;
}

extern "C" int icon_grid_slab_features(const icon_mesh_t *mesh, const icon_feat_t *feat,
                                       int prior_type, float sdf_clip, int cmap_mode,
                                       int res, int z0, int z1, int8_t *d_signs_local, int64_t *d_count_local,
                                       int search, icon_work_t *work, void *stream)
{
    return slab_features_impl(mesh, feat, prior_type, sdf_clip, cmap_mode, res, z0, z1, d_signs_local, d_count_local, nullptr, 0, search, work, stream);
}

extern "C" int icon_grid_slab_features_msg(const icon_mesh_t *mesh, const icon_feat_t *feat,
                                           int prior_type, float sdf_clip, int cmap_mode,
                                           int res, int z0, int z1, void *d_msg, int64_t msg_bytes,
                                           int search, icon_work_t *work, void *stream)
{
    ICON_ARG(d_msg != nullptr, "icon_grid_slab_features_msg: message buffer is null");
    return slab_features_impl(mesh, feat, prior_type, sdf_clip, cmap_mode, res, z0, z1, nullptr, nullptr, d_msg, msg_bytes, search, work, stream);
}

// the slab icon_grid_slab_features prepared on this workspace, if it is the one a finish call names
static QueryCall *prepared_slab(icon_work *work, int res, int z0, int z1)
{
    const LatticeMap &L = work->slab.L;
    return (work->slab_ready && L.res == res && L.z0 == z0 && L.z0 + L.nz == z1) ? &work->slab : nullptr;
}

extern "C" int icon_grid_slab_finish(const icon_mlp_t *mlp, int res, int z0, int z1,
                                     const int8_t *d_signs_global, int64_t k_total, int64_t rank_offset,
                                     float *d_occ, int precision, icon_work_t *work, void *stream)
{
    ICON_ARG(mlp && work && d_occ, "icon_grid_slab_finish: null argument");
    QueryCall *c = prepared_slab(work, res, z0, z1);
    if (!c) return fail(ICON_ERR_STATE, "icon_grid_slab_finish: no matching icon_grid_slab_features call on this workspace");
    ICON_ARG(c->c0 == mlp->c0, "icon_grid_slab_finish: MLP input width does not match the feature layout");
    SignSrc fs{};
    if (c->needs_patch) {
        ICON_ARG(k_total == 0 || d_signs_global != nullptr, "icon_grid_slab_finish: sign list is null");
        fs.mode = kSignGlobal; fs.list = d_signs_global; fs.k_host = k_total; fs.rank_offset = rank_offset;
    }
    work->slab_ready = false;
    return call_finish(*c, mlp, fs, d_occ, precision, work, (hipStream_t)stream, z0, z1);
}

extern "C" int icon_grid_slab_finish_gathered(const icon_mlp_t *mlp, int res, int z0, int z1, int za, int zb,
                                              const void *d_gathered, int64_t stride, int world, int rank,
                                              float *d_occ, int precision, icon_work_t *work, void *stream)
{
    ICON_ARG(mlp && work && d_occ, "icon_grid_slab_finish_gathered: null argument");
    QueryCall *c = prepared_slab(work, res, z0, z1);
    if (!c) return fail(ICON_ERR_STATE, "icon_grid_slab_finish_gathered: no matching icon_grid_slab_features call on this workspace");
    ICON_ARG(za >= z0 && zb > za && zb <= z1, "icon_grid_slab_finish_gathered: planes [za, zb) must lie inside the slab");
    ICON_ARG(c->c0 == mlp->c0, "icon_grid_slab_finish_gathered: MLP input width does not match the feature layout");
    SignSrc fs{};
    if (c->needs_patch) {
        if (d_gathered) {
            ICON_ARG(world >= 1 && world <= kMaxWorld && rank >= 0 && rank < world, "icon_grid_slab_finish_gathered: bad world / rank");
            ICON_ARG(stride >= 8 && (stride & 7) == 0, "icon_grid_slab_finish_gathered: stride must be a multiple of 8 (int64 header)");
            fs.mode = kSignSeg; fs.gathered = (const int8_t *)d_gathered; fs.stride = stride; fs.world = world; fs.rank = rank;
        } else {
            fs = self_signs(work, true);                                // no exchange: the slab's own list is the whole list
        }
    }
    // the slab stays prepared: its planes may be finished piece by piece (the next icon_grid_slab_features replaces it)
    return call_finish(*c, mlp, fs, d_occ, precision, work, (hipStream_t)stream, za, zb);
}

// ---- the MLP input rows of a call, handed out (regressors whose normalisation runs over the points of the call) ----
static int rows_out(QueryCall &c, float *d_rows, icon_work *work, hipStream_t st)
{
    int rc;
    if ((rc = begin_call(work, c))) return rc;
    if ((rc = call_geometry(c, nullptr, work, st))) return rc;
    if ((rc = materialise_rows(c, work, self_signs(work, c.needs_patch), st))) return rc;
    ICON_HIP(hipMemcpyAsync(d_rows, work->d_x, (size_t)c.N * kXRow * sizeof(float), hipMemcpyDeviceToDevice, st));
    return ICON_OK;
}

extern "C" int icon_query_rows(const icon_mesh_t *mesh, const icon_feat_t *feat, int prior_type, float sdf_clip, int cmap_mode,
                               const float *h_calib, const float *d_calib, const float *d_points, int64_t N, float *d_rows,
                               int search, icon_work_t *work, void *stream)
{
    ICON_ARG(work && d_points && d_rows, "icon_query_rows: null argument");
    ICON_ARG(N >= 0, "icon_query_rows: negative N");
    QueryCall c = query_call("icon_query_rows", Src::Points, feat, prior_type, sdf_clip, cmap_mode, search);
    c.mesh = mesh; c.cal = points_calib(h_calib, d_calib); c.points = d_points; c.N = N;
    const int rc = describe_call(c);
    if (rc) return rc;
    if (N == 0) return ICON_OK;
    return rows_out(c, d_rows, work, (hipStream_t)stream);
}

extern "C" int icon_grid_rows(const icon_mesh_t *mesh, const icon_feat_t *feat, int prior_type, float sdf_clip, int cmap_mode,
                              int res, int z0, int z1, float *d_rows, int search, icon_work_t *work, void *stream)
{
    ICON_ARG(work && d_rows, "icon_grid_rows: null argument");
    QueryCall c = query_call("icon_grid_rows", Src::Lattice, feat, prior_type, sdf_clip, cmap_mode, search);
    c.mesh = mesh;
    int rc = describe_call(c);
    if (rc) return rc;
    // no shell skip: the rows of the shell are inputs of the call's statistics like any other (HGPIFuNet.py:361-363 masks afterwards)
    if ((rc = lattice_map(res, z0, z1, nullptr, sdf_clip, false, &c.L))) return rc;
    c.N = (int64_t)c.L.nz * res * res;
    ICON_ARG(c.N < (1ll << 31), "icon_grid_rows: more than 2^31 points in one slab");
    return rows_out(c, d_rows, work, (hipStream_t)stream);
}

// k_walk_stats over the planes [z0, z1) of the res^3 lattice: clamp < 0 - the walk this mesh runs ("pair_box" / "node_box" /
// "box_clamp" as they were when the mesh was created)
constexpr int kWalkStatWords = 8;
static int walk_stats(const icon_mesh_t *mesh, int res, int z0, int z1, int clamp, unsigned long long h[kWalkStatWords])
{
    LatticeMap L;
    int rc = lattice_map(res, z0, z1, mesh, 0.05f, true, &L);
    if (rc) return rc;
    unsigned long long *d = nullptr;
    ICON_HIP(hipMalloc((void **)&d, kWalkStatWords * sizeof(unsigned long long)));
    ICON_HIP(hipMemset(d, 0, kWalkStatWords * sizeof(unsigned long long)));
    if (clamp < 0 ? mesh->dev.box_clamp : clamp) hipLaunchKernelGGL(k_walk_stats<true>, dim3((unsigned)(L.tx * L.ty * L.tz)), dim3(kBlock), 0, 0, mesh->dev, L, d);
    else hipLaunchKernelGGL(k_walk_stats<false>, dim3((unsigned)(L.tx * L.ty * L.tz)), dim3(kBlock), 0, 0, mesh->dev, L, d);
    hipError_t e = hipMemcpy(h, d, kWalkStatWords * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(ICON_ERR_HIP, std::string("walk stats: ") + hipGetErrorString(e));
    return ICON_OK;
}
// out = [packets, inner nodes visited, triangles of the visited leaves, longest walk] of the un-clamped walk (pair_box_bound)
extern "C" int icon_debug_traversal_stats(const icon_mesh_t *mesh, int res, int z0, int z1, uint64_t out[4])
{
    ICON_ARG(mesh && out, "icon_debug_traversal_stats: null argument");
    unsigned long long h[kWalkStatWords];
    int rc = walk_stats(mesh, res, z0, z1, 0, h);
    if (rc) return rc;
    out[0] = h[0]; out[1] = h[1]; out[2] = h[6]; out[3] = h[7];
    return ICON_OK;
}
// out = [packets, inner nodes visited (AABB and oriented parents together), leaf pairs offered to the distance test, leaf pairs
// tested, leaves visited, oriented parents visited] for the walk this mesh runs; icon_debug_pair_stats: the first four
extern "C" int icon_debug_walk_stats(const icon_mesh_t *mesh, int res, int z0, int z1, uint64_t out[6])
{
    ICON_ARG(mesh && out, "icon_debug_walk_stats: null argument");
    unsigned long long h[kWalkStatWords];
    int rc = walk_stats(mesh, res, z0, z1, -1, h);
    if (rc) return rc;
    for (int k = 0; k < 6; ++k) out[k] = h[k];
    return ICON_OK;
}
extern "C" int icon_debug_pair_stats(const icon_mesh_t *mesh, int res, int z0, int z1, uint64_t out[4])
{
    ICON_ARG(mesh && out, "icon_debug_pair_stats: null argument");
    unsigned long long h[kWalkStatWords];
    int rc = walk_stats(mesh, res, z0, z1, -1, h);
    if (rc) return rc;
    for (int k = 0; k < 4; ++k) out[k] = h[k];
    return ICON_OK;
}

extern "C" int icon_grid_eval_slab(const icon_mesh_t *mesh, const icon_feat_t *feat, const icon_mlp_t *mlp,
                                   int prior_type, float sdf_clip, int cmap_mode,
                                   int res, int z0, int z1, float *d_occ,
                                   int search, int precision, icon_work_t *work, void *stream)
{
    ICON_ARG(mlp && work && d_occ, "icon_grid_eval_slab: null argument");
    int rc = icon_grid_slab_features(mesh, feat, prior_type, sdf_clip, cmap_mode, res, z0, z1, nullptr, nullptr, search, work, stream);
    if (rc) return rc;
    QueryCall &c = work->slab;
    ICON_ARG(c.c0 == mlp->c0, "icon_grid_eval_slab: MLP input width does not match the feature layout");
    // the slab's own sign list is the whole list (single call == whole lattice or caller's choice)
    work->slab_ready = false;
    return call_finish(c, mlp, self_signs(work, c.needs_patch), d_occ, precision, work, (hipStream_t)stream, z0, z1);
}

extern "C" int icon_sdf_query_ties(const icon_mesh_t *mesh, const float *d_points, int64_t N,
                                   int32_t *d_face, int32_t *d_face2, uint8_t *d_ulps, void *stream)
{
    ICON_ARG(mesh && d_points && d_face && d_face2 && d_ulps, "icon_sdf_query_ties: null argument");
    ICON_ARG(N >= 0, "icon_sdf_query_ties: negative N");
    if (N == 0) return ICON_OK;
    const int64_t nb = (N + kBlock - 1) / kBlock;
    ICON_ARG(nb < (1ll << 31), "icon_sdf_query_ties: N too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    icon_work tmp;
    const int32_t *perm = nullptr;
    int rc = morton_order(&tmp, d_points, kIdentCalib, nullptr, N, st, &perm);
    if (!rc) {
        hipLaunchKernelGGL(k_nearest_ties, dim3((unsigned)nb), dim3(kBlock), 0, st, mesh->dev, d_points, N, perm, d_face, d_face2, d_ulps);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = fail(ICON_ERR_HIP, "icon_sdf_query_ties: launch failed");
    }
    (void)hipFree(tmp.d_sort_keys); (void)hipFree(tmp.d_sort_idx); (void)hipFree(tmp.d_sort_tmp);
    return rc;
}

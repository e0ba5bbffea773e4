// render_normal.hip - normal maps and depth maps of a mesh from ICON's four orthographic cameras (lib/common/render.py
// Render.load_meshes / get_rgb_image / get_depth_map: pytorch3d MeshRasterizer + cleanShader; call sites
// lib/dataset/TestDataset.py:289-299, apps/ICON.py:387-392, apps/infer.py:423/448/482).
//
// The rule (PARITY UNPINNED): pytorch3d's rasteriser for RasterizationSettings(image_size=S,
// blur_radius=log(1/1e-4)*1e-7, faces_per_pixel=30) under FoVOrthographicCameras(+-100, scale 100) restated in float32, with
// the softmax blend (gamma = 1e-8) replaced by its limit: the candidate of smallest (depth bits, face id) wins.
//   The cameras, the pixel centres, the face test |area| > 1e-8, the barycentrics w_k = ef_k / (area + 1e-8), their clamp and the
//   depth (b0 D0 + b1 D1) + b2 D2 are raster_device.h's, shared with silhouette.hip and render_normal_bwd.hip.  The normal maps'
//   own (rs_normal_*, there too since turntable.hip renders the video's frames by it): a face is a candidate at a pixel centre p inside its bounding box grown by sqrt(blur) when its three barycentrics are all > 0 or
//   the squared distance of p to its nearest edge is < blur, and its depth is not negative.
//   Colour of the winner: ((b0 t0 + b1 t1) + b2 t2 - 0.5) * 2 per channel, t = (n + 1) * 0.5, n the S1 vertex normal.
//   Background: colour 0, depth -1, face -1.
// Every expression is written out in the order it is evaluated in (this file is compiled with -ffp-contract=off), here as there, and
// tests/render_checker.py render_f32 states the same expressions in numpy: face ids, depths and colours are compared for equality.
//
// Shape of the work: one stream-ordered call; every buffer lives in the caller's scratch (icon_render_bytes); nothing is
// allocated, read back or waited for.  The S1 normals of ALL vertices come from the count / scan / fill / ordered-add kernels
// of s1_normals_device.h (shared with query_color.hip, which computes them only where a vertex is hidden: S1Ctx::vis is null here);
// this file keeps the per-vertex kernel of the short lists and the functor that stores a normal into the scratch.
// One raster launch covers every requested view (blockIdx.y); kRsLanes lanes - or one thread - sweep the pixel centres of a
// face's box and atomicMin the 64-bit key into the view's S x S z-buffer; a box above 64 pixels per lane is appended to a
// device-side list that a fixed grid of workgroups consumes.  The resolve pass recomputes the winner's clamped barycentrics
// with the same function and writes colour, depth and face id, the cam-2 left-right flip of the two-view call in the store address.
#pragma clang fp contract(off)

#include "raster_device.h"

namespace icon {

int g_rn_lanes = 0;       // icon_debug_set_option("rn_lanes"): 0 = by the sizes (rs_lanes); 1 = a thread per face; 8 = eight lanes per face

namespace {

struct RnCtx : RsCtx {               // vis null: every vertex gets a normal
    float *images, *depth; int *pix;
    int *n_big, *big;                // the deferred list (raster_device.h) [n_views F] and its length in the header
    float *nrm;                      // [V][3] S1 normals
    unsigned long long *zb;          // [n_views][S][S], image orientation
};

// face f as camera `cam` sees it.  false: nothing to rasterise (bad index, zero area, box off the image)
template <class IT>
__device__ __forceinline__ bool rn_setup(const RnCtx &c, int cam, int64_t f, RsNormalFace &r)
{
    if (!s1_face<IT>(c, f, r.id)) return false;
    rs_project(c, cam, r.id, r.X, r.Y, r.D);
    return rs_normal_setup(r, c.S);
}

// mirrored pixel (i, j) of face f in view `view`: both in [0, S)
__device__ __forceinline__ void rn_pixel(const RnCtx &c, const RsNormalFace &r, int view, int64_t f, int i, int j)
{
    rs_normal_pixel(c.zb + (size_t)view * c.S * c.S, c.S, r, f, i, j);
}

// G lanes per face, 256 / G faces per workgroup; blockIdx.y: the view
template <class IT, int G>
__global__ __launch_bounds__(256) void k_rn_raster(RnCtx c)
{
    const int64_t f = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x % G;
    const int view = blockIdx.y;
    if (f >= c.F) return;
    RsNormalFace r;
    if (!rn_setup<IT>(c, c.cam(view), f, r)) return;
    if (r.box.n() > kRsBigPerLane * G) {
        if (sub == 0) rs_defer(c, c.n_big, c.big, view, f);
        return;
    }
    rs_sweep<G>(r.box, sub, [&](int i, int j) { rn_pixel(c, r, view, f, i, j); });
}

// the deferred faces: a workgroup per entry, as many rounds as the list (read from device memory) needs
template <class IT>
__global__ __launch_bounds__(256) void k_rn_raster_big(RnCtx c)
{
    const int nb = rs_deferred_count(c, c.n_big);
    for (int e = blockIdx.x; e < nb; e += gridDim.x) {
        int view;
        int64_t f;
        RsNormalFace r;
        if (!rs_deferred(c, c.big, e, view, f) || !rn_setup<IT>(c, c.cam(view), f, r)) continue;
        rs_sweep_block(r.box, [&](int i, int j) { rn_pixel(c, r, view, f, i, j); });
    }
}

// one thread per pixel and view: the winner's colour, depth and face id
template <class IT>
__global__ __launch_bounds__(256) void k_rn_resolve(RnCtx c)
{
    const int npx = c.S * c.S;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int view = blockIdx.y, cam = c.cam(view);
    if (p >= npx) return;
    const int row = p / c.S, col = p - row * c.S;
    const int i = c.S - 1 - col, j = c.S - 1 - row;
    const size_t at = rs_at(c, cam, i, j);
    const unsigned long long key = c.zb[(size_t)view * npx + p];
    float rgb[3] = { 0.0f, 0.0f, 0.0f }, pz = -1.0f;
    int face = -1;
    RsNormalFace r;
    RsBary q;
    // a face in the z-buffer passed rn_setup and rs_normal_eval at this pixel: the same expressions give the same answer
    if (key != ~0ull && (int64_t)(key & 0xffffffffull) < c.F && rn_setup<IT>(c, cam, (int64_t)(uint32_t)(key & 0xffffffffull), r) &&
        rs_normal_eval(r, rs_centre(i, c.S), rs_centre(j, c.S), q, pz)) {
        face = (int)(uint32_t)(key & 0xffffffffull);
        const float *n0 = c.nrm + 3 * r.id[0], *n1 = c.nrm + 3 * r.id[1], *n2 = c.nrm + 3 * r.id[2];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            rgb[ch] = (rs_normal_texel(q, n0, n1, n2, ch) - 0.5f) * 2.0f;
    } else {
        pz = -1.0f;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        c.images[((size_t)view * 3 + ch) * npx + at] = rgb[ch];
    if (c.depth) c.depth[(size_t)view * npx + at] = pz;
    if (c.pix) c.pix[(size_t)view * npx + at] = face;
}

// a normal into the scratch: n = s / max(|s|, 1e-6)
struct RnStore {
    float *nrm;
    __device__ void operator()(int64_t v, float x, float y, float z) const
    {
        s1_normalise(x, y, z);
        nrm[3 * v] = x; nrm[3 * v + 1] = y; nrm[3 * v + 2] = z;
    }
};

// one thread per vertex: the normal of a short incidence list; a long one goes to k_s1_normals_long's list
template <class IT>
__global__ __launch_bounds__(256) void k_rn_normals(RnCtx c)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= c.V) return;
    const int n = c.deg[v];
    if (n > kShort) { s1_defer_long(c, v); return; }
    float s[3];
    s1_sum_short<IT>(c, v, n, s);
    RnStore{c.nrm}(v, s[0], s[1], s[2]);
}

struct RnLayout { S1Layout s1; size_t nrm, zb, total; };            // the deferred list: s1.mid

RnLayout rn_layout(int64_t V, int64_t F, int S, int n_views)
{
    RnLayout L{};
    ScratchTake take;
    L.s1 = s1_layout(take, V, F, (size_t)F * 4 * n_views);
    L.nrm = take((size_t)V * 12);
    L.zb = take((size_t)n_views * S * S * 8);
    L.total = take.o;
    return L;
}

template <class IT>
void rn_launch(const RnCtx &c, hipStream_t st)
{
    const dim3 gR((unsigned)((c.F * rs_lanes(c) + 255) / 256), (unsigned)c.n_views);
    if (rs_lanes(c) == 1) hipLaunchKernelGGL((k_rn_raster<IT, 1>), gR, dim3(256), 0, st, c);
    else hipLaunchKernelGGL((k_rn_raster<IT, 8>), gR, dim3(256), 0, st, c);
    hipLaunchKernelGGL(k_rn_raster_big<IT>, dim3(kRsBigGrid), dim3(256), 0, st, c);
    const S1Ctx &s1 = c;                                                   // the shared kernels take the base alone
    s1_launch_lists<IT>(s1, st);
    hipLaunchKernelGGL(k_rn_normals<IT>, dim3((unsigned)((c.V + 255) / 256)), dim3(256), 0, st, c);
    hipLaunchKernelGGL((k_s1_normals_long<IT, RnStore>), dim3(kLongGrid), dim3(64), 0, st, s1, RnStore{c.nrm});
    hipLaunchKernelGGL(k_rn_resolve<IT>, dim3((unsigned)((c.S * c.S + 255) / 256), (unsigned)c.n_views), dim3(256), 0, st, c);
}

}  // namespace
}  // namespace icon

using namespace icon;

extern "C" int icon_render_bytes(int64_t V, int64_t F, int size, int n_views, int64_t *bytes)
{
    ICON_ARG(bytes != nullptr, "icon_render_bytes: null argument");
    const int rc = rs_check_sizes("icon_render_normal", V, F, size, n_views);
    if (rc) return rc;
    *bytes = (int64_t)rn_layout(V, F, size, n_views).total;
    return ICON_OK;
}

extern "C" int icon_render_normal(const float *d_verts, int64_t V, const void *d_faces, int64_t F, int faces_int64,
                                  const int *cam_ids, int n_views, int size, float *d_images, float *d_depth, int32_t *d_pix_to_face,
                                  void *d_scratch, int64_t scratch_bytes, void *stream)
{
    ICON_ARG(d_verts && d_faces && cam_ids && d_images && d_scratch, "icon_render_normal: null argument");
    const RnLayout L = rn_layout(V, F, size, n_views);
    RnCtx c{};
    const int rc = rs_context("icon_render_normal", "icon_render_bytes", d_verts, V, d_faces, F, cam_ids, n_views, size,
                              d_scratch, scratch_bytes, L.total, c);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    char *s = static_cast<char *>(d_scratch);
    c.images = d_images; c.depth = d_depth; c.pix = d_pix_to_face;
    c.n_big = &s1_bind(c, s, L.s1)->n_big; c.big = reinterpret_cast<int *>(s + L.s1.mid);
    c.nrm = reinterpret_cast<float *>(s + L.nrm); c.zb = reinterpret_cast<unsigned long long *>(s + L.zb);
    rs_clear(s, L.s1, c.zb, (size_t)n_views * size * size, st);
    if (faces_int64) rn_launch<int64_t>(c, st); else rn_launch<int32_t>(c, st);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

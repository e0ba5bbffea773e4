// render_normal.hip - normal maps and depth maps of a mesh from ICON's four orthographic cameras (lib/common/render.py
// Render.load_meshes / get_rgb_image / get_depth_map: pytorch3d MeshRasterizer + cleanShader; call sites
// lib/dataset/TestDataset.py:289-299, apps/ICON.py:387-392, apps/infer.py:423/448/482).
//
// The rule (PARITY UNPINNED): pytorch3d's rasteriser for RasterizationSettings(image_size=S,
// blur_radius=log(1/1e-4)*1e-7, faces_per_pixel=30) under FoVOrthographicCameras(+-100, scale 100) restated in float32, with
// the softmax blend (gamma = 1e-8) replaced by its limit: the candidate of smallest (depth bits, face id) wins.
//   NDC of a vertex, as pytorch3d sees it (+X is left, +Y is up), and its view depth:
//     cam 0 (eye +z): X = -x, D = 100 - z      cam 1 (eye +x): X = +z, D = 100 - x
//     cam 2 (eye -z): X = +x, D = 100 + z      cam 3 (eye -x): X = -z, D = 100 + x         Y = y
//   pixel (row r, column c) has its centre at X = -1 + (2 (S-1-c) + 1) / S, Y = -1 + (2 (S-1-r) + 1) / S.
//   A face with |area| > 1e-8 is a candidate at a pixel centre p inside its bounding box grown by sqrt(blur) when its three
//   barycentrics w_k = ef_k / (area + 1e-8) are all > 0 or the squared distance of p to its nearest edge is < blur.  Its
//   barycentrics are clamped to [0, 1] and divided by max(sum, 1e-5); its depth is (b0 D0 + b1 D1) + b2 D2 (skipped if < 0).
//   Colour of the winner: ((b0 t0 + b1 t1) + b2 t2 - 0.5) * 2 per channel, t = (n + 1) * 0.5, n the S1 vertex normal.
//   Background: colour 0, depth -1, face -1.
// Every expression is written out in the order it is evaluated in (this file is compiled with -ffp-contract=off) and
// tests/render_checker.py render_f32 states the same expressions in numpy: face ids, depths and colours are compared for equality.
//
// Shape of the work: one stream-ordered call; every buffer lives in the caller's scratch (icon_render_bytes); nothing is
// allocated, read back or waited for.  The S1 normals of ALL vertices come from the count / scan / fill / ordered-add kernels
// of s1_normals_device.h (shared with query_color.hip, which computes them only where a vertex is hidden: S1Ctx::vis is null here);
// this file keeps the per-vertex kernel of the short lists and the functor that stores a normal into the scratch.
// One raster launch covers every requested view (blockIdx.y); kRnLanes lanes - or one thread - sweep the pixel centres of a
// face's box and atomicMin the 64-bit key into the view's S x S z-buffer; a box above 64 pixels per lane is appended to a
// device-side list that a fixed grid of workgroups consumes.  The resolve pass recomputes the winner's clamped barycentrics
// with the same function and writes colour, depth and face id, the cam-2 left-right flip of the two-view call in the store address.
#pragma clang fp contract(off)

#include "s1_normals_device.h"

namespace icon {

int g_rn_lanes = 0;       // icon_debug_set_option("rn_lanes"): 0 = by the sizes (rn_launch); 1 = a thread per face; 8 = eight lanes per face

namespace {

constexpr int kRnLanes = 8;          // lanes per face of the rasteriser while faces are large; one thread per face otherwise (rn_launch)
constexpr int kRnBigPerLane = 64;    // a bounding box of more than this many pixels per lane goes to the deferred list
constexpr int kRnBigGrid = 1024;     // workgroups (256 lanes, one deferred face at a time each)
constexpr float kRnBlur = 9.210340295e-07f;     // float32(log(1 / 1e-4) * 1e-7): squared NDC distance
constexpr float kRnBlurR = 9.597051539e-04f;    // float32 sqrt of it: the bounding box grows by this
constexpr float kRnEps = 1e-8f;                 // pytorch3d's kEpsilon

struct RnHdr { int bad_faces, n_big, n_long, pad; };

struct RnCtx : S1Ctx {               // the mesh and the normals' scratch (vis null: every vertex gets a normal), and
    int S, n_views, cams, flip;      // cams: 2 bits per view; flip: the two-view call mirrors cam 2 left-right
    float *images, *depth; int *pix;
    RnHdr *hdr;
    int *big;                        // deferred (view << 29 | face) [n_views F]
    float *nrm;                      // [V][3] S1 normals
    unsigned long long *zb;          // [n_views][S][S], image orientation
};

__device__ __forceinline__ float rn_ef(float px, float py, float ax, float ay, float bx, float by)
{
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}
__device__ __forceinline__ float rn_max(float a, float b) { return (a > b) ? a : b; }
__device__ __forceinline__ float rn_min(float a, float b) { return (b < a) ? b : a; }

// squared distance of p to the segment a b (pytorch3d PointLineDistanceForward)
__device__ __forceinline__ float rn_seg(float px, float py, float ax, float ay, float bx, float by)
{
    const float dx = bx - ax, dy = by - ay;
    const float l2 = dx * dx + dy * dy;
    float qx = bx, qy = by;
    if (!(l2 <= kRnEps)) {
        const float t = (dx * (px - ax) + dy * (py - ay)) / l2;
        const float tt = rn_min(rn_max(t, 0.0f), 1.0f);
        qx = ax + tt * dx; qy = ay + tt * dy;
    }
    const float ex = px - qx, ey = py - qy;
    return ex * ex + ey * ey;
}

struct RnRast {
    float X[3], Y[3], D[3];
    float xlo, xhi, ylo, yhi, den;   // the bounding box grown by kRnBlurR; area + eps
    int i0, j0, w, n;                // pixel box in MIRRORED indices (i = S-1-column, j = S-1-row: NDC +X is left, +Y is up)
    int64_t id[3];
};

// face f as camera `cam` sees it.  false: nothing to rasterise (bad index, zero area, box off the image)
template <class IT>
__device__ __forceinline__ bool rn_setup(const RnCtx &c, int cam, int64_t f, RnRast &r)
{
    if (!s1_face<IT>(c, f, r.id)) return false;
    const bool side = (cam & 1) != 0, neg = (cam == 0 || cam == 3), front = cam < 2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float *p = c.verts + 3 * r.id[k];
        const float xa = side ? p[2] : p[0], za = side ? p[0] : p[2];
        r.X[k] = neg ? -xa : xa; r.Y[k] = p[1]; r.D[k] = front ? 100.0f - za : 100.0f + za;
    }
    const float area = rn_ef(r.X[2], r.Y[2], r.X[0], r.Y[0], r.X[1], r.Y[1]);
    if (!(fabsf(area) > kRnEps)) return false;
    r.den = area + kRnEps;
    r.xlo = rn_min(r.X[0], rn_min(r.X[1], r.X[2])) - kRnBlurR; r.xhi = rn_max(r.X[0], rn_max(r.X[1], r.X[2])) + kRnBlurR;
    r.ylo = rn_min(r.Y[0], rn_min(r.Y[1], r.Y[2])) - kRnBlurR; r.yhi = rn_max(r.Y[0], rn_max(r.Y[1], r.Y[2])) + kRnBlurR;
    // centre of mirrored index i: -1 + (2 i + 1) / S.  xlo <= centre <= xhi needs (xlo + 1) S / 2 - 1/2 <= i <= (xhi + 1) S / 2 - 1/2:
    // floor of the products without the halves is wider by up to half a pixel on each side (their rounding is ~1e-4 pixel).
    // Clamped as floats: what is converted to int lies in [-1, S], whatever the coordinates are (NaN included)
    const float fS = (float)c.S;
    const int i0 = (int)floorf(fminf(fmaxf((r.xlo + 1.0f) * 0.5f * fS, 0.0f), fS));
    const int i1 = (int)floorf(fminf(fmaxf((r.xhi + 1.0f) * 0.5f * fS, -1.0f), fS - 1.0f));
    const int j0 = (int)floorf(fminf(fmaxf((r.ylo + 1.0f) * 0.5f * fS, 0.0f), fS));
    const int j1 = (int)floorf(fminf(fmaxf((r.yhi + 1.0f) * 0.5f * fS, -1.0f), fS - 1.0f));
    if (i0 > i1 || j0 > j1) return false;
    r.i0 = i0; r.j0 = j0; r.w = i1 - i0 + 1; r.n = r.w * (j1 - j0 + 1);   // <= S^2 <= 2^22
    return true;
}

// the per-pixel rule: is the face a candidate at the pixel centre (px, py); its clamped barycentrics and depth
__device__ __forceinline__ bool rn_eval(const RnRast &r, float px, float py, float b[3], float &pz)
{
    if (!(px >= r.xlo && px <= r.xhi && py >= r.ylo && py <= r.yhi)) return false;
    const float w0 = rn_ef(px, py, r.X[1], r.Y[1], r.X[2], r.Y[2]) / r.den;
    const float w1 = rn_ef(px, py, r.X[2], r.Y[2], r.X[0], r.Y[0]) / r.den;
    const float w2 = rn_ef(px, py, r.X[0], r.Y[0], r.X[1], r.Y[1]) / r.den;
    if (!(w0 > 0.0f && w1 > 0.0f && w2 > 0.0f)) {
        const float d01 = rn_seg(px, py, r.X[0], r.Y[0], r.X[1], r.Y[1]);
        const float d02 = rn_seg(px, py, r.X[0], r.Y[0], r.X[2], r.Y[2]);
        const float d12 = rn_seg(px, py, r.X[1], r.Y[1], r.X[2], r.Y[2]);
        if (!(rn_min(rn_min(d01, d02), d12) < kRnBlur)) return false;
    }
    const float c0 = rn_max(rn_min(w0, 1.0f), 0.0f), c1 = rn_max(rn_min(w1, 1.0f), 0.0f), c2 = rn_max(rn_min(w2, 1.0f), 0.0f);
    const float s = rn_max((c0 + c1) + c2, 1e-5f);
    b[0] = c0 / s; b[1] = c1 / s; b[2] = c2 / s;
    pz = (b[0] * r.D[0] + b[1] * r.D[1]) + b[2] * r.D[2];
    return !(pz < 0.0f);
}

__device__ __forceinline__ float rn_centre(int i, int S) { return -1.0f + (float)(2 * i + 1) / (float)S; }

// mirrored pixel (i, j) of face f in view `view`: both in [0, S)
__device__ __forceinline__ void rn_pixel(const RnCtx &c, const RnRast &r, int view, int64_t f, int i, int j)
{
    float b[3], pz;
    if (!rn_eval(r, rn_centre(i, c.S), rn_centre(j, c.S), b, pz)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(pz) << 32) | (unsigned long long)(uint32_t)f;
    atomicMin(&c.zb[((size_t)view * c.S + (size_t)(c.S - 1 - j)) * c.S + (size_t)(c.S - 1 - i)], key);
}

// G lanes per face, 256 / G faces per workgroup; blockIdx.y: the view
template <class IT, int G>
__global__ __launch_bounds__(256) void k_rn_raster(RnCtx c)
{
    const int64_t f = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x % G;
    const int view = blockIdx.y, cam = (c.cams >> (2 * view)) & 3;
    if (f >= c.F) return;
    RnRast r;
    if (!rn_setup<IT>(c, cam, f, r)) return;
    if (r.n > kRnBigPerLane * G) {
        if (sub == 0) {                                                    // at most n_views F entries; F < 2^29
            const int at = atomicAdd(&c.hdr->n_big, 1);
            if ((int64_t)at < c.F * c.n_views) c.big[at] = (view << 29) | (int)f;
        }
        return;
    }
    int j = sub / r.w, i = sub - j * r.w;
    for (int t = sub; t < r.n; t += G) {
        rn_pixel(c, r, view, f, r.i0 + i, r.j0 + j);
        i += G;
        while (i >= r.w) { i -= r.w; ++j; }
    }
}

// the deferred faces: a workgroup per entry, as many rounds as the list (read from device memory) needs
template <class IT>
__global__ __launch_bounds__(256) void k_rn_raster_big(RnCtx c)
{
    const int nb = (int)min((int64_t)c.hdr->n_big, c.F * c.n_views);
    for (int e = blockIdx.x; e < nb; e += gridDim.x) {
        const int code = c.big[e];
        const int view = code >> 29, cam = (c.cams >> (2 * view)) & 3;
        const int64_t f = code & ((1 << 29) - 1);
        if (view < 0 || view >= c.n_views || f >= c.F) continue;
        RnRast r;
        if (!rn_setup<IT>(c, cam, f, r)) continue;
        for (int t = threadIdx.x; t < r.n; t += 256) {
            const int j = t / r.w;
            rn_pixel(c, r, view, f, r.i0 + (t - j * r.w), r.j0 + j);
        }
    }
}

// one thread per pixel and view: the winner's colour, depth and face id
template <class IT>
__global__ __launch_bounds__(256) void k_rn_resolve(RnCtx c)
{
    const int npx = c.S * c.S;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int view = blockIdx.y, cam = (c.cams >> (2 * view)) & 3;
    if (p >= npx) return;
    const int row = p / c.S, col = p - row * c.S;
    const int cs = (c.flip && cam == 2) ? c.S - 1 - col : col;
    const size_t at = ((size_t)view * c.S + row) * c.S + cs;
    const unsigned long long key = c.zb[(size_t)view * npx + p];
    float rgb[3] = { 0.0f, 0.0f, 0.0f }, pz = -1.0f;
    int face = -1;
    RnRast r;
    float b[3];
    // a face in the z-buffer passed rn_setup and rn_eval at this pixel: the same expressions give the same answer
    if (key != ~0ull && (int64_t)(key & 0xffffffffull) < c.F && rn_setup<IT>(c, cam, (int64_t)(uint32_t)(key & 0xffffffffull), r) &&
        rn_eval(r, rn_centre(c.S - 1 - col, c.S), rn_centre(c.S - 1 - row, c.S), b, pz)) {
        face = (int)(uint32_t)(key & 0xffffffffull);
        const float *n0 = c.nrm + 3 * r.id[0], *n1 = c.nrm + 3 * r.id[1], *n2 = c.nrm + 3 * r.id[2];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float t0 = (n0[ch] + 1.0f) * 0.5f, t1 = (n1[ch] + 1.0f) * 0.5f, t2 = (n2[ch] + 1.0f) * 0.5f;
            rgb[ch] = (((b[0] * t0 + b[1] * t1) + b[2] * t2) - 0.5f) * 2.0f;
        }
    } else {
        pz = -1.0f;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        c.images[(((size_t)view * 3 + ch) * c.S + row) * c.S + cs] = rgb[ch];
    if (c.depth) c.depth[at] = pz;
    if (c.pix) c.pix[at] = face;
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

// the call's clears: [0, zero_end) of the scratch to 0, the z-buffers to ~0 - a kernel like the others, so that a captured call
// consists of kernel nodes only
__global__ __launch_bounds__(256) void k_rn_clear(uint32_t *zero, size_t n_zero, unsigned long long *zb, size_t n_zb)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_zero || i < n_zb; i += stride) {
        if (i < n_zero) zero[i] = 0u;
        if (i < n_zb) zb[i] = ~0ull;
    }
}

struct RnLayout { size_t hdr, deg, cur, zero_end, loc, part, inc, tmp, big, longv, nrm, zb, total; };

RnLayout rn_layout(int64_t V, int64_t F, int S, int n_views)
{
    RnLayout L{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = (o + bytes + 255) / 256 * 256; return at; };
    L.hdr = take(sizeof(RnHdr)); L.deg = take((size_t)V * 4); L.cur = take((size_t)V * 4);
    L.zero_end = o;                                                        // [0, zero_end): cleared by one memset per call
    L.loc = take((size_t)V * 4); L.part = take((size_t)((V + kScanItems - 1) / kScanItems) * 4);
    L.inc = take((size_t)F * 12); L.tmp = take((size_t)F * 12);
    L.big = take((size_t)F * 4 * n_views); L.longv = take((size_t)V * 4);
    L.nrm = take((size_t)V * 12);
    L.zb = take((size_t)n_views * S * S * 8);
    L.total = o;
    return L;
}

int rn_check_sizes(int64_t V, int64_t F, int size, int n_views)
{
    ICON_ARG(V > 0 && F > 0 && V < (1ll << 31) && F < (1ll << 29), "icon_render_normal: 0 < V < 2^31, 0 < F < 2^29");
    ICON_ARG(size >= 8 && size <= 2048, "icon_render_normal: size must be 8..2048");
    ICON_ARG(n_views >= 1 && n_views <= 4, "icon_render_normal: n_views must be 1..4");
    return ICON_OK;
}

template <class IT>
void rn_launch(const RnCtx &c, hipStream_t st)
{
    const unsigned gF = (unsigned)((c.F + 255) / 256), gV = (unsigned)((c.V + 255) / 256);
    const int nb = (int)((c.V + kScanItems - 1) / kScanItems);
    // default mapping by the sizes alone (no read-back): eight lanes per face while a face covers many pixels (the SMPL body: 19 pixels
    // of a 512^2 image per face), one thread per face once 8 F exceeds the pixel count (marching-cubes meshes: under 2) - DESIGN.md 4.13
    const int G = g_rn_lanes == 1 ? 1 : (g_rn_lanes == 8 ? 8 : (8 * c.F > (int64_t)c.S * c.S ? 1 : kRnLanes));
    const dim3 gR((unsigned)((c.F * G + 255) / 256), (unsigned)c.n_views);
    if (G == 1) hipLaunchKernelGGL((k_rn_raster<IT, 1>), gR, dim3(256), 0, st, c);
    else hipLaunchKernelGGL((k_rn_raster<IT, 8>), gR, dim3(256), 0, st, c);
    hipLaunchKernelGGL(k_rn_raster_big<IT>, dim3(kRnBigGrid), dim3(256), 0, st, c);
    const S1Ctx &s1 = c;                                                   // the shared kernels take the base alone
    hipLaunchKernelGGL(k_s1_count<IT>, dim3(gF), dim3(256), 0, st, s1);
    hipLaunchKernelGGL(k_s1_scan_blocks, dim3((unsigned)nb), dim3(256), 0, st, s1);
    hipLaunchKernelGGL(k_s1_scan_parts, dim3(1), dim3(1024), 0, st, s1, nb);
    hipLaunchKernelGGL(k_s1_fill<IT>, dim3(gF), dim3(256), 0, st, s1);
    hipLaunchKernelGGL(k_rn_normals<IT>, dim3(gV), dim3(256), 0, st, c);
    hipLaunchKernelGGL((k_s1_normals_long<IT, RnStore>), dim3(kLongGrid), dim3(64), 0, st, s1, RnStore{c.nrm});
    hipLaunchKernelGGL(k_rn_resolve<IT>, dim3((unsigned)((c.S * c.S + 255) / 256), (unsigned)c.n_views), dim3(256), 0, st, c);
}

}  // namespace
}  // namespace icon

using namespace icon;

extern "C" int icon_render_bytes(int64_t V, int64_t F, int size, int n_views, int64_t *bytes)
{
    ICON_ARG(bytes != nullptr, "icon_render_bytes: null argument");
    const int rc = rn_check_sizes(V, F, size, n_views);
    if (rc) return rc;
    *bytes = (int64_t)rn_layout(V, F, size, n_views).total;
    return ICON_OK;
}

extern "C" int icon_render_normal(const float *d_verts, int64_t V, const void *d_faces, int64_t F, int faces_int64,
                                  const int *cam_ids, int n_views, int size, float *d_images, float *d_depth, int32_t *d_pix_to_face,
                                  void *d_scratch, int64_t scratch_bytes, void *stream)
{
    ICON_ARG(d_verts && d_faces && cam_ids && d_images && d_scratch, "icon_render_normal: null argument");
    const int rc = rn_check_sizes(V, F, size, n_views);
    if (rc) return rc;
    int cams = 0;
    for (int k = 0; k < n_views; ++k) {
        ICON_ARG(cam_ids[k] >= 0 && cam_ids[k] <= 3, "icon_render_normal: cam_ids must be 0..3");
        cams |= cam_ids[k] << (2 * k);
    }
    ICON_ARG(((uintptr_t)d_scratch & 255) == 0, "icon_render_normal: the scratch must be 256-byte aligned");
    const RnLayout L = rn_layout(V, F, size, n_views);
    ICON_ARG(scratch_bytes >= (int64_t)L.total, "icon_render_normal: scratch smaller than icon_render_bytes");
    hipStream_t st = (hipStream_t)stream;
    char *s = static_cast<char *>(d_scratch);
    RnCtx c{};
    c.verts = d_verts; c.faces = d_faces; c.V = V; c.F = F; c.S = size; c.n_views = n_views; c.cams = cams; c.flip = n_views == 2 ? 1 : 0;
    c.images = d_images; c.depth = d_depth; c.pix = d_pix_to_face;
    c.hdr = reinterpret_cast<RnHdr *>(s + L.hdr); c.bad_faces = &c.hdr->bad_faces; c.n_long = &c.hdr->n_long;
    c.deg = reinterpret_cast<int *>(s + L.deg); c.cur = reinterpret_cast<int *>(s + L.cur);
    c.loc = reinterpret_cast<int *>(s + L.loc); c.part = reinterpret_cast<int *>(s + L.part);
    c.inc = reinterpret_cast<int *>(s + L.inc); c.tmp = reinterpret_cast<int *>(s + L.tmp); c.big = reinterpret_cast<int *>(s + L.big);
    c.longv = reinterpret_cast<int *>(s + L.longv); c.nrm = reinterpret_cast<float *>(s + L.nrm);
    c.zb = reinterpret_cast<unsigned long long *>(s + L.zb);
    const size_t n_zero = L.zero_end / 4, n_zb = (size_t)n_views * size * size;
    const size_t n_clear = n_zero > n_zb ? n_zero : n_zb;
    hipLaunchKernelGGL(k_rn_clear, dim3((unsigned)((n_clear + 255) / 256 < 2048 ? (n_clear + 255) / 256 : 2048)), dim3(256), 0, st,
                       reinterpret_cast<uint32_t *>(s), n_zero, c.zb, n_zb);
    if (faces_int64) rn_launch<int64_t>(c, st); else rn_launch<int32_t>(c, st);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

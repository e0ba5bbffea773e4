// raster_device.h - the float32 raster rule of ICON's four orthographic cameras, stated once for
// render_normal.hip (normal and depth maps), silhouette.hip (soft silhouette, both directions) and render_normal_bwd.hip (the normal
// maps' gradient): pytorch3d's rasteriser under FoVOrthographicCameras(+-100, scale 100), restated expression by expression.
//   NDC of a vertex, as pytorch3d sees it (+X is left, +Y is up), and its view depth:
//     cam 0 (eye +z): X = -x, D = 100 - z      cam 1 (eye +x): X = +z, D = 100 - x
//     cam 2 (eye -z): X = +x, D = 100 + z      cam 3 (eye -x): X = -z, D = 100 + x         Y = y
//   pixel (row r, column c) has its centre at X = -1 + (2 (S-1-c) + 1) / S, Y = -1 + (2 (S-1-r) + 1) / S: the kernels count pixels in
//   MIRRORED indices i = S-1-c, j = S-1-r.
//   turntable.hip (the video's camera at any azimuth) projects with rs_project_turn and shares everything else.
//   A face is drawn when |area| > 1e-8; at a pixel centre p inside its bounding box grown by sqrt(blur) its barycentrics are
//   w_k = ef_k / (area + 1e-8), clamped to [0, 1] and divided by max(sum, 1e-5); its depth is (b0 D0 + b1 D1) + b2 D2.  The blur
//   radius of the normal maps and the silhouette's differ: every function that needs one takes it as an argument.
// Every function keeps the order its expression is evaluated in (the including files are compiled with -ffp-contract=off, divisions
// are correctly rounded): tests/render_checker.py states the same expressions in numpy and compares for equality.  As in
// s1_normals_device.h everything lives in the including file's anonymous namespace, device functions are forced inline, and
// nothing here holds state; every index taken out of the scratch is range-checked before it is an address.
#pragma once
#pragma clang fp contract(off)

#include "s1_normals_device.h"

namespace icon {
namespace {

constexpr int kRsLanes = 8;          // lanes per face of a sweep while faces are large; one thread per face otherwise (rs_lanes)
constexpr int kRsBigPerLane = 64;    // a pixel box of more than this many pixels per lane goes to the deferred list
constexpr int kRsBigGrid = 1024;     // workgroups (256 lanes, one deferred face at a time each)
constexpr float kRsEps = 1e-8f;      // pytorch3d's kEpsilon
constexpr float kRsMinSum = 1e-5f;   // the clamped barycentrics are divided by max(sum, this)
// the normal maps' blur radius (render_normal.hip; its gradient sweeps the same boxes) - the silhouette's differs and lives in silhouette.hip
constexpr float kRsNormalBlur = 9.210340295e-07f;     // float32(log(1 / 1e-4) * 1e-7): squared NDC distance
constexpr float kRsNormalBlurR = 9.597051539e-04f;    // float32 sqrt of it: the bounding box grows by this

struct RsCtx : S1Ctx {               // the mesh and the S1 scratch, and
    int S, n_views, cams, flip;      // cams: 2 bits per view; flip: the two-view call mirrors cam 2 left-right
    __device__ __forceinline__ int cam(int view) const { return (cams >> (2 * view)) & 3; }
};

__device__ __forceinline__ float rs_ef(float px, float py, float ax, float ay, float bx, float by)
{
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}
__device__ __forceinline__ float rs_max(float a, float b) { return (a > b) ? a : b; }
__device__ __forceinline__ float rs_min(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float rs_centre(int i, int S) { return -1.0f + (float)(2 * i + 1) / (float)S; }

// squared distance of p to the segment a b (pytorch3d PointLineDistanceForward), with what a gradient needs: e = p - q, q the
// nearest point, and the clamped parameter t (1 in the degenerate branch)
struct RsSeg { float d2, ex, ey, t; };
__device__ __forceinline__ RsSeg rs_seg(float px, float py, float ax, float ay, float bx, float by)
{
    const float dx = bx - ax, dy = by - ay;
    const float l2 = dx * dx + dy * dy;
    float qx = bx, qy = by;
    RsSeg s;
    s.t = 1.0f;
    if (!(l2 <= kRsEps)) {
        const float t = (dx * (px - ax) + dy * (py - ay)) / l2;
        s.t = rs_min(rs_max(t, 0.0f), 1.0f);
        qx = ax + s.t * dx; qy = ay + s.t * dy;
    }
    s.ex = px - qx; s.ey = py - qy;
    s.d2 = s.ex * s.ex + s.ey * s.ey;
    return s;
}

// the corners `id` as camera `cam` sees them (a caller that needs no depth passes a D it never reads)
__device__ __forceinline__ void rs_project(const RsCtx &c, int cam, const int64_t id[3], float X[3], float Y[3], float D[3])
{
    const bool side = (cam & 1) != 0, neg = (cam == 0 || cam == 3), front = cam < 2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float *p = c.verts + 3 * id[k];
        const float xa = side ? p[2] : p[0], za = side ? p[0] : p[2];
        X[k] = neg ? -xa : xa; Y[k] = p[1]; D[k] = front ? 100.0f - za : 100.0f + za;
    }
}
// ... as the turntable camera of azimuth a sees them (turntable.hip): eye (100 cos a, 0, 100 sin a), (cs, sn) the
// float32 pair of a.  Each product is rounded, then subtracted, in this order; at (1,0) / (0,1) / (-1,0) / (0,-1) it gives the
// X and D of cam 1 / 0 / 3 / 2 above
__device__ __forceinline__ void rs_project_turn(const RsCtx &c, float cs, float sn, const int64_t id[3], float X[3], float Y[3], float D[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float *p = c.verts + 3 * id[k];
        X[k] = p[2] * cs - p[0] * sn; Y[k] = p[1]; D[k] = (100.0f - p[0] * cs) - p[2] * sn;
    }
}
// ... and a gradient (d/dX, d/dY) taken back onto the world's axes (X = -x, +z, +x, -z for cam 0..3): the addends of incidence key
// 3 f + corner in view `view` out of a [n_views][3 F][2] array; the coordinate along the view's axis gets nothing
__device__ __forceinline__ void rs_world_term(const float *gxy, int64_t F, int cams, int view, int key, float o[3])
{
    o[0] = o[1] = o[2] = 0.0f;
    if (key < 0 || key / 3 >= F) return;
    const float *g = gxy + ((size_t)view * 3 * F + key) * 2;
    const int cam = (cams >> (2 * view)) & 3;
    const float gx = (cam == 0 || cam == 3) ? -g[0] : g[0];
    if (cam & 1) o[2] = gx; else o[0] = gx;
    o[1] = g[1];
}

// the signed area of a projected face; it is drawn when rs_drawn(area), and its barycentrics divide by area + kRsEps
__device__ __forceinline__ float rs_area(const float X[3], const float Y[3]) { return rs_ef(X[2], Y[2], X[0], Y[0], X[1], Y[1]); }
__device__ __forceinline__ bool rs_drawn(float area) { return fabsf(area) > kRsEps; }

// the bounding box of a projected face grown by `grow` (the sqrt of the caller's blur radius)
struct RsBounds { float xlo, xhi, ylo, yhi; };
__device__ __forceinline__ RsBounds rs_bounds(const float X[3], const float Y[3], float grow)
{
    RsBounds b;
    b.xlo = rs_min(X[0], rs_min(X[1], X[2])) - grow; b.xhi = rs_max(X[0], rs_max(X[1], X[2])) + grow;
    b.ylo = rs_min(Y[0], rs_min(Y[1], Y[2])) - grow; b.yhi = rs_max(Y[0], rs_max(Y[1], Y[2])) + grow;
    return b;
}

// ... as a box of MIRRORED pixel indices clipped to the image: 0 <= i0 <= i1 < S, 0 <= j0 <= j1 < S unless it is empty
struct RsBox {
    int i0, i1, j0, j1;
    __device__ __forceinline__ bool empty() const { return i0 > i1 || j0 > j1; }
    __device__ __forceinline__ int w() const { return i1 - i0 + 1; }
    __device__ __forceinline__ int n() const { return w() * (j1 - j0 + 1); }     // <= S^2 <= 2^22
};
__device__ __forceinline__ RsBox rs_box(const RsBounds &b, int S)
{
    // centre of mirrored index i: -1 + (2 i + 1) / S.  xlo <= centre <= xhi needs (xlo + 1) S / 2 - 1/2 <= i <= (xhi + 1) S / 2 - 1/2:
    // floor of the products without the halves is wider by up to half a pixel on each side (their rounding is ~1e-4 pixel).
    // Clamped as floats: what is converted to int lies in [-1, S], whatever the coordinates are (NaN included)
    const float fS = (float)S;
    RsBox q;
    q.i0 = (int)floorf(fminf(fmaxf((b.xlo + 1.0f) * 0.5f * fS, 0.0f), fS));
    q.i1 = (int)floorf(fminf(fmaxf((b.xhi + 1.0f) * 0.5f * fS, -1.0f), fS - 1.0f));
    q.j0 = (int)floorf(fminf(fmaxf((b.ylo + 1.0f) * 0.5f * fS, 0.0f), fS));
    q.j1 = (int)floorf(fminf(fmaxf((b.yhi + 1.0f) * 0.5f * fS, -1.0f), fS - 1.0f));
    return q;
}

// the barycentrics of the pixel centre (px, py): w_k = ef_k / den, den = area + kRsEps
__device__ __forceinline__ void rs_weights(const float X[3], const float Y[3], float den, float px, float py, float w[3])
{
    w[0] = rs_ef(px, py, X[1], Y[1], X[2], Y[2]) / den;
    w[1] = rs_ef(px, py, X[2], Y[2], X[0], Y[0]) / den;
    w[2] = rs_ef(px, py, X[0], Y[0], X[1], Y[1]) / den;
}
__device__ __forceinline__ bool rs_inside(const float w[3]) { return w[0] > 0.0f && w[1] > 0.0f && w[2] > 0.0f; }
// ... clamped to [0, 1] and divided by s = max(sraw, kRsMinSum), sraw their sum; the depth they interpolate
struct RsBary { float b[3], sraw, s; };
__device__ __forceinline__ RsBary rs_bary(const float w[3])
{
    const float c0 = rs_max(rs_min(w[0], 1.0f), 0.0f), c1 = rs_max(rs_min(w[1], 1.0f), 0.0f), c2 = rs_max(rs_min(w[2], 1.0f), 0.0f);
    RsBary q;
    q.sraw = (c0 + c1) + c2;
    q.s = rs_max(q.sraw, kRsMinSum);
    q.b[0] = c0 / q.s; q.b[1] = c1 / q.s; q.b[2] = c2 / q.s;
    return q;
}
__device__ __forceinline__ float rs_depth(const RsBary &q, const float D[3]) { return (q.b[0] * D[0] + q.b[1] * D[1]) + q.b[2] * D[2]; }

// where the pixel of mirrored indices (i, j) lives in an [S][S] plane of camera `cam`'s view, the cam-2 mirror of the two-view call included
__device__ __forceinline__ size_t rs_at(const RsCtx &c, int cam, int i, int j)
{
    const int row = c.S - 1 - j, col = c.S - 1 - i;
    const int cs = (c.flip && cam == 2) ? c.S - 1 - col : col;
    return (size_t)row * c.S + cs;
}

// ---- the normal maps' own part of the rule, shared by render_normal.hip's four cameras and turntable.hip's any ----
struct RsNormalFace {
    float X[3], Y[3], D[3], den;     // the projected corners (the caller's rs_project / rs_project_turn); den: area + eps
    RsBounds bb;                     // the bounding box grown by kRsNormalBlurR
    RsBox box;
    int64_t id[3];
};
// after id, X, Y and D are filled.  false: nothing to rasterise (zero area, box off the image)
__device__ __forceinline__ bool rs_normal_setup(RsNormalFace &r, int S)
{
    const float area = rs_area(r.X, r.Y);
    if (!rs_drawn(area)) return false;
    r.den = area + kRsEps;
    r.bb = rs_bounds(r.X, r.Y, kRsNormalBlurR);
    r.box = rs_box(r.bb, S);
    return !r.box.empty();
}
// the per-pixel rule: is the face a candidate at the pixel centre (px, py); its clamped barycentrics and depth
__device__ __forceinline__ bool rs_normal_eval(const RsNormalFace &r, float px, float py, RsBary &q, float &pz)
{
    if (!(px >= r.bb.xlo && px <= r.bb.xhi && py >= r.bb.ylo && py <= r.bb.yhi)) return false;
    float w[3];
    rs_weights(r.X, r.Y, r.den, px, py, w);
    if (!rs_inside(w)) {
        const float d01 = rs_seg(px, py, r.X[0], r.Y[0], r.X[1], r.Y[1]).d2;
        const float d02 = rs_seg(px, py, r.X[0], r.Y[0], r.X[2], r.Y[2]).d2;
        const float d12 = rs_seg(px, py, r.X[1], r.Y[1], r.X[2], r.Y[2]).d2;
        if (!(rs_min(rs_min(d01, d02), d12) < kRsNormalBlur)) return false;
    }
    q = rs_bary(w);
    pz = rs_depth(q, r.D);
    return !(pz < 0.0f);
}
// mirrored pixel (i, j), both in [0, S), of face f into a view's [S][S] z-buffer plane (image orientation).  The key: (depth bits,
// face id), the smallest wins
__device__ __forceinline__ void rs_normal_pixel(unsigned long long *zb, int S, const RsNormalFace &r, int64_t f, int i, int j)
{
    RsBary q;
    float pz;
    if (!rs_normal_eval(r, rs_centre(i, S), rs_centre(j, S), q, pz)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(pz) << 32) | (unsigned long long)(uint32_t)f;
    atomicMin(&zb[(size_t)(S - 1 - j) * S + (size_t)(S - 1 - i)], key);
}
// the winner's blend of its corners' t = (n + 1) * 0.5 in channel ch: the image holds (t - 0.5) * 2, a video frame (uint8) (t * 255)
__device__ __forceinline__ float rs_normal_texel(const RsBary &q, const float *n0, const float *n1, const float *n2, int ch)
{
    const float t0 = (n0[ch] + 1.0f) * 0.5f, t1 = (n1[ch] + 1.0f) * 0.5f, t2 = (n2[ch] + 1.0f) * 0.5f;
    return (q.b[0] * t0 + q.b[1] * t1) + q.b[2] * t2;
}

// G lanes sweep a face's box: lane `sub` takes pixels sub, sub + G, ... in row order and calls fn(i, j)
template <int G, class Fn>
__device__ __forceinline__ void rs_sweep(const RsBox &q, int sub, Fn fn)
{
    const int w = q.w(), n = q.n();
    int j = sub / w, i = sub - j * w;
    for (int t = sub; t < n; t += G) {
        fn(q.i0 + i, q.j0 + j);
        i += G;
        while (i >= w) { i -= w; ++j; }
    }
}
// ... and a workgroup of 256 a deferred face's
template <class Fn>
__device__ __forceinline__ void rs_sweep_block(const RsBox &q, Fn fn)
{
    const int w = q.w(), n = q.n();
    for (int t = threadIdx.x; t < n; t += 256) {
        const int j = t / w;
        fn(q.i0 + (t - j * w), q.j0 + j);
    }
}

// the deferred list: (view << 29 | face), at most n_views F entries (F < 2^29), its length in the header's n_big
__device__ __forceinline__ void rs_defer(const RsCtx &c, int *n_big, int *big, int view, int64_t f)
{
    const int at = atomicAdd(n_big, 1);
    if ((int64_t)at < c.F * c.n_views) big[at] = (view << 29) | (int)f;
}
__device__ __forceinline__ int rs_deferred_count(const RsCtx &c, const int *n_big) { return (int)min((int64_t)*n_big, c.F * c.n_views); }
// entry e; false: it names no (view, face) of this call
__device__ __forceinline__ bool rs_deferred(const RsCtx &c, const int *big, int e, int &view, int64_t &f)
{
    const int code = big[e];
    view = code >> 29; f = code & ((1 << 29) - 1);
    return view >= 0 && view < c.n_views && f < c.F;
}

// a call of more views than the two bits above name (turntable.hip) keeps ONE LIST PER VIEW of the chunk it is rasterising: the view
// is the list's index, an entry the face alone (below 2^29); list `lv` holds at most F entries at big[lv F ..], its length in n_big[lv]
__device__ __forceinline__ void rs_defer_view(int *n_big, int *big, int64_t F, int lv, int64_t f)
{
    const int at = atomicAdd(&n_big[lv], 1);
    if (at >= 0 && (int64_t)at < F) big[(size_t)lv * F + at] = (int)f;
}
__device__ __forceinline__ int rs_deferred_view_count(const int *n_big, int64_t F, int lv) { return (int)min((int64_t)max(n_big[lv], 0), F); }
// entry e of list lv; false: it names no face of this call
__device__ __forceinline__ bool rs_deferred_view(const int *big, int64_t F, int lv, int e, int64_t &f)
{
    f = big[(size_t)lv * F + e];
    return f >= 0 && f < F;
}

// the call's clears: n_zero words of the scratch to 0, n_zb z-buffer words (0 where a call has none) to ~0 - a kernel like the
// others, so that a captured call consists of kernel nodes only
__global__ __launch_bounds__(256) void k_rs_clear(uint32_t *zero, size_t n_zero, unsigned long long *zb, size_t n_zb)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_zero || i < n_zb; i += stride) {
        if (i < n_zero) zero[i] = 0u;
        if (i < n_zb) zb[i] = ~0ull;
    }
}

// ---- host ----
void rs_clear(void *d_scratch, const S1Layout &L, unsigned long long *zb, size_t n_zb, hipStream_t st)
{
    const size_t n_zero = L.zero_end / 4, n = n_zero > n_zb ? n_zero : n_zb;
    hipLaunchKernelGGL(k_rs_clear, dim3((unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), dim3(256), 0, st,
                       static_cast<uint32_t *>(d_scratch), n_zero, zb, n_zb);
}

// lanes per face of the sweeps, by the sizes alone (no read-back): eight while a face covers many pixels (the SMPL body: 19 pixels of
// a 512^2 image per face), one thread per face once 8 F exceeds the pixel count (marching-cubes meshes: under 2) - DESIGN.md 4.13;
// icon_debug_set_option("rn_lanes") forces 1 or 8
int rs_lanes(const RsCtx &c)
{
    return g_rn_lanes == 1 ? 1 : (g_rn_lanes == 8 ? 8 : (8 * c.F > (int64_t)c.S * c.S ? 1 : kRsLanes));
}

// the checks of an entry `name`: the sizes (all a *_bytes entry needs; max_views: four cameras, or the turntable's frames) ...
int rs_check_sizes(const std::string &name, int64_t V, int64_t F, int size, int n_views, int max_views = 4)
{
    ICON_ARG(V > 0 && F > 0 && V < (1ll << 31) && F < (1ll << 29), name + ": 0 < V < 2^31, 0 < F < 2^29");
    ICON_ARG(size >= 8 && size <= 2048, name + ": size must be 8..2048");
    ICON_ARG(n_views >= 1 && n_views <= max_views, name + ": n_views must be 1.." + std::to_string(max_views));
    return ICON_OK;
}
// ... and the call's: the cameras, the scratch against the `total` its bytes_name entry gives.  Fills the rule's part of the context
int rs_context(const std::string &name, const char *bytes_name, const float *d_verts, int64_t V, const void *d_faces, int64_t F,
               const int *cam_ids, int n_views, int size, const void *d_scratch, int64_t scratch_bytes, size_t total, RsCtx &c)
{
    const int rc = rs_check_sizes(name, V, F, size, n_views);
    if (rc) return rc;
    int cams = 0;
    for (int k = 0; k < n_views; ++k) {
        ICON_ARG(cam_ids[k] >= 0 && cam_ids[k] <= 3, name + ": cam_ids must be 0..3");
        cams |= cam_ids[k] << (2 * k);
    }
    if (const int e = scratch_check(name, bytes_name, d_scratch, scratch_bytes, total)) return e;
    c.verts = d_verts; c.faces = d_faces; c.V = V; c.F = F; c.S = size; c.n_views = n_views; c.cams = cams; c.flip = n_views == 2 ? 1 : 0;
    return ICON_OK;
}

}  // namespace
}  // namespace icon

// query_color.hip - vertex colours of the reconstructed mesh (lib/common/render.py:60-84 query_color; call site
// apps/infer.py:531 on the cleaned marching-cubes mesh: ~275 k vertices, ~551 k faces at mcube_res 512).
//
//   vis    = get_visibility(xy, z, faces[:, [0, 2, 1]])                     (corners swapped, z as it is)
//   colour = ((grid_sample(image, (x, -y)) + 1) * 0.5) * 255                where vis == 1
//          = ((n + 1) * 0.5) * 255, n = S1 vertex normal of `faces`         where vis == 0
//
// The visibility rule is icon_visibility's (vis_kernels.hip): the same float32 expressions in the same order (this file is
// compiled with -ffp-contract=off), the same (depth bits, face id) key under atomicMin - the z-buffer does not depend on the
// order the faces arrive in, so the visible set is the checker's exactly.  What differs is the shape of the work:
//   * one call, stream-ordered: every buffer lives in the caller's scratch (icon_query_color_bytes); nothing is allocated,
//     nothing is read back, the stream is never waited for;
//   * faces are int32 or int64 (a template parameter): no conversion copy of icon_clean_mesh's or icon_mc_emit's output;
//   * marching-cubes triangles cover ~50 pixel centres of their bounding box, not the hundreds an SMPL triangle does: a group of
//     kQcLanes lanes sweeps a face (8 faces per wavefront) instead of a whole wavefront; a face whose box holds more than
//     kQcBigPx pixels is appended to a list that a fixed-size grid of workgroups consumes from device memory;
//   * the winners are marked per horizontal run of equal pixels, not per pixel.
// The normals (incident faces in ascending face id, then corner; v / max(|v|, 1e-6)) are computed only where
// vis == 0, by the count / scan / fill / ordered-add kernels of s1_normals_device.h (shared with render_normal.hip; S1Ctx::vis
// selects the hidden vertices).  This file keeps the per-vertex kernel - the sampled colour, or the normal colour of a short
// incidence list - and the functor that stores a long list's normal as a colour.
#pragma clang fp contract(off)

#include "s1_normals_device.h"

namespace icon {

int g_qc_lanes = 0;       // icon_debug_set_option("qc_lanes"): 0 = kQcLanes; 64 = one wavefront per face, icon_visibility's mapping (the timing tool's comparison)

namespace {

constexpr int kQcLanes = 8;          // lanes that sweep one face's bounding box: 8 / 16 / 64 measured 57 / 69 / 145 us on the 513^3 mesh
constexpr int kQcBigPx = 4096;       // bounding boxes above this many pixels: the deferred list
constexpr int kQcBigGrid = 1024;     // workgroups (256 lanes, one face at a time each) consuming the deferred faces

struct QcHdr { int bad_faces, n_big, n_long, pad; };

struct QcCtx : S1Ctx {               // the mesh and the normals' scratch (vis set: only the hidden vertices get a normal), and
    const float *image;
    int S, H, W;
    float *colors, *vis_out;
    QcHdr *hdr;
    float *vis_w;                    // [V] the array behind vis, as the resolve pass writes it
    int *big;                        // deferred faces [F]
    unsigned long long *zb;          // [(S/2)^2]
};

__device__ __forceinline__ float qc_ef(float px, float py, float ax, float ay, float bx, float by)
{
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}
__device__ __forceinline__ float qc_max(float a, float b) { return (a > b) ? a : b; }
__device__ __forceinline__ float qc_min(float a, float b) { return (b < a) ? b : a; }

// face f as get_visibility(xy, z, faces[:, [0,2,1]]) sees it: screen corners, pixel box.  false: nothing to rasterise
struct QcRast {
    float X[3], Y[3], Z[3];
    float xmin, xmax, ymin, ymax, den;
    int i0, j0, w, n;
};
template <class IT>
__device__ __forceinline__ bool qc_setup(const QcCtx &c, int64_t f, QcRast &r)
{
    int64_t id[3];
    if (!s1_face<IT>(c, f, id)) return false;
    const int64_t v[3] = { id[0], id[2], id[1] };
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.X[k] = (c.verts[3 * v[k]] + 1.0f) / 2.0f; r.Y[k] = (c.verts[3 * v[k] + 1] + 1.0f) / 2.0f; r.Z[k] = (-c.verts[3 * v[k] + 2] + 1.0f) / 2.0f;
    }
    const float eps = 1e-8f;
    const float area = qc_ef(r.X[2], r.Y[2], r.X[0], r.Y[0], r.X[1], r.Y[1]);
    if (area < 0.0f || fabsf(area) <= eps) return false;                 // back face / degenerate
    r.xmin = qc_min(r.X[0], qc_min(r.X[1], r.X[2])); r.xmax = qc_max(r.X[0], qc_max(r.X[1], r.X[2]));
    r.ymin = qc_min(r.Y[0], qc_min(r.Y[1], r.Y[2])); r.ymax = qc_max(r.Y[0], qc_max(r.Y[1], r.Y[2]));
    const int S = c.S, H = S / 2;
    int i0 = (int)floorf((r.xmin + 1.0f) * 0.5f * (float)S) - 1, i1 = (int)ceilf((r.xmax + 1.0f) * 0.5f * (float)S) + 1;
    int j0 = (int)floorf((r.ymin + 1.0f) * 0.5f * (float)S) - 1, j1 = (int)ceilf((r.ymax + 1.0f) * 0.5f * (float)S) + 1;
    i0 = max(i0, H); j0 = max(j0, H); i1 = min(i1, S - 1); j1 = min(j1, S - 1);
    if (i0 > i1 || j0 > j1) return false;
    r.i0 = i0; r.j0 = j0; r.w = i1 - i0 + 1; r.n = r.w * (j1 - j0 + 1);   // <= (S/2)^2 <= 2^26
    r.den = area + eps;
    return true;
}

// pixel (i, j) of face f: icon_visibility's per-pixel rule, expression for expression.  i, j in [S/2, S)
__device__ __forceinline__ void qc_pixel(const QcCtx &c, const QcRast &r, int64_t f, int i, int j)
{
    const int S = c.S, H = S / 2;
    const float eps = 1e-8f;
    const float px = -1.0f + (float)(2 * i + 1) / (float)S, py = -1.0f + (float)(2 * j + 1) / (float)S;
    if (px < r.xmin || px > r.xmax || py < r.ymin || py > r.ymax) return;
    const float w0 = qc_ef(px, py, r.X[1], r.Y[1], r.X[2], r.Y[2]) / r.den;
    const float w1 = qc_ef(px, py, r.X[2], r.Y[2], r.X[0], r.Y[0]) / r.den;
    const float w2 = qc_ef(px, py, r.X[0], r.Y[0], r.X[1], r.Y[1]) / r.den;
    const float t0 = w0 * r.Z[1] * r.Z[2], t1 = r.Z[0] * w1 * r.Z[2], t2 = r.Z[0] * r.Z[1] * w2;
    const float dn = qc_max(t0 + t1 + t2, eps);
    const float b0 = t0 / dn, b1 = t1 / dn, b2 = t2 / dn;
    const float pz = b0 * r.Z[0] + b1 * r.Z[1] + b2 * r.Z[2];
    if (pz < 0.0f) return;
    if (!(b0 > 0.0f && b1 > 0.0f && b2 > 0.0f)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(pz) << 32) | (unsigned long long)(uint32_t)f;
    atomicMin(&c.zb[(size_t)(j - H) * H + (i - H)], key);
}

// G lanes per face, 256 / G faces per workgroup
template <class IT, int G>
__global__ __launch_bounds__(256) void k_qc_raster(QcCtx c)
{
    const int64_t f = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x % G;
    if (f >= c.F) return;
    QcRast r;
    if (!qc_setup<IT>(c, f, r)) return;
    if (G < 64 && r.n > kQcBigPx) {
        if (sub == 0) c.big[atomicAdd(&c.hdr->n_big, 1)] = (int)f;        // at most F entries
        return;
    }
    int j = sub / r.w, i = sub - j * r.w;
    for (int t = sub; t < r.n; t += G) {
        qc_pixel(c, r, f, r.i0 + i, r.j0 + j);
        i += G;
        while (i >= r.w) { i -= r.w; ++j; }
    }
}

// the deferred faces: a workgroup per face, as many rounds as the list (read from device memory) needs
template <class IT>
__global__ __launch_bounds__(256) void k_qc_raster_big(QcCtx c)
{
    const int nb = c.hdr->n_big;
    for (int b = blockIdx.x; b < nb; b += gridDim.x) {
        const int64_t f = c.big[b];
        QcRast r;
        if (!qc_setup<IT>(c, f, r)) continue;
        for (int t = threadIdx.x; t < r.n; t += 256) {
            const int j = t / r.w;
            qc_pixel(c, r, f, r.i0 + (t - j * r.w), r.j0 + j);
        }
    }
}

// vis[corners of every face that owns a pixel] = 1, one marking per horizontal run of a face inside a wavefront's 64 pixels;
// faces[-1] always (the background index, as in the reference)
template <class IT>
__global__ __launch_bounds__(256) void k_qc_resolve(QcCtx c, int64_t npx)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p == 0) {
        int64_t v[3];
        if (s1_face<IT>(c, c.F - 1, v)) { c.vis_w[v[0]] = 1.0f; c.vis_w[v[1]] = 1.0f; c.vis_w[v[2]] = 1.0f; }
    }
    const unsigned long long key = p < npx ? c.zb[p] : ~0ull;
    const int f = key == ~0ull ? -1 : (int)(uint32_t)(key & 0xffffffffull);
    const int left = __shfl_up(f, 1);
    if (f < 0 || ((threadIdx.x & 63) != 0 && left == f)) return;
    int64_t v[3];
    s1_face<IT>(c, f, v);                                                 // a face in the z-buffer passed qc_setup's index check
    c.vis_w[v[0]] = 1.0f; c.vis_w[v[1]] = 1.0f; c.vis_w[v[2]] = 1.0f;
}

// a normal as a colour: ((n + 1) * 0.5) * 255, n = s / max(|s|, 1e-6)
struct QcStore {
    float *colors;
    __device__ void operator()(int64_t v, float x, float y, float z) const
    {
        s1_normalise(x, y, z);
        colors[3 * v] = (x + 1.0f) * 0.5f * 255.0f;
        colors[3 * v + 1] = (y + 1.0f) * 0.5f * 255.0f;
        colors[3 * v + 2] = (z + 1.0f) * 0.5f * 255.0f;
    }
};

// one thread per vertex: the sampled colour, or the normal colour of a short incidence list
template <class IT>
__global__ __launch_bounds__(256) void k_qc_shade(QcCtx c)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= c.V) return;
    const float visible = c.vis[v];
    if (c.vis_out) c.vis_out[v] = visible;
    if (visible != 0.0f) {
        const BilinearTaps t = bilinear_taps(c.verts[3 * v], -c.verts[3 * v + 1], c.H, c.W);     // uv = xy * (1, -1)
        const int x1 = t.x0 + 1, y1 = t.y0 + 1;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float *pl = c.image + (size_t)ch * c.H * c.W;
            const float t00 = (t.bx0 && t.by0) ? pl[(size_t)t.y0 * c.W + t.x0] : 0.0f;
            const float t01 = (t.bx1 && t.by0) ? pl[(size_t)t.y0 * c.W + x1] : 0.0f;
            const float t10 = (t.bx0 && t.by1) ? pl[(size_t)y1 * c.W + t.x0] : 0.0f;
            const float t11 = (t.bx1 && t.by1) ? pl[(size_t)y1 * c.W + x1] : 0.0f;
            float acc = t00 * t.nw; acc += t01 * t.ne; acc += t10 * t.sw; acc += t11 * t.se;
            c.colors[3 * v + ch] = (acc + 1.0f) * 0.5f * 255.0f;
        }
        return;
    }
    const int n = c.deg[v];
    if (n > kShort) { s1_defer_long(c, v); return; }
    float s[3];
    s1_sum_short<IT>(c, v, n, s);
    QcStore{c.colors}(v, s[0], s[1], s[2]);
}

struct QcLayout { size_t hdr, deg, cur, vis, zero_end, loc, part, inc, tmp, big, longv, zb, total; };

QcLayout qc_layout(int64_t V, int64_t F, int S)
{
    QcLayout L{};
    ScratchTake take;
    L.hdr = take(sizeof(QcHdr)); L.deg = take((size_t)V * 4); L.cur = take((size_t)V * 4); L.vis = take((size_t)V * 4);
    L.zero_end = take.o;                                                   // [0, zero_end): cleared by one memset per call
    L.loc = take((size_t)V * 4); L.part = take((size_t)((V + kScanItems - 1) / kScanItems) * 4);
    L.inc = take((size_t)F * 12); L.tmp = take((size_t)F * 12);
    L.big = take((size_t)F * 4); L.longv = take((size_t)V * 4);
    L.zb = take((size_t)(S / 2) * (S / 2) * 8);
    L.total = take.o;
    return L;
}

int qc_check_sizes(int64_t V, int64_t F, int image_size)
{
    ICON_ARG(V > 0 && F > 0 && V < (1ll << 31) && F < (1ll << 29), "icon_query_color: 0 < V < 2^31, 0 < F < 2^29");
    ICON_ARG(image_size >= 2 && image_size <= 16384 && (image_size & 1) == 0, "icon_query_color: image_size must be even, 2..16384");
    return ICON_OK;
}

template <class IT>
void qc_launch(const QcCtx &c, hipStream_t st)
{
    const int64_t npx = (int64_t)(c.S / 2) * (c.S / 2);
    const unsigned gF = (unsigned)((c.F + 255) / 256), gV = (unsigned)((c.V + 255) / 256);
    const int nb = (int)((c.V + kScanItems - 1) / kScanItems);
    const int G = g_qc_lanes == 64 ? 64 : kQcLanes;
    const unsigned gR = (unsigned)((c.F * G + 255) / 256);
    if (G == 64) hipLaunchKernelGGL((k_qc_raster<IT, 64>), dim3(gR), dim3(256), 0, st, c);
    else hipLaunchKernelGGL((k_qc_raster<IT, kQcLanes>), dim3(gR), dim3(256), 0, st, c);
    if (G != 64) hipLaunchKernelGGL(k_qc_raster_big<IT>, dim3(kQcBigGrid), dim3(256), 0, st, c);
    hipLaunchKernelGGL(k_qc_resolve<IT>, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, st, c, npx);
    const S1Ctx &s1 = c;                                                   // the shared kernels take the base alone
    hipLaunchKernelGGL(k_s1_count<IT>, dim3(gF), dim3(256), 0, st, s1);
    hipLaunchKernelGGL(k_s1_scan_blocks, dim3((unsigned)nb), dim3(256), 0, st, s1);
    hipLaunchKernelGGL(k_s1_scan_parts, dim3(1), dim3(1024), 0, st, s1, nb);
    hipLaunchKernelGGL(k_s1_fill<IT>, dim3(gF), dim3(256), 0, st, s1);
    hipLaunchKernelGGL(k_qc_shade<IT>, dim3(gV), dim3(256), 0, st, c);
    hipLaunchKernelGGL((k_s1_normals_long<IT, QcStore>), dim3(kLongGrid), dim3(64), 0, st, s1, QcStore{c.colors});
}

}  // namespace
}  // namespace icon

using namespace icon;

extern "C" int icon_query_color_bytes(int64_t V, int64_t F, int image_size, int64_t *bytes)
{
    ICON_ARG(bytes != nullptr, "icon_query_color_bytes: null argument");
    const int rc = qc_check_sizes(V, F, image_size);
    if (rc) return rc;
    *bytes = (int64_t)qc_layout(V, F, image_size).total;
    return ICON_OK;
}

extern "C" int icon_query_color(const float *d_verts, int64_t V, const void *d_faces, int64_t F, int faces_int64,
                                const float *d_image, int H, int W, int image_size, float *d_colors, float *d_vis,
                                void *d_scratch, int64_t scratch_bytes, void *stream)
{
    ICON_ARG(d_verts && d_faces && d_image && d_colors && d_scratch, "icon_query_color: null argument");
    const int rc = qc_check_sizes(V, F, image_size);
    if (rc) return rc;
    ICON_ARG(H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "icon_query_color: bad image size");
    const QcLayout L = qc_layout(V, F, image_size);
    if (const int e = scratch_check("icon_query_color", "icon_query_color_bytes", d_scratch, scratch_bytes, L.total)) return e;
    hipStream_t st = (hipStream_t)stream;
    char *s = static_cast<char *>(d_scratch);
    QcCtx c{};
    c.verts = d_verts; c.faces = d_faces; c.image = d_image; c.V = V; c.F = F; c.S = image_size; c.H = H; c.W = W;
    c.colors = d_colors; c.vis_out = d_vis;
    c.hdr = reinterpret_cast<QcHdr *>(s + L.hdr); c.bad_faces = &c.hdr->bad_faces; c.n_long = &c.hdr->n_long;
    c.deg = reinterpret_cast<int *>(s + L.deg); c.cur = reinterpret_cast<int *>(s + L.cur);
    c.vis_w = reinterpret_cast<float *>(s + L.vis); c.vis = c.vis_w; c.loc = reinterpret_cast<int *>(s + L.loc); c.part = reinterpret_cast<int *>(s + L.part);
    c.inc = reinterpret_cast<int *>(s + L.inc); c.tmp = reinterpret_cast<int *>(s + L.tmp); c.big = reinterpret_cast<int *>(s + L.big);
    c.longv = reinterpret_cast<int *>(s + L.longv); c.zb = reinterpret_cast<unsigned long long *>(s + L.zb);
    ICON_HIP(hipMemsetAsync(s, 0, L.zero_end, st));
    ICON_HIP(hipMemsetAsync(c.zb, 0xff, L.total - L.zb, st));
    if (faces_int64) qc_launch<int64_t>(c, st); else qc_launch<int32_t>(c, st);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

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
// vis == 0: count / scan / fill a vertex -> (3 face + corner) incidence list for those vertices, then one thread per vertex
// takes the entries in ascending order (selection: the lists hold ~6 entries); a vertex of more than kQcShort entries goes
// to a second device-side list, where one wavefront rank-sorts its entries and adds them in order.  The order of the
// additions is fixed by the keys alone: bit-identical from run to run and to the checker's sequential loop.
#pragma clang fp contract(off)

#include "common.h"

namespace icon {

int g_qc_lanes = 0;       // icon_debug_set_option("qc_lanes"): 0 = kQcLanes; 64 = one wavefront per face, icon_visibility's mapping (the timing tool's comparison)

namespace {

constexpr int kQcLanes = 8;          // lanes that sweep one face's bounding box: 8 / 16 / 64 measured 57 / 69 / 145 us on the 513^3 mesh
constexpr int kQcBigPx = 4096;       // bounding boxes above this many pixels: the deferred list
constexpr int kQcBigGrid = 1024;     // workgroups (256 lanes, one face at a time each) consuming the deferred faces
constexpr int kQcShort = 32;         // incidence lists up to this length are summed by one thread
constexpr int kQcLongGrid = 256;     // wavefronts consuming the long lists
constexpr int kQcScanItems = 1024;   // vertices per block of the scan (256 threads x 4)

struct QcHdr { int bad_faces, n_big, n_long, pad; };

struct QcCtx {
    const float *verts; const void *faces; const float *image;
    int64_t V, F;
    int S, H, W;
    float *colors, *vis_out;
    QcHdr *hdr;
    int *deg, *cur;                  // [V] incidence count / fill cursor of the non-visible vertices
    float *vis;                      // [V]
    int *loc, *part;                 // scan: exclusive prefix inside each kQcScanItems block, exclusive prefix of the block totals
    int *inc, *tmp;                  // [3F] incidence keys 3 f + corner, grouped by vertex; tmp: the long lists, sorted
    int *big, *longv;                // deferred faces [F], long-list vertices [V]
    unsigned long long *zb;          // [(S/2)^2]
};

__device__ __forceinline__ float qc_ef(float px, float py, float ax, float ay, float bx, float by)
{
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}
__device__ __forceinline__ float qc_max(float a, float b) { return (a > b) ? a : b; }
__device__ __forceinline__ float qc_min(float a, float b) { return (b < a) ? b : a; }

// the three vertex ids of face f; false: the face names a vertex that does not exist (it is skipped everywhere)
template <class IT>
__device__ __forceinline__ bool qc_face(const QcCtx &c, int64_t f, int64_t v[3])
{
    const IT *fp = static_cast<const IT *>(c.faces) + 3 * f;
    v[0] = (int64_t)fp[0]; v[1] = (int64_t)fp[1]; v[2] = (int64_t)fp[2];
    return v[0] >= 0 && v[0] < c.V && v[1] >= 0 && v[1] < c.V && v[2] >= 0 && v[2] < c.V;
}

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
    if (!qc_face<IT>(c, f, id)) return false;
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
        if (qc_face<IT>(c, c.F - 1, v)) { c.vis[v[0]] = 1.0f; c.vis[v[1]] = 1.0f; c.vis[v[2]] = 1.0f; }
    }
    const unsigned long long key = p < npx ? c.zb[p] : ~0ull;
    const int f = key == ~0ull ? -1 : (int)(uint32_t)(key & 0xffffffffull);
    const int left = __shfl_up(f, 1);
    if (f < 0 || ((threadIdx.x & 63) != 0 && left == f)) return;
    int64_t v[3];
    qc_face<IT>(c, f, v);                                                 // a face in the z-buffer passed qc_setup's index check
    c.vis[v[0]] = 1.0f; c.vis[v[1]] = 1.0f; c.vis[v[2]] = 1.0f;
}

// incidence count of the vertices that need a normal; faces that name a missing vertex are counted in the header
template <class IT>
__global__ __launch_bounds__(256) void k_qc_count(QcCtx c)
{
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= c.F) return;
    int64_t v[3];
    if (!qc_face<IT>(c, f, v)) { atomicAdd(&c.hdr->bad_faces, 1); return; }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (c.vis[v[k]] == 0.0f) atomicAdd(&c.deg[v[k]], 1);
}

__device__ __forceinline__ int qc_wave_incl_scan(int v)
{
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d); if (lane >= d) v += o; }
    return v;
}
// exclusive prefix of v over the workgroup (NW wavefronts); total: the workgroup's sum
template <int NW>
__device__ __forceinline__ int qc_block_excl_scan(int v, int *s_w, int &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int incl = qc_wave_incl_scan(v);
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    int before = 0, all = 0;
    for (int q = 0; q < NW; ++q) { const int t = s_w[q]; before += q < w ? t : 0; all += t; }
    __syncthreads();
    total = all;
    return before + incl - v;
}

__global__ __launch_bounds__(256) void k_qc_scan_blocks(QcCtx c)
{
    __shared__ int s_w[4];
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    int d[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { d[k] = i0 + k < c.V ? c.deg[i0 + k] : 0; sum += d[k]; }
    int total;
    int run = qc_block_excl_scan<4>(sum, s_w, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (i0 + k < c.V) c.loc[i0 + k] = run; run += d[k]; }
    if (threadIdx.x == 0) c.part[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void k_qc_scan_parts(QcCtx c, int nb)
{
    __shared__ int s_w[16];
    int carry = 0;
    for (int base = 0; base < nb; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < nb ? c.part[i] : 0;
        int total;
        const int ex = qc_block_excl_scan<16>(v, s_w, total);
        if (i < nb) c.part[i] = carry + ex;
        carry += total;
    }
}

__device__ __forceinline__ int qc_start(const QcCtx &c, int64_t v) { return c.loc[v] + c.part[v / kQcScanItems]; }

template <class IT>
__global__ __launch_bounds__(256) void k_qc_fill(QcCtx c)
{
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= c.F) return;
    int64_t v[3];
    if (!qc_face<IT>(c, f, v)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (c.vis[v[k]] == 0.0f) c.inc[qc_start(c, v[k]) + atomicAdd(&c.cur[v[k]], 1)] = (int)(3 * f + k);
}

// (v1 - v0) x (v2 - v0) of the face behind an incidence key (S1; the un-swapped corner order)
template <class IT>
__device__ __forceinline__ void qc_face_normal(const QcCtx &c, int key, float n[3])
{
    int64_t v[3];
    qc_face<IT>(c, key / 3, v);                                           // listed faces passed the index check
    const float *a = c.verts + 3 * v[0], *b = c.verts + 3 * v[1], *d = c.verts + 3 * v[2];
    const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const float vx = d[0] - a[0], vy = d[1] - a[1], vz = d[2] - a[2];
    n[0] = fmaf(uy, vz, -(uz * vy)); n[1] = fmaf(uz, vx, -(ux * vz)); n[2] = fmaf(ux, vy, -(uy * vx));
}

__device__ __forceinline__ void qc_store_normal_colour(const QcCtx &c, int64_t v, float x, float y, float z)
{
    float len = sqrtf(fmaf(z, z, fmaf(y, y, x * x)));
    if (len < 1e-6f) len = 1e-6f;
    c.colors[3 * v] = (x / len + 1.0f) * 0.5f * 255.0f;
    c.colors[3 * v + 1] = (y / len + 1.0f) * 0.5f * 255.0f;
    c.colors[3 * v + 2] = (z / len + 1.0f) * 0.5f * 255.0f;
}

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
    if (n > kQcShort) { c.longv[atomicAdd(&c.hdr->n_long, 1)] = (int)v; return; }   // at most V entries
    const int *list = c.inc + qc_start(c, v);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    int last = -1;
    for (int step = 0; step < n; ++step) {                                 // the next larger key: ascending face id, then corner
        int best = 0x7fffffff;
        for (int q = 0; q < n; ++q) { const int k = list[q]; if (k > last && k < best) best = k; }
        float fn[3];
        qc_face_normal<IT>(c, best, fn);
        sx += fn[0]; sy += fn[1]; sz += fn[2];
        last = best;
    }
    qc_store_normal_colour(c, v, sx, sy, sz);
}

// the long lists: one wavefront per vertex - rank-sort the keys into tmp, then add the face normals in that order
template <class IT>
__global__ __launch_bounds__(64) void k_qc_normals_long(QcCtx c)
{
    const int nl = c.hdr->n_long;
    const int lane = threadIdx.x;
    for (int b = blockIdx.x; b < nl; b += gridDim.x) {
        const int64_t v = c.longv[b];
        const int n = c.deg[v], st = qc_start(c, v);
        const int *list = c.inc + st;
        for (int i = lane; i < n; i += 64) {
            const int key = list[i];
            int rank = 0;
            for (int q = 0; q < n; ++q) rank += list[q] < key ? 1 : 0;     // keys are distinct
            c.tmp[st + rank] = key;
        }
        __threadfence();                                                   // the wave's own stores, read back by other lanes below
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            float fn[3] = { 0.0f, 0.0f, 0.0f };
            if (i < n) qc_face_normal<IT>(c, __hip_atomic_load(&c.tmp[st + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), fn);   // (not through a stale L1 line)
            const int cnt = min(64, n - base);
            for (int l = 0; l < cnt; ++l) { sx += __shfl(fn[0], l); sy += __shfl(fn[1], l); sz += __shfl(fn[2], l); }
        }
        if (lane == 0) qc_store_normal_colour(c, v, sx, sy, sz);
    }
}

struct QcLayout { size_t hdr, deg, cur, vis, zero_end, loc, part, inc, tmp, big, longv, zb, total; };

QcLayout qc_layout(int64_t V, int64_t F, int S)
{
    QcLayout L{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = (o + bytes + 255) / 256 * 256; return at; };
    L.hdr = take(sizeof(QcHdr)); L.deg = take((size_t)V * 4); L.cur = take((size_t)V * 4); L.vis = take((size_t)V * 4);
    L.zero_end = o;                                                        // [0, zero_end): cleared by one memset per call
    L.loc = take((size_t)V * 4); L.part = take((size_t)((V + kQcScanItems - 1) / kQcScanItems) * 4);
    L.inc = take((size_t)F * 12); L.tmp = take((size_t)F * 12);
    L.big = take((size_t)F * 4); L.longv = take((size_t)V * 4);
    L.zb = take((size_t)(S / 2) * (S / 2) * 8);
    L.total = o;
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
    const int nb = (int)((c.V + kQcScanItems - 1) / kQcScanItems);
    const int G = g_qc_lanes == 64 ? 64 : kQcLanes;
    const unsigned gR = (unsigned)((c.F * G + 255) / 256);
    if (G == 64) hipLaunchKernelGGL((k_qc_raster<IT, 64>), dim3(gR), dim3(256), 0, st, c);
    else hipLaunchKernelGGL((k_qc_raster<IT, kQcLanes>), dim3(gR), dim3(256), 0, st, c);
    if (G != 64) hipLaunchKernelGGL(k_qc_raster_big<IT>, dim3(kQcBigGrid), dim3(256), 0, st, c);
    hipLaunchKernelGGL(k_qc_resolve<IT>, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, st, c, npx);
    hipLaunchKernelGGL(k_qc_count<IT>, dim3(gF), dim3(256), 0, st, c);
    hipLaunchKernelGGL(k_qc_scan_blocks, dim3((unsigned)nb), dim3(256), 0, st, c);
    hipLaunchKernelGGL(k_qc_scan_parts, dim3(1), dim3(1024), 0, st, c, nb);
    hipLaunchKernelGGL(k_qc_fill<IT>, dim3(gF), dim3(256), 0, st, c);
    hipLaunchKernelGGL(k_qc_shade<IT>, dim3(gV), dim3(256), 0, st, c);
    hipLaunchKernelGGL(k_qc_normals_long<IT>, dim3(kQcLongGrid), dim3(64), 0, st, c);
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
    ICON_ARG(((uintptr_t)d_scratch & 255) == 0, "icon_query_color: the scratch must be 256-byte aligned");
    const QcLayout L = qc_layout(V, F, image_size);
    ICON_ARG(scratch_bytes >= (int64_t)L.total, "icon_query_color: scratch smaller than icon_query_color_bytes");
    hipStream_t st = (hipStream_t)stream;
    char *s = static_cast<char *>(d_scratch);
    QcCtx c{};
    c.verts = d_verts; c.faces = d_faces; c.image = d_image; c.V = V; c.F = F; c.S = image_size; c.H = H; c.W = W;
    c.colors = d_colors; c.vis_out = d_vis;
    c.hdr = reinterpret_cast<QcHdr *>(s + L.hdr); c.deg = reinterpret_cast<int *>(s + L.deg); c.cur = reinterpret_cast<int *>(s + L.cur);
    c.vis = reinterpret_cast<float *>(s + L.vis); c.loc = reinterpret_cast<int *>(s + L.loc); c.part = reinterpret_cast<int *>(s + L.part);
    c.inc = reinterpret_cast<int *>(s + L.inc); c.tmp = reinterpret_cast<int *>(s + L.tmp); c.big = reinterpret_cast<int *>(s + L.big);
    c.longv = reinterpret_cast<int *>(s + L.longv); c.zb = reinterpret_cast<unsigned long long *>(s + L.zb);
    ICON_HIP(hipMemsetAsync(s, 0, L.zero_end, st));
    ICON_HIP(hipMemsetAsync(c.zb, 0xff, L.total - L.zb, st));
    if (faces_int64) qc_launch<int64_t>(c, st); else qc_launch<int32_t>(c, st);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

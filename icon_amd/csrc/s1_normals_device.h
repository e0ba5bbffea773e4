// s1_normals_device.h - the S1 vertex normals (incident faces in ascending 3 face + corner order, float32,
// v / max(|v|, 1e-6)) as query_color.hip, render_normal.hip and render_normal_bwd.hip compute them, stated once: count / scan / fill a
// vertex -> (3 face + corner) incidence list, then one thread per vertex takes the entries in ascending order (selection: the lists
// hold ~6 entries); a vertex of more than kShort entries goes to a device-side list, where one wavefront rank-sorts its entries
// and adds them in order.  The order of the additions is fixed by the keys alone: bit-identical from run to run and to the
// checkers' sequential loops.  Everything lives in the including file's anonymous namespace: each file instantiates the kernels
// with its own context (S1Ctx is the base of QcCtx and, through raster_device.h's RsCtx, of RnCtx / SilCtx / RnbCtx), its own per-vertex
// kernel (s1_sum_short, s1_defer_long) and its own Store functor (k_s1_normals_long); the host side lays the pieces out in the caller's
// scratch (s1_layout), binds them (s1_bind) and launches count / scan / fill (s1_launch_lists).  Every index taken out of the scratch
// (list lengths, segment starts, keys, list entries) is range-checked before it is used as an address: the checks always pass after the
// call's own clears and are never relied on - a call replayed from a captured graph once met the previous call's counters.
#pragma once
#pragma clang fp contract(off)

#include "scan_device.h"

namespace icon {
namespace {

constexpr int kShort = 32;           // incidence lists up to this length are summed by one thread
constexpr int kLongGrid = 256;       // wavefronts consuming the long lists
constexpr int kScanItems = 1024;     // vertices per block of the scan (256 threads x 4)

struct S1Ctx {
    const float *verts; const void *faces;
    int64_t V, F;
    int *bad_faces, *n_long;         // words of the caller's header: faces that name a missing vertex, length of longv
    int *deg, *cur;                  // [V] incidence count / fill cursor (both 0 when k_s1_count starts)
    int *loc, *part;                 // scan: exclusive prefix inside each kScanItems block, exclusive prefix of the block totals
    int *inc, *tmp;                  // [3F] incidence keys 3 f + corner, grouped by vertex; tmp: the long lists, sorted
    int *longv;                      // [V] the vertices of more than kShort entries
    const float *vis;                // null: every vertex gets a normal; otherwise only those with vis[v] == 0
};

// the first words of a call's scratch: the counters its kernels raise (0 after the call's clear).  n_big: the length of the caller's
// list of deferred faces, where it keeps one (raster_device.h)
struct S1Hdr { int bad_faces, n_big, n_long, pad; };

// ---- host: the S1 pieces of a call's scratch, 256-byte aligned; [0, zero_end) is what the call's clear sets to 0 ----
struct S1Layout { size_t hdr, deg, cur, zero_end, loc, part, inc, tmp, mid, longv; };

// appends the pieces to `take`; mid: `mid_bytes` of the caller's own between tmp and longv (render_normal.hip's deferred list lives there)
S1Layout s1_layout(ScratchTake &take, int64_t V, int64_t F, size_t mid_bytes = 0)
{
    S1Layout L{};
    L.hdr = take(sizeof(S1Hdr)); L.deg = take((size_t)V * 4); L.cur = take((size_t)V * 4);
    L.zero_end = take.o;
    L.loc = take((size_t)V * 4); L.part = take((size_t)((V + kScanItems - 1) / kScanItems) * 4);
    L.inc = take((size_t)F * 12); L.tmp = take((size_t)F * 12);
    L.mid = take(mid_bytes); L.longv = take((size_t)V * 4);
    return L;
}

// binds the pieces over the scratch `s` into the context; the header, for the caller's own counters
S1Hdr *s1_bind(S1Ctx &c, char *s, const S1Layout &L)
{
    S1Hdr *hdr = reinterpret_cast<S1Hdr *>(s + L.hdr);
    c.bad_faces = &hdr->bad_faces; c.n_long = &hdr->n_long;
    c.deg = reinterpret_cast<int *>(s + L.deg); c.cur = reinterpret_cast<int *>(s + L.cur);
    c.loc = reinterpret_cast<int *>(s + L.loc); c.part = reinterpret_cast<int *>(s + L.part);
    c.inc = reinterpret_cast<int *>(s + L.inc); c.tmp = reinterpret_cast<int *>(s + L.tmp);
    c.longv = reinterpret_cast<int *>(s + L.longv);
    return hdr;
}

// the three vertex ids of face f; false: the face names a vertex that does not exist (it is skipped everywhere)
template <class IT>
__device__ __forceinline__ bool s1_face(const S1Ctx &c, int64_t f, int64_t v[3])
{
    const IT *fp = static_cast<const IT *>(c.faces) + 3 * f;
    v[0] = (int64_t)fp[0]; v[1] = (int64_t)fp[1]; v[2] = (int64_t)fp[2];
    return v[0] >= 0 && v[0] < c.V && v[1] >= 0 && v[1] < c.V && v[2] >= 0 && v[2] < c.V;
}

__device__ __forceinline__ bool s1_wanted(const S1Ctx &c, int64_t v) { return !c.vis || c.vis[v] == 0.0f; }

// incidence count of the vertices that need a normal; faces that name a missing vertex are counted in the header
template <class IT>
__global__ __launch_bounds__(256) void k_s1_count(S1Ctx c)
{
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= c.F) return;
    int64_t v[3];
    if (!s1_face<IT>(c, f, v)) { atomicAdd(c.bad_faces, 1); return; }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (s1_wanted(c, v[k])) atomicAdd(&c.deg[v[k]], 1);
}

__global__ __launch_bounds__(256) void k_s1_scan_blocks(S1Ctx c)
{
    __shared__ int s_w[4];
    const int total = block_scan_tile<4, 4>(c.deg, c.loc, ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4, c.V, 0, s_w);
    if (threadIdx.x == 0) c.part[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void k_s1_scan_parts(S1Ctx c, int nb)
{
    __shared__ int s_w[16];
    int carry = 0;
    for (int base = 0; base < nb; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < nb ? c.part[i] : 0;
        int total;
        __syncthreads();                                        // (the previous round's s_w has been read)
        const int ex = block_excl_scan<16>(v, s_w, total);
        if (i < nb) c.part[i] = carry + ex;
        carry += total;
    }
}

// where vertex v's segment of inc / tmp starts
__device__ __forceinline__ int s1_start(const S1Ctx &c, int64_t v) { return c.loc[v] + c.part[v / kScanItems]; }

// per face: the key 3 face + corner into each wanted vertex's segment (cursor by atomicAdd: the order inside a segment is arbitrary)
template <class IT>
__global__ __launch_bounds__(256) void k_s1_fill(S1Ctx c)
{
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= c.F) return;
    int64_t v[3];
    if (!s1_face<IT>(c, f, v)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!s1_wanted(c, v[k])) continue;
        const int64_t at = (int64_t)s1_start(c, v[k]) + atomicAdd(&c.cur[v[k]], 1);
        if (at >= 0 && at < 3 * c.F) c.inc[at] = (int)(3 * f + k);
    }
}

// host: count / scan / fill on stream st - the incidence lists every per-vertex kernel below reads
template <class IT>
void s1_launch_lists(const S1Ctx &c, hipStream_t st)
{
    const unsigned gF = (unsigned)((c.F + 255) / 256);
    const int nb = (int)((c.V + kScanItems - 1) / kScanItems);
    hipLaunchKernelGGL(k_s1_count<IT>, dim3(gF), dim3(256), 0, st, c);
    hipLaunchKernelGGL(k_s1_scan_blocks, dim3((unsigned)nb), dim3(256), 0, st, c);
    hipLaunchKernelGGL(k_s1_scan_parts, dim3(1), dim3(1024), 0, st, c, nb);
    hipLaunchKernelGGL(k_s1_fill<IT>, dim3(gF), dim3(256), 0, st, c);
}

// (v1 - v0) x (v2 - v0) of the face behind an incidence key (S1; the corner order as given); 0 for a key that names no face
template <class IT>
__device__ __forceinline__ void s1_face_normal(const S1Ctx &c, int key, float n[3])
{
    int64_t v[3];
    n[0] = n[1] = n[2] = 0.0f;
    if (key < 0 || key / 3 >= c.F || !s1_face<IT>(c, key / 3, v)) return;   // listed faces passed the index check
    const float *a = c.verts + 3 * v[0], *b = c.verts + 3 * v[1], *d = c.verts + 3 * v[2];
    const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const float vx = d[0] - a[0], vy = d[1] - a[1], vz = d[2] - a[2];
    n[0] = fmaf(uy, vz, -(uz * vy)); n[1] = fmaf(uz, vx, -(ux * vz)); n[2] = fmaf(ux, vy, -(uy * vx));
}

// v / max(|v|, 1e-6), in place
__device__ __forceinline__ void s1_normalise(float &x, float &y, float &z)
{
    float len = sqrtf(fmaf(z, z, fmaf(y, y, x * x)));
    if (len < 1e-6f) len = 1e-6f;
    x = x / len; y = y / len; z = z / len;
}

// the un-normalised S1 sum of vertex v's n <= kShort entries: the next larger key each step (ascending face id, then corner)
template <class IT>
__device__ __forceinline__ void s1_sum_short(const S1Ctx &c, int64_t v, int n, float s[3])
{
    s[0] = s[1] = s[2] = 0.0f;
    const int64_t st = s1_start(c, v);
    if (n < 0 || st < 0 || st + n > 3 * c.F) return;
    const int *list = c.inc + st;
    int last = -1;
    for (int step = 0; step < n; ++step) {
        int best = 0x7fffffff;
        for (int q = 0; q < n; ++q) { const int k = list[q]; if (k > last && k < best) best = k; }
        float fn[3];
        s1_face_normal<IT>(c, best, fn);
        s[0] += fn[0]; s[1] += fn[1]; s[2] += fn[2];
        last = best;
    }
}

// vertex v has more than kShort entries: k_s1_normals_long's (at most V entries)
__device__ __forceinline__ void s1_defer_long(const S1Ctx &c, int64_t v)
{
    const int at = atomicAdd(c.n_long, 1);
    if ((int64_t)at < c.V) c.longv[at] = (int)v;
}

// the long lists: one wavefront per vertex - rank-sort the keys into tmp, then add the face normals in that order.
// Store: a trivially copyable functor; lane 0 calls store(v, sx, sy, sz) with the un-normalised sum
template <class IT, class Store>
__global__ __launch_bounds__(64) void k_s1_normals_long(S1Ctx c, Store store)
{
    const int nl = (int)min((int64_t)*c.n_long, c.V);
    const int lane = threadIdx.x;
    for (int e = blockIdx.x; e < nl; e += gridDim.x) {
        const int64_t v = c.longv[e];
        if (v < 0 || v >= c.V) continue;
        const int n = c.deg[v], st = s1_start(c, v);
        if (n < 0 || st < 0 || (int64_t)st + n > 3 * c.F) continue;
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
            if (i < n) s1_face_normal<IT>(c, __hip_atomic_load(&c.tmp[st + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), fn);   // (not through a stale L1 line)
            const int cnt = min(64, n - base);
            for (int l = 0; l < cnt; ++l) { sx += __shfl(fn[0], l); sy += __shfl(fn[1], l); sz += __shfl(fn[2], l); }
        }
        if (lane == 0) store(v, sx, sy, sz);
    }
}

// ---- ordered sums of OTHER per-corner terms over the same lists (silhouette.hip: the per-corner gradients of a face) ----
// Term: a trivially copyable functor; term(pass, key, out) gives the three addends of incidence key `key` in pass `pass` (it checks
// the key's range itself).  The passes are added one after the other, each in ascending key order, into one sum.  T: the type the
// terms come in and are added in - float, or double (evaluator.hip's angle-weighted normals)
template <class Term, class T = float>
__device__ __forceinline__ void s1_sum_short_terms(const S1Ctx &c, int64_t v, int n, int passes, const Term &term, T s[3])
{
    s[0] = s[1] = s[2] = T(0);
    const int64_t st = s1_start(c, v);
    if (n < 0 || st < 0 || st + n > 3 * c.F) return;
    const int *list = c.inc + st;
    for (int p = 0; p < passes; ++p) {
        int last = -1;
        for (int step = 0; step < n; ++step) {
            int best = 0x7fffffff;
            for (int q = 0; q < n; ++q) { const int k = list[q]; if (k > last && k < best) best = k; }
            T a[3];
            term(p, best, a);
            s[0] += a[0]; s[1] += a[1]; s[2] += a[2];
            last = best;
        }
    }
}

// the long lists of such a sum: k_s1_normals_long's rank sort, then the terms of every pass in that order; lane 0 calls store(v, sx, sy, sz)
template <class Term, class Store, class T = float>
__global__ __launch_bounds__(64) void k_s1_sum_long(S1Ctx c, int passes, Term term, Store store)
{
    const int nl = (int)min((int64_t)*c.n_long, c.V);
    const int lane = threadIdx.x;
    for (int e = blockIdx.x; e < nl; e += gridDim.x) {
        const int64_t v = c.longv[e];
        if (v < 0 || v >= c.V) continue;
        const int n = c.deg[v], st = s1_start(c, v);
        if (n < 0 || st < 0 || (int64_t)st + n > 3 * c.F) continue;
        const int *list = c.inc + st;
        for (int i = lane; i < n; i += 64) {
            const int key = list[i];
            int rank = 0;
            for (int q = 0; q < n; ++q) rank += list[q] < key ? 1 : 0;     // keys are distinct
            c.tmp[st + rank] = key;
        }
        __threadfence();                                                   // the wave's own stores, read back by other lanes below
        T sx = T(0), sy = T(0), sz = T(0);
        for (int p = 0; p < passes; ++p)
            for (int base = 0; base < n; base += 64) {
                const int i = base + lane;
                T a[3] = { T(0), T(0), T(0) };
                if (i < n) term(p, __hip_atomic_load(&c.tmp[st + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), a);
                const int cnt = min(64, n - base);
                for (int l = 0; l < cnt; ++l) { sx += __shfl(a[0], l); sy += __shfl(a[1], l); sz += __shfl(a[2], l); }
            }
        if (lane == 0) store(v, sx, sy, sz);
    }
}

}  // namespace
}  // namespace icon

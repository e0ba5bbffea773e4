// garment.hip - extract_cloth (lib/common/cloth_extraction.py:45-170, called at apps/infer.py:565-605): the submesh of the
// reconstruction whose vertices lie inside the garment's 2-D segmentation polygons and are not labelled, through their nearest
// SMPL vertex, with a body part the garment type excludes - as ONE native call on the stream.  The rule is DESIGN.md 4.19; every
// decision is made in float64 on the float32 coordinates widened exactly (EXACT flags: no contraction), so the result is held to
// EQUALITY with matplotlib's Path.contains_points and sklearn's 1-nearest-neighbour classifier (tests/test_garment.py pins both).
//   selection  one thread per vertex; the polygon's vertices staged through LDS in tiles of kPolyTile + 1 float64 pairs (the
//              "+ 1": an edge needs both ends, and the closing edge wraps to the polygon's first vertex); every lane reads the
//              same LDS address (a broadcast); parity per polygon, ORed over the polygons
//   nearest    one LANE per query, 64 queries per workgroup; the source vertices staged through LDS in tiles of kSrcTile,
//              widened once; the four waves of the workgroup take a quarter (kSrcSplit) of every tile each, so a 70,000-vertex
//              mesh is 1,100 workgroups instead of 275; the four (d, j) pairs are combined lexicographically: the lowest index
//              of the exact minimum, whatever the split.  Workgroups without a selected vertex leave at once.
//   output     face flags (any corner kept) and vertex reference flags here; block counts, one scan, order-preserving emission
//              of vertices, vertex ids and renumbered faces: compact_device.h, shared with clean_mesh.hip
// No floating-point atomics, no atomics at all: the flag stores race only with stores of the same value.  Equal bytes from run
// to run.  Coordinates are taken as finite (the host entry points check what they can see).
#include "compact_device.h"

namespace icon {
namespace {

constexpr int kPolyTile = 256;           // polygon edges per LDS tile of the containment kernel (tile + 1 vertices staged)
constexpr int kSrcTile = 512;            // source vertices per LDS tile of the nearest-vertex kernel
constexpr int kSrcSplit = kSrcTile / 4;  // ... of which each of the workgroup's four waves scans this many
constexpr int kNnQueries = 64;           // queries per workgroup of the nearest-vertex kernel: one per lane, the same in all four waves

struct GmCtx {
    const float *verts; const void *faces; int64_t V, F;
    const double *poly; const int32_t *poly_off; int64_t poly_total; int P;
    const float *src; int64_t Vs; const uint8_t *src_remove;
    uint8_t *sel;                                // [V] inside any polygon
    int32_t *nn;                                 // [V] nearest source vertex of a selected vertex, -1 elsewhere
    uint8_t *keep_f, *ref_v;                     // [F], [V]
    int *blk_f, *blk_v;                          // counts / offsets per 256 entries
    int *remap;                                  // [V] new index of a referenced vertex
    int64_t *totals;                             // [0] vertices kept, [1] faces kept
};

// rule 2: the crossings test of Path.contains_points(radius = 0) on a path without codes, closed from the last vertex to the first
__global__ __launch_bounds__(256) void k_gm_contain(const float *__restrict__ verts, int64_t V, const double *__restrict__ poly,
                                                    const int32_t *__restrict__ poly_off, int64_t poly_total, int P, uint8_t *__restrict__ sel)
{
    __shared__ double sx[kPolyTile + 1], sy[kPolyTile + 1];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const double tx = i < V ? (double)verts[3 * i] : 0.0, ty = i < V ? (double)verts[3 * i + 1] : 0.0;
    bool inside = false;
    for (int p = 0; p < P; ++p) {
        const int64_t b = poly_off[p], n = (int64_t)poly_off[p + 1] - b;       // uniform
        if (n < 3 || b < 0 || b + n > poly_total) continue;                    // fewer than 3 vertices select nothing; a bad table reads nothing
        bool odd = false;
        for (int64_t base = 0; base < n; base += kPolyTile) {
            const int m = (int)min((int64_t)kPolyTile, n - base);              // edges of this tile: base + e -> base + e + 1 (n wraps to 0)
            __syncthreads();
            for (int k = threadIdx.x; k <= m; k += 256) {
                int64_t idx = base + k;
                if (idx == n) idx = 0;
                sx[k] = poly[2 * (b + idx)]; sy[k] = poly[2 * (b + idx) + 1];
            }
            __syncthreads();
            double x0 = sx[0], y0 = sy[0];
            bool f0 = y0 >= ty;
            for (int e = 1; e <= m; ++e) {
                const double x1 = sx[e], y1 = sy[e];
                const bool f1 = y1 >= ty;
                if (f0 != f1 && (((y1 - ty) * (x0 - x1) >= (x1 - tx) * (y0 - y1)) == f1)) odd = !odd;
                x0 = x1; y0 = y1; f0 = f1;
            }
        }
        inside = inside || odd;
    }
    if (i < V) sel[i] = inside ? 1 : 0;
}

// rule 3: the lowest j minimising ((dx*dx + dy*dy) + dz*dz), d = verts[i] - src[j], every operation rounded in float64
__global__ __launch_bounds__(256) void k_gm_nearest(const float *__restrict__ verts, int64_t V, const float *__restrict__ src, int64_t Vs,
                                                    const uint8_t *__restrict__ only, int32_t *__restrict__ out)
{
    __shared__ double s[3 * kSrcTile];
    __shared__ double rd[4][kNnQueries];
    __shared__ int rj[4][kNnQueries];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * kNnQueries + lane;
    const bool active = q < V && (!only || only[q]);
    if (!__any(active)) {                                                      // the four waves hold the same 64 queries: uniform over the workgroup
        if (w == 0 && q < V) out[q] = -1;
        return;
    }
    const double qx = q < V ? (double)verts[3 * q] : 0.0, qy = q < V ? (double)verts[3 * q + 1] : 0.0, qz = q < V ? (double)verts[3 * q + 2] : 0.0;
    double bd = __builtin_huge_val();
    int bj = 0;
    for (int64_t base = 0; base < Vs; base += kSrcTile) {
        const int m = (int)min((int64_t)kSrcTile, Vs - base);
        __syncthreads();
        for (int k = threadIdx.x; k < 3 * m; k += 256) s[k] = (double)src[3 * base + k];
        __syncthreads();
        const int lo = w * kSrcSplit, hi = min(lo + kSrcSplit, m);
        for (int k = lo; k < hi; ++k) {                                        // ascending j within the wave: a strict < keeps the lowest index
            const double dx = qx - s[3 * k], dy = qy - s[3 * k + 1], dz = qz - s[3 * k + 2];
            const double d = (dx * dx + dy * dy) + dz * dz;
            if (d < bd) { bd = d; bj = (int)base + k; }
        }
    }
    rd[w][lane] = bd; rj[w][lane] = bj;
    __syncthreads();
    if (w != 0 || q >= V) return;
    for (int o = 1; o < 4; ++o) {                                              // (d, j) pairs, compared as pairs: a wave that saw nothing holds (inf, 0)
        const double d = rd[o][lane]; const int j = rj[o][lane];
        if (d < bd || (d == bd && j < bj)) { bd = d; bj = j; }
    }
    out[q] = active ? bj : -1;
}

// rules 4 and 5: keep_v = selected & !src_remove[nn]; a face is kept when any corner is; a face naming a missing vertex never is
__device__ __forceinline__ bool gm_keep_v(const GmCtx &c, int64_t v)
{
    if (!c.sel[v]) return false;
    if (!c.src_remove) return true;
    const int j = c.nn[v];
    return j >= 0 && j < c.Vs && !c.src_remove[j];
}

template <class IT>
__global__ __launch_bounds__(256) void k_gm_flags(GmCtx c)
{
    const IT *faces = static_cast<const IT *>(c.faces);
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (f < c.F) {
        const int64_t a = faces[3 * f], b = faces[3 * f + 1], d = faces[3 * f + 2];
        if (a >= 0 && b >= 0 && d >= 0 && a < c.V && b < c.V && d < c.V) {
            keep = gm_keep_v(c, a) || gm_keep_v(c, b) || gm_keep_v(c, d);
            if (keep) { c.ref_v[a] = 1; c.ref_v[b] = 1; c.ref_v[d] = 1; }
        }
        c.keep_f[f] = keep ? 1 : 0;
    }
    compact_count(keep, c.blk_f);                                              // a kept face names existing vertices only
}

struct GmLayout { size_t totals, ref_v, zero_end, sel, nn, keep_f, blk_f, blk_v, remap, total; };

GmLayout gm_layout(int64_t V, int64_t F)
{
    GmLayout L{};
    ScratchTake take;
    L.totals = take(16); L.ref_v = take((size_t)V);
    L.zero_end = take.o;                                                       // [0, zero_end): cleared by one memset per call
    L.sel = take((size_t)V); L.nn = take((size_t)V * 4); L.keep_f = take((size_t)F);
    L.blk_f = take((size_t)((F + 255) / 256) * 4); L.blk_v = take((size_t)((V + 255) / 256) * 4); L.remap = take((size_t)V * 4);
    L.total = take.o;
    return L;
}

int gm_check_sizes(int64_t V, int64_t F, int64_t total_poly_verts, int64_t P)
{
    ICON_ARG(V > 0 && F > 0 && V < (1ll << 31) && F < (1ll << 29), "icon_extract_cloth: 0 < V < 2^31, 0 < F < 2^29");
    ICON_ARG(P >= 0 && P < (1ll << 24) && total_poly_verts >= 0 && total_poly_verts < (1ll << 31),
             "icon_extract_cloth: 0 <= P < 2^24 polygons of 0 <= total < 2^31 vertices");
    return ICON_OK;
}

}  // namespace
}  // namespace icon

using namespace icon;

extern "C" int icon_nearest_vertex(const float *d_verts, int64_t V, const float *d_src, int64_t Vs, const uint8_t *d_only,
                                   int32_t *d_out_idx, void *stream)
{
    ICON_ARG(d_verts && d_src && d_out_idx, "icon_nearest_vertex: null argument");
    ICON_ARG(V > 0 && Vs > 0 && V < (1ll << 31) && Vs < (1ll << 31), "icon_nearest_vertex: 0 < V < 2^31, 0 < Vs < 2^31");
    hipLaunchKernelGGL(k_gm_nearest, dim3((unsigned)((V + kNnQueries - 1) / kNnQueries)), dim3(256), 0, (hipStream_t)stream,
                       d_verts, V, d_src, Vs, d_only, d_out_idx);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

extern "C" int icon_extract_cloth_bytes(int64_t V, int64_t F, int64_t total_poly_verts, int64_t P, int64_t *bytes)
{
    ICON_ARG(bytes != nullptr, "icon_extract_cloth_bytes: null argument");
    const int rc = gm_check_sizes(V, F, total_poly_verts, P);
    if (rc) return rc;
    *bytes = (int64_t)gm_layout(V, F).total;
    return ICON_OK;
}

extern "C" int icon_extract_cloth(const float *d_verts, int64_t V, const void *d_faces, int64_t F, int faces_int64,
                                  const double *d_poly_xy, const int32_t *d_poly_off, int64_t total_poly_verts, int64_t P,
                                  const float *d_src, int64_t Vs, const uint8_t *d_src_remove,
                                  float *d_out_verts, int32_t *d_out_faces, int32_t *d_out_vert_ids, int64_t *h_counts,
                                  void *d_scratch, int64_t scratch_bytes, void *stream)
{
    ICON_ARG(d_verts && d_faces && d_poly_off && d_out_verts && d_out_faces && d_out_vert_ids && h_counts && d_scratch,
             "icon_extract_cloth: null argument");
    const int rc = gm_check_sizes(V, F, total_poly_verts, P);
    if (rc) return rc;
    ICON_ARG(d_poly_xy || total_poly_verts == 0, "icon_extract_cloth: null polygon vertices");
    const bool with_src = d_src || Vs || d_src_remove;
    ICON_ARG(!with_src || (d_src && d_src_remove && Vs > 0 && Vs < (1ll << 31)),
             "icon_extract_cloth: d_src, Vs and d_src_remove go together (all NULL / 0: no source mesh), 0 < Vs < 2^31");
    const GmLayout L = gm_layout(V, F);
    if (const int e = scratch_check("icon_extract_cloth", "icon_extract_cloth_bytes", d_scratch, scratch_bytes, L.total)) return e;
    hipStream_t st = (hipStream_t)stream;
    char *s = static_cast<char *>(d_scratch);
    GmCtx c{};
    c.verts = d_verts; c.faces = d_faces; c.V = V; c.F = F;
    c.poly = d_poly_xy; c.poly_off = d_poly_off; c.poly_total = total_poly_verts; c.P = (int)P;
    c.src = d_src; c.Vs = Vs; c.src_remove = d_src_remove;
    c.totals = reinterpret_cast<int64_t *>(s + L.totals); c.ref_v = reinterpret_cast<uint8_t *>(s + L.ref_v);
    c.sel = reinterpret_cast<uint8_t *>(s + L.sel); c.nn = reinterpret_cast<int32_t *>(s + L.nn);
    c.keep_f = reinterpret_cast<uint8_t *>(s + L.keep_f); c.blk_f = reinterpret_cast<int *>(s + L.blk_f);
    c.blk_v = reinterpret_cast<int *>(s + L.blk_v); c.remap = reinterpret_cast<int *>(s + L.remap);
    const unsigned gF = (unsigned)((F + 255) / 256), gV = (unsigned)((V + 255) / 256);
    ICON_HIP(hipMemsetAsync(s, 0, L.zero_end, st));
    hipLaunchKernelGGL(k_gm_contain, dim3(gV), dim3(256), 0, st, d_verts, V, d_poly_xy, d_poly_off, total_poly_verts, (int)P, c.sel);
    if (with_src)
        hipLaunchKernelGGL(k_gm_nearest, dim3((unsigned)((V + kNnQueries - 1) / kNnQueries)), dim3(256), 0, st, d_verts, V, d_src, Vs,
                           (const uint8_t *)c.sel, c.nn);
    if (faces_int64) hipLaunchKernelGGL(k_gm_flags<int64_t>, dim3(gF), dim3(256), 0, st, c);
    else hipLaunchKernelGGL(k_gm_flags<int32_t>, dim3(gF), dim3(256), 0, st, c);
    hipLaunchKernelGGL(k_compact_count_v, dim3(gV), dim3(256), 0, st, c.ref_v, V, c.blk_v);
    hipLaunchKernelGGL(k_compact_scan<int64_t>, dim3(2), dim3(1024), 0, st, c.blk_v, V, c.blk_f, F, c.totals);
    hipLaunchKernelGGL(k_compact_emit_v, dim3(gV), dim3(256), 0, st, d_verts, c.ref_v, V, c.blk_v, c.remap, d_out_verts, d_out_vert_ids);
    if (faces_int64)
        hipLaunchKernelGGL(k_compact_emit_f<int64_t>, dim3(gF), dim3(256), 0, st, static_cast<const int64_t *>(d_faces), c.keep_f, F, c.blk_f, c.remap, d_out_faces);
    else
        hipLaunchKernelGGL(k_compact_emit_f<int32_t>, dim3(gF), dim3(256), 0, st, static_cast<const int32_t *>(d_faces), c.keep_f, F, c.blk_f, c.remap, d_out_faces);
    ICON_HIP(hipGetLastError());
    ICON_HIP(hipMemcpyAsync(h_counts, c.totals, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ICON_HIP(hipStreamSynchronize(st));
    return ICON_OK;
}

// evaluator.hip - the reference's Evaluator on the device (lib/dataset/Evaluator.py: _render_normal / _get_reproj_normal_error /
// calculate_normal_consist / render_normal; call sites apps/ICON.py:556 and :639): the normal maps of one or two meshes from up to
// 32 views by the rule of raster_gl_device.h (PARITY UNPINNED), and per view the mean over the pixels of the
// squared colour difference of the two meshes' maps - the third metric of the paper's table.
//
// Shape of the work: one stream-ordered call, launches only; every buffer lives in the caller's scratch
// (icon_normal_consistency_bytes); nothing is allocated, read back or waited for.  Per mesh: where the caller gives no vertex
// normals, the incidence lists of s1_normals_device.h (count / scan / fill) and its ordered sums over them, in float64, of the
// angle-weighted terms - one thread per vertex for lists up to kShort entries, one wavefront per longer list; one raster launch over
// (face, view): 8 lanes - or one thread - sweep the pixel centres of a face's box and atomicMin the 64-bit key (ordered depth bits,
// face id) into the view's S x S z-buffer; a box above 64 pixels per lane goes to the view's deferred list, which a fixed grid
// of workgroups consumes.  One resolve launch then recomputes every winner's fragment with the same functions, writes the RGBA
// planes and face ids the caller asked for and - with two meshes - reduces the per-pixel error ((d0 d0 + d1 d1) + d2 d2), float32, in
// float64 over 1,024 consecutive pixels by halving (x[i] + x[i + n/2], n = 1024 .. 2); a last launch halves the <= 4,096 partial sums
// of a view (zero-padded to 4,096) the same way and divides by S^2.  No floating-point atomics: equal bytes from run to run.
#pragma clang fp contract(off)

#include "raster_gl_device.h"

namespace icon {

int g_ev_lanes = 0;       // icon_debug_set_option("ev_lanes"): 0 = by the sizes; 1 = a thread per face; 8 = eight lanes per face

namespace {

constexpr int kEvMaxViews = 32;
constexpr int kEvChunk = 1024;       // pixels per workgroup of the resolve pass: 4 per thread
constexpr int kEvParts = 4096;       // partial sums of a view: 2048^2 / kEvChunk at most

struct EvMesh : S1Ctx {              // vis null: every vertex gets a normal
    const float *nrm;                // [V][3] vertex normals: the caller's, or own (below)
    float *own;                      // [V][3] in the scratch, or where the caller wants them
    int *n_big, *big;                // [K] lengths / [K][F] faces of the deferred lists, one per view (raster_device.h)
    unsigned long long *zb;          // [K][S][S], image orientation
    float *rgba; int *pix;           // outputs, or null
    int i64;                         // faces are int64
};
struct EvViews { const float *mats, *muls; int S, K; };
struct EvCtx { EvMesh m[2]; EvViews vw; int n_mesh, nb; double *partial, *err; };

__device__ __forceinline__ bool ev_face(const EvMesh &m, int64_t f, int64_t id[3])
{
    return m.i64 ? s1_face<int64_t>(m, f, id) : s1_face<int32_t>(m, f, id);
}
__device__ __forceinline__ bool ev_setup(const EvMesh &m, const GlView &w, int S, int64_t f, GlFace &r)
{
    return ev_face(m, f, r.id) && gl_setup(m.verts, w, S, r);
}
// pixel (column i, window row j), both in [0, S), of face f into the view's z-buffer plane
__device__ __forceinline__ void ev_pixel(unsigned long long *zb, int S, const GlFace &r, int64_t f, int i, int j)
{
    GlFrag q;
    if (!gl_fragment(r, i, j, q)) return;
    atomicMin(&zb[(size_t)(S - 1 - j) * S + (size_t)i], gl_key(q.z, f));
}

// G lanes per face, 256 / G faces per workgroup; blockIdx.y: the view
template <int G>
__global__ __launch_bounds__(256) void k_ev_raster(EvMesh m, EvViews vw)
{
    const int64_t f = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x % G;
    const int view = blockIdx.y;
    if (f >= m.F) return;
    const GlView w = gl_view(vw.mats, vw.muls, view);
    GlFace r;
    if (!ev_setup(m, w, vw.S, f, r)) return;
    if (r.box.n() > kRsBigPerLane * G) {
        if (sub == 0) rs_defer_view(m.n_big, m.big, m.F, view, f);
        return;
    }
    unsigned long long *zb = m.zb + (size_t)view * vw.S * vw.S;
    rs_sweep<G>(r.box, sub, [&](int i, int j) { ev_pixel(zb, vw.S, r, f, i, j); });
}

// the deferred faces of view blockIdx.y: a workgroup per entry, as many rounds as the list (read from device memory) needs
__global__ __launch_bounds__(256) void k_ev_raster_big(EvMesh m, EvViews vw)
{
    const int view = blockIdx.y;
    const int nb = rs_deferred_view_count(m.n_big, m.F, view);
    const GlView w = gl_view(vw.mats, vw.muls, view);
    unsigned long long *zb = m.zb + (size_t)view * vw.S * vw.S;
    for (int e = blockIdx.x; e < nb; e += gridDim.x) {
        int64_t f;
        GlFace r;
        if (!rs_deferred_view(m.big, m.F, view, e, f) || !ev_setup(m, w, vw.S, f, r)) continue;
        rs_sweep_block(r.box, [&](int i, int j) { ev_pixel(zb, vw.S, r, f, i, j); });
    }
}

// the colour and face of pixel p = (row, col) of a view: the winner's, or the background's
__device__ __forceinline__ void ev_resolve_pixel(const EvMesh &m, const GlView &w, int S, int view, int p, float rgba[4], int &face)
{
    const int row = p / S, col = p - row * S;
    const unsigned long long key = m.zb[(size_t)view * S * S + p];
    rgba[0] = rgba[1] = rgba[2] = 1.0f; rgba[3] = 0.0f;
    face = -1;
    GlFace r;
    GlFrag q;
    // a face in the z-buffer passed ev_setup and gl_fragment at this pixel: the same expressions give the same answer
    const int64_t f = (int64_t)(key & 0xffffffffull);
    if (key == ~0ull || f >= m.F || !ev_setup(m, w, S, f, r) || !gl_fragment(r, col, S - 1 - row, q)) return;
    face = (int)f;
    gl_colour(w, q, m.nrm + 3 * r.id[0], m.nrm + 3 * r.id[1], m.nrm + 3 * r.id[2], rgba);
}

// 256 doubles of a workgroup to one by halving; the result in s[0] after the last barrier
__device__ __forceinline__ void ev_halve_block(double *s)
{
    for (int h = 128; h >= 1; h >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
    }
    __syncthreads();
}

// kEvChunk pixels of view blockIdx.y per workgroup: both meshes' winners, the outputs asked for, the chunk's error sum
__global__ __launch_bounds__(256) void k_ev_resolve(EvCtx c)
{
    __shared__ double s_sum[256];
    const int S = c.vw.S, npx = S * S, view = blockIdx.y;
    const GlView w = gl_view(c.vw.mats, c.vw.muls, view);
    double acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = blockIdx.x * kEvChunk + 256 * j + threadIdx.x;
        float e = 0.0f;
        if (p < npx) {
            float px[2][4];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                if (mi >= c.n_mesh) continue;
                const EvMesh &m = c.m[mi];
                int face;
                ev_resolve_pixel(m, w, S, view, p, px[mi], face);
                if (m.rgba) *reinterpret_cast<float4 *>(m.rgba + ((size_t)view * npx + p) * 4) = make_float4(px[mi][0], px[mi][1], px[mi][2], px[mi][3]);
                if (m.pix) m.pix[(size_t)view * npx + p] = face;
            }
            if (c.n_mesh == 2) {
                const float d0 = px[0][0] - px[1][0], d1 = px[0][1] - px[1][1], d2 = px[0][2] - px[1][2];
                e = (d0 * d0 + d1 * d1) + d2 * d2;
            }
        }
        acc[j] = (double)e;
    }
    if (!c.err) return;
    s_sum[threadIdx.x] = (acc[0] + acc[2]) + (acc[1] + acc[3]);
    ev_halve_block(s_sum);
    if (threadIdx.x == 0) c.partial[(size_t)view * kEvParts + blockIdx.x] = s_sum[0];
}

// view blockIdx.x: its nb partial sums, zero-padded to kEvParts, halved to one; err = sum / S^2
__global__ __launch_bounds__(256) void k_ev_final(EvCtx c)
{
    __shared__ double s_sum[256];
    const int view = blockIdx.x;
    double v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = 256 * j + threadIdx.x;
        v[j] = i < c.nb ? c.partial[(size_t)view * kEvParts + i] : 0.0;
    }
#pragma unroll
    for (int h = 8; h >= 1; h >>= 1)
#pragma unroll
        for (int j = 0; j < h; ++j) v[j] += v[j + h];
    s_sum[threadIdx.x] = v[0];
    ev_halve_block(s_sum);
    if (threadIdx.x == 0) c.err[view] = s_sum[0] / (double)((int64_t)c.vw.S * c.vw.S);
}

// the angle-weighted addend of incidence key `key` (3 face + corner) as s1_normals_device.h's ordered sums take their terms (one
// pass, float64); 0 for a key that names no face
struct EvTerm {
    EvMesh m;
    __device__ void operator()(int, int key, double o[3]) const
    {
        int64_t id[3];
        o[0] = o[1] = o[2] = 0.0;
        if (key < 0 || key / 3 >= m.F || !ev_face(m, key / 3, id)) return;
        gl_angle_term(m.verts + 3 * id[0], m.verts + 3 * id[1], m.verts + 3 * id[2], key % 3, o);
    }
};
// a sum into the mesh's normals: sum / |sum|, rounded once
struct EvStore {
    float *nrm;
    __device__ void operator()(int64_t v, double x, double y, double z) const { gl_store_normal(nrm, v, x, y, z); }
};

// one thread per vertex: the normal of a short incidence list; a long one goes to k_s1_sum_long's list - with a zero written
// first, which stays if that kernel ever found the vertex's list out of range
__global__ __launch_bounds__(256) void k_ev_normals(EvTerm term)
{
    const EvMesh &m = term.m;
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= m.V) return;
    const int n = m.deg[v];
    double s[3] = { 0.0, 0.0, 0.0 };
    if (n > kShort) s1_defer_long(m, v);
    else s1_sum_short_terms(m, v, n, 1, term, s);
    gl_store_normal(m.own, v, s[0], s[1], s[2]);
}

// the call's clears: each mesh's counters and S1 words to 0, the z-buffers to ~0 - a kernel like the others, so that a captured
// call consists of kernel nodes only
__global__ __launch_bounds__(256) void k_ev_clear(uint32_t *z0, size_t n0, uint32_t *z1, size_t n1, unsigned long long *zb, size_t n_zb)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n0 || i < n1 || i < n_zb; i += stride) {
        if (i < n0) z0[i] = 0u;
        if (i < n1) z1[i] = 0u;
        if (i < n_zb) zb[i] = ~0ull;
    }
}

// ---- host ----
struct EvLayout { size_t cnt[2]; S1Layout s1[2]; size_t nrm[2], zb, partial, total; };     // a mesh's deferred lists: s1.mid

EvLayout ev_layout(const int64_t V[2], const int64_t F[2], int n_mesh, int S, int K)
{
    EvLayout L{};
    ScratchTake take;
    for (int mi = 0; mi < n_mesh; ++mi) {
        L.cnt[mi] = take((size_t)kEvMaxViews * 4);                          // directly in front of the S1 header: one range to clear
        L.s1[mi] = s1_layout(take, V[mi], F[mi], (size_t)F[mi] * 4 * K);
        L.nrm[mi] = take((size_t)V[mi] * 12);
    }
    L.zb = take((size_t)n_mesh * K * S * S * 8);
    L.partial = take((size_t)K * kEvParts * 8);
    L.total = take.o;
    return L;
}

int ev_check_sizes(const int64_t V[2], const int64_t F[2], int n_mesh, int size, int n_views)
{
    for (int mi = 0; mi < n_mesh; ++mi) {
        const int rc = rs_check_sizes("icon_normal_consistency", V[mi], F[mi], size, n_views, kEvMaxViews);
        if (rc) return rc;
    }
    return ICON_OK;
}

template <class IT>
void ev_launch_normals(const EvMesh &m, hipStream_t st)
{
    const S1Ctx &s1 = m;                                                    // the shared kernels take the base alone
    s1_launch_lists<IT>(s1, st);
    hipLaunchKernelGGL(k_ev_normals, dim3((unsigned)((m.V + 255) / 256)), dim3(256), 0, st, EvTerm{m});
    hipLaunchKernelGGL((k_s1_sum_long<EvTerm, EvStore, double>), dim3(kLongGrid), dim3(64), 0, st, s1, 1, EvTerm{m}, EvStore{m.own});
}

// lanes per face of a mesh's sweep, by the sizes alone (rs_lanes' rule); icon_debug_set_option("ev_lanes") forces 1 or 8
int ev_lanes(int64_t F, int S)
{
    return g_ev_lanes == 1 ? 1 : (g_ev_lanes == 8 ? 8 : (8 * F > (int64_t)S * S ? 1 : kRsLanes));
}

}  // namespace
}  // namespace icon

using namespace icon;

extern "C" int icon_normal_consistency_bytes(int64_t Va, int64_t Fa, int64_t Vb, int64_t Fb, int size, int n_views, int64_t *bytes)
{
    ICON_ARG(bytes != nullptr, "icon_normal_consistency_bytes: null argument");
    const int64_t V[2] = { Va, Vb }, F[2] = { Fa, Fb };
    const int n_mesh = (Vb == 0 && Fb == 0) ? 1 : 2;
    const int rc = ev_check_sizes(V, F, n_mesh, size, n_views);
    if (rc) return rc;
    *bytes = (int64_t)ev_layout(V, F, n_mesh, size, n_views).total;
    return ICON_OK;
}

extern "C" int icon_normal_consistency(const float *d_verts_a, int64_t Va, const void *d_faces_a, int64_t Fa, int faces_a_int64,
                                       const float *d_normals_a, const float *d_verts_b, int64_t Vb, const void *d_faces_b, int64_t Fb,
                                       int faces_b_int64, const float *d_normals_b, const float *d_view_mats, const float *d_view_muls,
                                       int n_views, int size, double *d_err, float *d_rgba_a, float *d_rgba_b, int32_t *d_pix_a,
                                       int32_t *d_pix_b, float *d_normals_out_a, float *d_normals_out_b, void *d_scratch,
                                       int64_t scratch_bytes, void *stream)
{
    ICON_ARG(d_verts_a && d_faces_a && d_view_mats && d_view_muls && d_scratch, "icon_normal_consistency: null argument");
    const int n_mesh = (d_verts_b || d_faces_b || Vb || Fb) ? 2 : 1;
    if (n_mesh == 2) ICON_ARG(d_verts_b && d_faces_b && d_err, "icon_normal_consistency: the second mesh needs verts, faces and err");
    else ICON_ARG(!d_err && !d_normals_b && !d_rgba_b && !d_pix_b && !d_normals_out_b, "icon_normal_consistency: a single mesh has no err and no second outputs");
    ICON_ARG(!(d_normals_a && d_normals_out_a) && !(d_normals_b && d_normals_out_b), "icon_normal_consistency: normals are given or asked for, not both");
    const int64_t V[2] = { Va, Vb }, F[2] = { Fa, Fb };
    const int rc = ev_check_sizes(V, F, n_mesh, size, n_views);
    if (rc) return rc;
    const EvLayout L = ev_layout(V, F, n_mesh, size, n_views);
    if (const int e = scratch_check("icon_normal_consistency", "icon_normal_consistency_bytes", d_scratch, scratch_bytes, L.total)) return e;
    ICON_ARG((((uintptr_t)d_rgba_a | (uintptr_t)d_rgba_b) & 15) == 0, "icon_normal_consistency: the RGBA outputs must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char *s = static_cast<char *>(d_scratch);
    const float *verts[2] = { d_verts_a, d_verts_b }, *normals[2] = { d_normals_a, d_normals_b };
    const void *faces[2] = { d_faces_a, d_faces_b };
    float *rgba[2] = { d_rgba_a, d_rgba_b };
    int32_t *pix[2] = { d_pix_a, d_pix_b };
    float *nrm_out[2] = { d_normals_out_a, d_normals_out_b };
    const int i64[2] = { faces_a_int64, faces_b_int64 };
    const size_t npx = (size_t)size * size;
    EvCtx c{};
    c.vw = EvViews{ d_view_mats, d_view_muls, size, n_views };
    c.n_mesh = n_mesh; c.nb = (int)((npx + kEvChunk - 1) / kEvChunk);
    c.partial = reinterpret_cast<double *>(s + L.partial); c.err = d_err;
    for (int mi = 0; mi < n_mesh; ++mi) {
        EvMesh &m = c.m[mi];
        m.verts = verts[mi]; m.faces = faces[mi]; m.V = V[mi]; m.F = F[mi]; m.vis = nullptr;
        s1_bind(m, s, L.s1[mi]);
        m.own = nrm_out[mi] ? nrm_out[mi] : reinterpret_cast<float *>(s + L.nrm[mi]); m.nrm = normals[mi] ? normals[mi] : m.own;
        m.n_big = reinterpret_cast<int *>(s + L.cnt[mi]); m.big = reinterpret_cast<int *>(s + L.s1[mi].mid);
        m.zb = reinterpret_cast<unsigned long long *>(s + L.zb) + (size_t)mi * n_views * npx;
        m.rgba = rgba[mi]; m.pix = pix[mi]; m.i64 = i64[mi] ? 1 : 0;
    }
    const size_t n0 = (L.s1[0].zero_end - L.cnt[0]) / 4, n1 = n_mesh == 2 ? (L.s1[1].zero_end - L.cnt[1]) / 4 : 0;
    const size_t n_zb = (size_t)n_mesh * n_views * npx, n = n_zb > (n0 > n1 ? n0 : n1) ? n_zb : (n0 > n1 ? n0 : n1);
    hipLaunchKernelGGL(k_ev_clear, dim3((unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), dim3(256), 0, st,
                       reinterpret_cast<uint32_t *>(s + L.cnt[0]), n0, reinterpret_cast<uint32_t *>(s + L.cnt[n_mesh - 1]), n1,
                       reinterpret_cast<unsigned long long *>(s + L.zb), n_zb);
    for (int mi = 0; mi < n_mesh; ++mi) {
        const EvMesh &m = c.m[mi];
        const int G = ev_lanes(m.F, size);
        const dim3 gR((unsigned)((m.F * G + 255) / 256), (unsigned)n_views);
        if (G == 1) hipLaunchKernelGGL(k_ev_raster<1>, gR, dim3(256), 0, st, m, c.vw);
        else hipLaunchKernelGGL(k_ev_raster<8>, gR, dim3(256), 0, st, m, c.vw);
        hipLaunchKernelGGL(k_ev_raster_big, dim3(256, (unsigned)n_views), dim3(256), 0, st, m, c.vw);
        if (!normals[mi]) {
            if (m.i64) ev_launch_normals<int64_t>(m, st); else ev_launch_normals<int32_t>(m, st);
        }
    }
    hipLaunchKernelGGL(k_ev_resolve, dim3((unsigned)c.nb, (unsigned)n_views), dim3(256), 0, st, c);
    if (d_err) hipLaunchKernelGGL(k_ev_final, dim3((unsigned)n_views), dim3(256), 0, st, c);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

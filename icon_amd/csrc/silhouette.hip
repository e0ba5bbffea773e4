// silhouette.hip - the soft silhouette of a mesh from ICON's four orthographic cameras, forwards and backwards
// (lib/common/render.py Render.get_silhouette_image: pytorch3d MeshRasterizer + SoftSilhouetteShader; the SMPL fit loop of
// apps/infer.py:163-273 renders it every iteration and back-propagates its loss into pose, shape and translation).
//
// The rule (PARITY UNPINNED): pytorch3d's rasteriser for RasterizationSettings(image_size=S,
// blur_radius=log(1/1e-4 - 1)*5e-5, faces_per_pixel=50, cull_backfaces=True) and SoftSilhouetteShader(sigma=1e-4), restated in
// float32 with the views, NDC and per-face expressions of raster_device.h (shared with render_normal.hip):
//   a face is skipped unless |area| > 1e-8, culled when area < 0; at a pixel centre p it is a candidate when its three barycentrics
//   are all > 0 (inside) or m = min(seg(v0,v1), seg(v0,v2), seg(v1,v2)) < blur (the first minimum wins), and its clamped-barycentric
//   depth is not negative; d = -m inside, +m outside; prob = 1 / (1 + exp(d / sigma)); alpha = 1 - prod(1 - prob) over ALL the
//   pixel's candidates, in ascending face order (pytorch3d keeps the 50 nearest: a storage limit, not part of the definition).
//   Backwards: d alpha / d d_k = -(1 - alpha) prob_k / sigma; d m / d(a, b) of the winning edge with e = p - q: -2 (1 - t) e and -2 t e,
//   t the clamped parameter (1 in the degenerate branch).  Candidate set and culling carry no gradient.
//
// Shape of the work.  Forward: a pre-pass writes one record per (view, face) - projected corners, area + eps - and its pixel box
// grown by sqrt(blur) (empty for a skipped or culled face); one wavefront per 8 x 8 pixel tile then walks ALL faces in ascending
// order, 64 box tests at a time, ballots the overlaps and lets each pixel lane multiply 1 - prob for the hits in that order: no
// bins, no atomics, one writer per pixel.  Backward: eight lanes sweep a face's box (lane s takes pixels s, s + 8, ...), skip a
// pixel whose grad_alpha (1 - alpha) is zero, accumulate the six partials in registers and add them across the lanes in lane
// order; each (view, face) writes its per-corner gradients into the scratch, and a per-vertex kernel adds a vertex's corners in
// ascending 3 face + corner order, view by view, through the S1 incidence lists (s1_normals_device.h).  Both directions give the same
// bytes from run to run.  Everything is enqueued on the caller's stream; nothing is allocated, read back or waited for; the call's
// clears are a kernel of its own (a captured call consists of kernel nodes only).
#pragma clang fp contract(off)

#include "raster_device.h"

namespace icon {
namespace {

constexpr float kSilBlur = 4.605120048e-04f;     // float32(log(1 / 1e-4 - 1) * 5e-5): squared NDC distance
constexpr float kSilBlurR = 2.145954408e-02f;    // float32 sqrt of it: the pixel box grows by this
constexpr float kSilSigma = 9.999999747e-05f;    // float32(1e-4): BlendParams().sigma
constexpr uint32_t kSilEmptyBox = 0x0000ffffu;   // i0 = 0xffff > i1 = 0: overlaps no tile

struct SilRec { float X[3], Y[3], D[3], den, pad0, pad1; };          // 48 bytes
struct SilBox { uint32_t i, j; };                                    // lo | hi << 16, MIRRORED pixel indices (i = S-1-column, j = S-1-row)

struct SilCtx : RsCtx {
    int count_bad;
    SilRec *rec;                     // [n_views][F]
    SilBox *box;                     // [n_views][F]
    float *cg;                       // [n_views][3 F][2] per-corner gradient (d/dX, d/dY), backward only
    float *alpha_out;                // forward
    const float *alpha, *grad_alpha; // backward
    float *grad_verts;               // [V][3]
};

// the per-pixel rule: is the face a candidate at the pixel centre (px, py); its probability, and for the gradient the sign of
// d d / d m, the winning edge (0: v0 v1, 1: v0 v2, 2: v1 v2) and that edge's e and t
struct SilHit { float prob, sgn, ex, ey, t; int edge; };
__device__ __forceinline__ bool sil_eval(const SilRec &r, float px, float py, SilHit &h)
{
    float w[3];
    rs_weights(r.X, r.Y, r.den, px, py, w);
    const bool inside = rs_inside(w);
    RsSeg best = rs_seg(px, py, r.X[0], r.Y[0], r.X[1], r.Y[1]);
    h.edge = 0;
    const RsSeg s02 = rs_seg(px, py, r.X[0], r.Y[0], r.X[2], r.Y[2]);
    if (s02.d2 < best.d2) { best = s02; h.edge = 1; }
    const RsSeg s12 = rs_seg(px, py, r.X[1], r.Y[1], r.X[2], r.Y[2]);
    if (s12.d2 < best.d2) { best = s12; h.edge = 2; }
    if (!(inside || best.d2 < kSilBlur)) return false;
    if (rs_depth(rs_bary(w), r.D) < 0.0f) return false;
    const float d = inside ? -best.d2 : best.d2;
    h.prob = 1.0f / (1.0f + expf(d / kSilSigma));
    h.sgn = inside ? -1.0f : 1.0f;
    h.ex = best.ex; h.ey = best.ey; h.t = best.t;
    return true;
}

// one thread per (face, view): the record and the pixel box of the face as the view's camera sees it - for a skipped or culled
// face the record still holds its corners and den, and the box is empty
template <class IT>
__global__ __launch_bounds__(256) void k_sil_pre(SilCtx c)
{
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int view = blockIdx.y;
    if (f >= c.F) return;
    SilRec r = {};
    SilBox b = { kSilEmptyBox, kSilEmptyBox };
    int64_t id[3];
    if (!s1_face<IT>(c, f, id)) {
        if (c.count_bad && view == 0) atomicAdd(c.bad_faces, 1);
    } else {
        rs_project(c, c.cam(view), id, r.X, r.Y, r.D);
        const float area = rs_area(r.X, r.Y);
        r.den = area + kRsEps;
        if (rs_drawn(area) && !(area < 0.0f)) {
            const RsBox q = rs_box(rs_bounds(r.X, r.Y, kSilBlurR), c.S);
            if (!q.empty()) { b.i = (uint32_t)q.i0 | ((uint32_t)q.i1 << 16); b.j = (uint32_t)q.j0 | ((uint32_t)q.j1 << 16); }   // 0 <= lo <= hi < S <= 2048
        }
    }
    const size_t at = (size_t)view * c.F + f;
    c.rec[at] = r; c.box[at] = b;
}

// forward: one wavefront per 8 x 8 tile of mirrored pixel indices, four tiles per workgroup; blockIdx.y: the view
__global__ __launch_bounds__(256) void k_sil_tile(SilCtx c)
{
    const int lane = threadIdx.x & 63;
    const int T = (c.S + 7) >> 3;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int view = blockIdx.y, cam = c.cam(view);
    if (tile >= T * T) return;                                             // the whole wavefront
    const int tj = tile / T, ti = tile - tj * T;
    const uint32_t ilo = (uint32_t)ti * 8, jlo = (uint32_t)tj * 8;
    const int i = (int)ilo + (lane & 7), j = (int)jlo + (lane >> 3);
    const float px = rs_centre(i, c.S), py = rs_centre(j, c.S);
    const SilBox *box = c.box + (size_t)view * c.F;
    const SilRec *rec = c.rec + (size_t)view * c.F;
    float prod = 1.0f;
    for (int64_t base = 0; base < c.F; base += 64) {
        bool hit = false;
        if (base + lane < c.F) {
            const SilBox b = box[base + lane];
            hit = (b.i & 0xffffu) <= ilo + 7 && (b.i >> 16) >= ilo && (b.j & 0xffffu) <= jlo + 7 && (b.j >> 16) >= jlo;
        }
        unsigned long long mask = __ballot(hit);
        while (mask) {                                                     // wave-uniform: ascending face order
            const int k = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const SilRec r = rec[base + k];
            SilHit h;
            if (sil_eval(r, px, py, h)) prod = prod * (1.0f - h.prob);
        }
    }
    if (i < c.S && j < c.S) c.alpha_out[(size_t)view * c.S * c.S + rs_at(c, cam, i, j)] = 1.0f - prod;
}

// backward: kRsLanes lanes per face, 256 / kRsLanes faces per workgroup; blockIdx.y: the view.  Writes the face's six partials
// (zeros for a face that draws nothing) to cg[view][3 f + corner][X, Y]
__global__ __launch_bounds__(256) void k_sil_bwd(SilCtx c)
{
    const int64_t f = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kRsLanes;
    const int sub = threadIdx.x % kRsLanes;
    const int view = blockIdx.y, cam = c.cam(view);
    if (f >= c.F) return;                                                  // whole groups of kRsLanes lanes
    const size_t at = (size_t)view * c.F + f;
    const SilBox b = c.box[at];
    const RsBox q = { (int)(b.i & 0xffffu), (int)(b.i >> 16), (int)(b.j & 0xffffu), (int)(b.j >> 16) };
    float g[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };                   // X0 Y0 X1 Y1 X2 Y2
    if (!q.empty() && q.i1 < c.S && q.j1 < c.S) {                          // what k_sil_pre wrote passes; nothing else is an address
        const SilRec r = c.rec[at];
        rs_sweep<kRsLanes>(q, sub, [&](int i, int j) {
            const size_t pix = (size_t)view * c.S * c.S + rs_at(c, cam, i, j);
            const float k = c.grad_alpha[pix] * (1.0f - c.alpha[pix]);
            SilHit h;
            if (k != 0.0f && sil_eval(r, rs_centre(i, c.S), rs_centre(j, c.S), h)) {
                const float dm = (-(k * h.prob) / kSilSigma) * h.sgn;      // d loss / d m of this pair
                const float ca = (-2.0f * (1.0f - h.t)) * dm, cb = (-2.0f * h.t) * dm;
                const float c0 = h.edge == 2 ? 0.0f : ca, c1 = h.edge == 0 ? cb : (h.edge == 2 ? ca : 0.0f), c2 = h.edge == 0 ? 0.0f : cb;
                g[0] += c0 * h.ex; g[1] += c0 * h.ey; g[2] += c1 * h.ex; g[3] += c1 * h.ey; g[4] += c2 * h.ex; g[5] += c2 * h.ey;
            }
        });
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {                                          // lane order: the same sum every run
        float s = 0.0f;
        for (int l = 0; l < kRsLanes; ++l) s += __shfl(g[q], l, kRsLanes);
        g[q] = s;
    }
    if (sub == 0) {
        float *o = c.cg + ((size_t)view * 3 * c.F + 3 * f) * 2;
#pragma unroll
        for (int q = 0; q < 6; ++q) o[q] = g[q];
    }
}

// the addends of incidence key 3 f + corner in view `pass`: (d/dX, d/dY) of that corner on the world's axes
struct SilTerm {
    const float *cg; int64_t F; int cams;
    __device__ void operator()(int pass, int key, float o[3]) const { rs_world_term(cg, F, cams, pass, key, o); }
};
struct SilStore {
    float *out;
    __device__ void operator()(int64_t v, float x, float y, float z) const { out[3 * v] = x; out[3 * v + 1] = y; out[3 * v + 2] = z; }
};

// one thread per vertex: the sum of a short incidence list; a long one goes to k_s1_sum_long's list
__global__ __launch_bounds__(256) void k_sil_vertex(SilCtx c, SilTerm term)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= c.V) return;
    const int n = c.deg[v];
    if (n > kShort) { s1_defer_long(c, v); return; }
    float s[3];
    s1_sum_short_terms(c, v, n, c.n_views, term, s);
    SilStore{c.grad_verts}(v, s[0], s[1], s[2]);
}

struct SilLayout { S1Layout s1; size_t rec, box, cg, total; };

SilLayout sil_layout(int64_t V, int64_t F, int n_views)
{
    SilLayout L{};
    ScratchTake take;
    L.s1 = s1_layout(take, V, F);
    L.rec = take((size_t)F * n_views * sizeof(SilRec)); L.box = take((size_t)F * n_views * sizeof(SilBox));
    L.cg = take((size_t)F * n_views * 24);
    L.total = take.o;
    return L;
}

// the checks both directions share, the context over the caller's scratch, and the call's clear
int sil_context(const float *d_verts, int64_t V, const void *d_faces, int64_t F, const int *cam_ids, int n_views, int size,
                void *d_scratch, int64_t scratch_bytes, hipStream_t st, SilCtx &c)
{
    ICON_ARG(d_verts && d_faces && cam_ids && d_scratch, "icon_silhouette: null argument");
    const SilLayout L = sil_layout(V, F, n_views);
    c = SilCtx{};
    const int rc = rs_context("icon_silhouette", "icon_silhouette_bytes", d_verts, V, d_faces, F, cam_ids, n_views, size,
                              d_scratch, scratch_bytes, L.total, c);
    if (rc) return rc;
    char *s = static_cast<char *>(d_scratch);
    s1_bind(c, s, L.s1);
    c.rec = reinterpret_cast<SilRec *>(s + L.rec); c.box = reinterpret_cast<SilBox *>(s + L.box); c.cg = reinterpret_cast<float *>(s + L.cg);
    rs_clear(s, L.s1, nullptr, 0, st);
    return ICON_OK;
}

template <class IT>
void sil_backward_launch(const SilCtx &c, hipStream_t st)
{
    hipLaunchKernelGGL(k_sil_pre<IT>, dim3((unsigned)((c.F + 255) / 256), (unsigned)c.n_views), dim3(256), 0, st, c);
    hipLaunchKernelGGL(k_sil_bwd, dim3((unsigned)((c.F * kRsLanes + 255) / 256), (unsigned)c.n_views), dim3(256), 0, st, c);
    const S1Ctx &s1 = c;                                                   // the shared kernels take the base alone
    s1_launch_lists<IT>(s1, st);
    const SilTerm term{c.cg, c.F, c.cams};
    hipLaunchKernelGGL(k_sil_vertex, dim3((unsigned)((c.V + 255) / 256)), dim3(256), 0, st, c, term);
    hipLaunchKernelGGL((k_s1_sum_long<SilTerm, SilStore>), dim3(kLongGrid), dim3(64), 0, st, s1, c.n_views, term, SilStore{c.grad_verts});
}

}  // namespace
}  // namespace icon

using namespace icon;

extern "C" int icon_silhouette_bytes(int64_t V, int64_t F, int size, int n_views, int64_t *bytes)
{
    ICON_ARG(bytes != nullptr, "icon_silhouette_bytes: null argument");
    const int rc = rs_check_sizes("icon_silhouette", V, F, size, n_views);
    if (rc) return rc;
    *bytes = (int64_t)sil_layout(V, F, n_views).total;
    return ICON_OK;
}

extern "C" int icon_silhouette_forward(const float *d_verts, int64_t V, const void *d_faces, int64_t F, int faces_int64,
                                       const int *cam_ids, int n_views, int size, float *d_alpha,
                                       void *d_scratch, int64_t scratch_bytes, void *stream)
{
    ICON_ARG(d_alpha != nullptr, "icon_silhouette_forward: null argument");
    SilCtx c;
    hipStream_t st = (hipStream_t)stream;
    const int rc = sil_context(d_verts, V, d_faces, F, cam_ids, n_views, size, d_scratch, scratch_bytes, st, c);
    if (rc) return rc;
    c.alpha_out = d_alpha; c.count_bad = 1;
    const dim3 gP((unsigned)((F + 255) / 256), (unsigned)n_views);
    if (faces_int64) hipLaunchKernelGGL(k_sil_pre<int64_t>, gP, dim3(256), 0, st, c);
    else hipLaunchKernelGGL(k_sil_pre<int32_t>, gP, dim3(256), 0, st, c);
    const int T = (size + 7) / 8;
    hipLaunchKernelGGL(k_sil_tile, dim3((unsigned)((T * T + 3) / 4), (unsigned)n_views), dim3(256), 0, st, c);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

extern "C" int icon_silhouette_backward(const float *d_verts, int64_t V, const void *d_faces, int64_t F, int faces_int64,
                                        const int *cam_ids, int n_views, int size, const float *d_alpha, const float *d_grad_alpha,
                                        float *d_grad_verts, void *d_scratch, int64_t scratch_bytes, void *stream)
{
    ICON_ARG(d_alpha && d_grad_alpha && d_grad_verts, "icon_silhouette_backward: null argument");
    SilCtx c;
    hipStream_t st = (hipStream_t)stream;
    const int rc = sil_context(d_verts, V, d_faces, F, cam_ids, n_views, size, d_scratch, scratch_bytes, st, c);
    if (rc) return rc;
    c.alpha = d_alpha; c.grad_alpha = d_grad_alpha; c.grad_verts = d_grad_verts; c.count_bad = 0;   // k_s1_count counts the bad faces here
    if (faces_int64) sil_backward_launch<int64_t>(c, st); else sil_backward_launch<int32_t>(c, st);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

// silhouette.hip - the soft silhouette of a mesh from ICON's four orthographic cameras, forwards and backwards
// (lib/common/render.py Render.get_silhouette_image: pytorch3d MeshRasterizer + SoftSilhouetteShader; the SMPL fit loop of
// apps/infer.py:163-273 renders it every iteration and back-propagates its loss into pose, shape and translation).
//
// The rule (PARITY UNPINNED): pytorch3d's rasteriser for RasterizationSettings(image_size=S,
// blur_radius=log(1/1e-4 - 1)*5e-5, faces_per_pixel=50, cull_backfaces=True) and SoftSilhouetteShader(sigma=1e-4), restated in
// float32 with the views, NDC and per-face expressions of render_normal.hip:
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

#include "s1_normals_device.h"

namespace icon {
namespace {

constexpr int kSilLanes = 8;                     // lanes per face of the backward sweep
constexpr float kSilBlur = 4.605120048e-04f;     // float32(log(1 / 1e-4 - 1) * 5e-5): squared NDC distance
constexpr float kSilBlurR = 2.145954408e-02f;    // float32 sqrt of it: the pixel box grows by this
constexpr float kSilSigma = 9.999999747e-05f;    // float32(1e-4): BlendParams().sigma
constexpr float kSilEps = 1e-8f;                 // pytorch3d's kEpsilon
constexpr uint32_t kSilEmptyBox = 0x0000ffffu;   // i0 = 0xffff > i1 = 0: overlaps no tile

struct SilHdr { int bad_faces, n_long, pad0, pad1; };
struct SilRec { float X[3], Y[3], D[3], den, pad0, pad1; };          // 48 bytes
struct SilBox { uint32_t i, j; };                                    // lo | hi << 16, MIRRORED pixel indices (i = S-1-column, j = S-1-row)

struct SilCtx : S1Ctx {
    int S, n_views, cams, flip, count_bad;
    SilHdr *hdr;
    SilRec *rec;                     // [n_views][F]
    SilBox *box;                     // [n_views][F]
    float *cg;                       // [n_views][3 F][2] per-corner gradient (d/dX, d/dY), backward only
    float *alpha_out;                // forward
    const float *alpha, *grad_alpha; // backward
    float *grad_verts;               // [V][3]
};

__device__ __forceinline__ float sil_ef(float px, float py, float ax, float ay, float bx, float by)
{
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}
__device__ __forceinline__ float sil_max(float a, float b) { return (a > b) ? a : b; }
__device__ __forceinline__ float sil_min(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float sil_centre(int i, int S) { return -1.0f + (float)(2 * i + 1) / (float)S; }

// squared distance of p to the segment a b (render_normal.hip's rn_seg), with what the gradient needs: e = p - q, the clamped t
struct SilSeg { float d2, ex, ey, t; };
__device__ __forceinline__ SilSeg sil_seg(float px, float py, float ax, float ay, float bx, float by)
{
    const float dx = bx - ax, dy = by - ay;
    const float l2 = dx * dx + dy * dy;
    float qx = bx, qy = by;
    SilSeg s;
    s.t = 1.0f;
    if (!(l2 <= kSilEps)) {
        const float t = (dx * (px - ax) + dy * (py - ay)) / l2;
        s.t = sil_min(sil_max(t, 0.0f), 1.0f);
        qx = ax + s.t * dx; qy = ay + s.t * dy;
    }
    s.ex = px - qx; s.ey = py - qy;
    s.d2 = s.ex * s.ex + s.ey * s.ey;
    return s;
}

// the per-pixel rule: is the face a candidate at the pixel centre (px, py); its probability, and for the gradient the sign of
// d d / d m, the winning edge (0: v0 v1, 1: v0 v2, 2: v1 v2) and that edge's e and t
struct SilHit { float prob, sgn, ex, ey, t; int edge; };
__device__ __forceinline__ bool sil_eval(const SilRec &r, float px, float py, SilHit &h)
{
    const float w0 = sil_ef(px, py, r.X[1], r.Y[1], r.X[2], r.Y[2]) / r.den;
    const float w1 = sil_ef(px, py, r.X[2], r.Y[2], r.X[0], r.Y[0]) / r.den;
    const float w2 = sil_ef(px, py, r.X[0], r.Y[0], r.X[1], r.Y[1]) / r.den;
    const bool inside = w0 > 0.0f && w1 > 0.0f && w2 > 0.0f;
    SilSeg best = sil_seg(px, py, r.X[0], r.Y[0], r.X[1], r.Y[1]);
    h.edge = 0;
    const SilSeg s02 = sil_seg(px, py, r.X[0], r.Y[0], r.X[2], r.Y[2]);
    if (s02.d2 < best.d2) { best = s02; h.edge = 1; }
    const SilSeg s12 = sil_seg(px, py, r.X[1], r.Y[1], r.X[2], r.Y[2]);
    if (s12.d2 < best.d2) { best = s12; h.edge = 2; }
    if (!(inside || best.d2 < kSilBlur)) return false;
    const float c0 = sil_max(sil_min(w0, 1.0f), 0.0f), c1 = sil_max(sil_min(w1, 1.0f), 0.0f), c2 = sil_max(sil_min(w2, 1.0f), 0.0f);
    const float s = sil_max((c0 + c1) + c2, 1e-5f);
    const float pz = ((c0 / s) * r.D[0] + (c1 / s) * r.D[1]) + (c2 / s) * r.D[2];
    if (pz < 0.0f) return false;
    const float d = inside ? -best.d2 : best.d2;
    h.prob = 1.0f / (1.0f + expf(d / kSilSigma));
    h.sgn = inside ? -1.0f : 1.0f;
    h.ex = best.ex; h.ey = best.ey; h.t = best.t;
    return true;
}

// the call's clears: [0, n) words of the scratch (header, incidence counts, fill cursors) - a kernel like the others
__global__ __launch_bounds__(256) void k_sil_clear(uint32_t *zero, size_t n)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) zero[i] = 0u;
}

// one thread per (face, view): the record and the pixel box of the face as the view's camera sees it
template <class IT>
__global__ __launch_bounds__(256) void k_sil_pre(SilCtx c)
{
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int view = blockIdx.y, cam = (c.cams >> (2 * view)) & 3;
    if (f >= c.F) return;
    SilRec r = {};
    SilBox b = { kSilEmptyBox, kSilEmptyBox };
    int64_t id[3];
    if (!s1_face<IT>(c, f, id)) {
        if (c.count_bad && view == 0) atomicAdd(&c.hdr->bad_faces, 1);
    } else {
        const bool side = (cam & 1) != 0, neg = (cam == 0 || cam == 3), front = cam < 2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float *p = c.verts + 3 * id[k];
            const float xa = side ? p[2] : p[0], za = side ? p[0] : p[2];
            r.X[k] = neg ? -xa : xa; r.Y[k] = p[1]; r.D[k] = front ? 100.0f - za : 100.0f + za;
        }
        const float area = sil_ef(r.X[2], r.Y[2], r.X[0], r.Y[0], r.X[1], r.Y[1]);
        r.den = area + kSilEps;
        if (fabsf(area) > kSilEps && !(area < 0.0f)) {
            const float xlo = sil_min(r.X[0], sil_min(r.X[1], r.X[2])) - kSilBlurR, xhi = sil_max(r.X[0], sil_max(r.X[1], r.X[2])) + kSilBlurR;
            const float ylo = sil_min(r.Y[0], sil_min(r.Y[1], r.Y[2])) - kSilBlurR, yhi = sil_max(r.Y[0], sil_max(r.Y[1], r.Y[2])) + kSilBlurR;
            // as rn_setup: the floors without the halves are wider than needed by up to half a pixel on each side (their rounding is
            // ~1e-4 pixel); clamped as floats, so that what is converted lies in [-1, S] whatever the coordinates are (NaN included)
            const float fS = (float)c.S;
            const int i0 = (int)floorf(fminf(fmaxf((xlo + 1.0f) * 0.5f * fS, 0.0f), fS));
            const int i1 = (int)floorf(fminf(fmaxf((xhi + 1.0f) * 0.5f * fS, -1.0f), fS - 1.0f));
            const int j0 = (int)floorf(fminf(fmaxf((ylo + 1.0f) * 0.5f * fS, 0.0f), fS));
            const int j1 = (int)floorf(fminf(fmaxf((yhi + 1.0f) * 0.5f * fS, -1.0f), fS - 1.0f));
            if (i0 <= i1 && j0 <= j1) { b.i = (uint32_t)i0 | ((uint32_t)i1 << 16); b.j = (uint32_t)j0 | ((uint32_t)j1 << 16); }   // 0 <= lo <= hi < S <= 2048
        }
    }
    const size_t at = (size_t)view * c.F + f;
    c.rec[at] = r; c.box[at] = b;
}

// where the pixel of mirrored indices (i, j) lives in an [n_views][S][S] plane set (the cam-2 mirror of the two-view call included)
__device__ __forceinline__ size_t sil_at(const SilCtx &c, int view, int cam, int i, int j)
{
    const int row = c.S - 1 - j, col = c.S - 1 - i;
    const int cs = (c.flip && cam == 2) ? c.S - 1 - col : col;
    return ((size_t)view * c.S + row) * c.S + cs;
}

// forward: one wavefront per 8 x 8 tile of mirrored pixel indices, four tiles per workgroup; blockIdx.y: the view
__global__ __launch_bounds__(256) void k_sil_tile(SilCtx c)
{
    const int lane = threadIdx.x & 63;
    const int T = (c.S + 7) >> 3;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int view = blockIdx.y, cam = (c.cams >> (2 * view)) & 3;
    if (tile >= T * T) return;                                             // the whole wavefront
    const int tj = tile / T, ti = tile - tj * T;
    const uint32_t ilo = (uint32_t)ti * 8, jlo = (uint32_t)tj * 8;
    const int i = (int)ilo + (lane & 7), j = (int)jlo + (lane >> 3);
    const float px = sil_centre(i, c.S), py = sil_centre(j, c.S);
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
    if (i < c.S && j < c.S) c.alpha_out[sil_at(c, view, cam, i, j)] = 1.0f - prod;
}

// backward: kSilLanes lanes per face, 256 / kSilLanes faces per workgroup; blockIdx.y: the view.  Writes the face's six partials
// (zeros for a face that draws nothing) to cg[view][3 f + corner][X, Y]
__global__ __launch_bounds__(256) void k_sil_bwd(SilCtx c)
{
    const int64_t f = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kSilLanes;
    const int sub = threadIdx.x % kSilLanes;
    const int view = blockIdx.y, cam = (c.cams >> (2 * view)) & 3;
    if (f >= c.F) return;                                                  // whole groups of kSilLanes lanes
    const size_t at = (size_t)view * c.F + f;
    const SilBox b = c.box[at];
    const int i0 = (int)(b.i & 0xffffu), i1 = (int)(b.i >> 16), j0 = (int)(b.j & 0xffffu), j1 = (int)(b.j >> 16);
    float g[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };                   // X0 Y0 X1 Y1 X2 Y2
    if (i0 <= i1 && j0 <= j1 && i1 < c.S && j1 < c.S) {                    // what k_sil_pre wrote passes; nothing else is an address
        const SilRec r = c.rec[at];
        const int w = i1 - i0 + 1, n = w * (j1 - j0 + 1);                  // <= S^2 <= 2^22
        int j = sub / w, i = sub - j * w;
        for (int t = sub; t < n; t += kSilLanes) {
            const size_t pix = sil_at(c, view, cam, i0 + i, j0 + j);
            const float k = c.grad_alpha[pix] * (1.0f - c.alpha[pix]);
            SilHit h;
            if (k != 0.0f && sil_eval(r, sil_centre(i0 + i, c.S), sil_centre(j0 + j, c.S), h)) {
                const float dm = (-(k * h.prob) / kSilSigma) * h.sgn;      // d loss / d m of this pair
                const float ca = (-2.0f * (1.0f - h.t)) * dm, cb = (-2.0f * h.t) * dm;
                const float c0 = h.edge == 2 ? 0.0f : ca, c1 = h.edge == 0 ? cb : (h.edge == 2 ? ca : 0.0f), c2 = h.edge == 0 ? 0.0f : cb;
                g[0] += c0 * h.ex; g[1] += c0 * h.ey; g[2] += c1 * h.ex; g[3] += c1 * h.ey; g[4] += c2 * h.ex; g[5] += c2 * h.ey;
            }
            i += kSilLanes;
            while (i >= w) { i -= w; ++j; }
        }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {                                          // lane order: the same sum every run
        float s = 0.0f;
        for (int l = 0; l < kSilLanes; ++l) s += __shfl(g[q], l, kSilLanes);
        g[q] = s;
    }
    if (sub == 0) {
        float *o = c.cg + ((size_t)view * 3 * c.F + 3 * f) * 2;
#pragma unroll
        for (int q = 0; q < 6; ++q) o[q] = g[q];
    }
}

// the addends of incidence key 3 f + corner in view `pass`: (d/dX, d/dY) of that corner taken back to the world's x, y, z - the
// coordinate along the view's axis gets nothing
struct SilTerm {
    const float *cg; int64_t F; int cams;
    __device__ void operator()(int pass, int key, float o[3]) const
    {
        o[0] = o[1] = o[2] = 0.0f;
        if (key < 0 || key / 3 >= F) return;
        const float *g = cg + ((size_t)pass * 3 * F + key) * 2;
        const int cam = (cams >> (2 * pass)) & 3;
        const float gx = (cam == 0 || cam == 3) ? -g[0] : g[0];            // X = -x, +z, +x, -z for cam 0..3
        if (cam & 1) o[2] = gx; else o[0] = gx;
        o[1] = g[1];
    }
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

struct SilLayout { size_t hdr, deg, cur, zero_end, loc, part, inc, tmp, longv, rec, box, cg, total; };

SilLayout sil_layout(int64_t V, int64_t F, int n_views)
{
    SilLayout L{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = (o + bytes + 255) / 256 * 256; return at; };
    L.hdr = take(sizeof(SilHdr)); L.deg = take((size_t)V * 4); L.cur = take((size_t)V * 4);
    L.zero_end = o;                                                        // [0, zero_end): cleared by k_sil_clear
    L.loc = take((size_t)V * 4); L.part = take((size_t)((V + kScanItems - 1) / kScanItems) * 4);
    L.inc = take((size_t)F * 12); L.tmp = take((size_t)F * 12); L.longv = take((size_t)V * 4);
    L.rec = take((size_t)F * n_views * sizeof(SilRec)); L.box = take((size_t)F * n_views * sizeof(SilBox));
    L.cg = take((size_t)F * n_views * 24);
    L.total = o;
    return L;
}

int sil_check_sizes(int64_t V, int64_t F, int size, int n_views)
{
    ICON_ARG(V > 0 && F > 0 && V < (1ll << 31) && F < (1ll << 29), "icon_silhouette: 0 < V < 2^31, 0 < F < 2^29");
    ICON_ARG(size >= 8 && size <= 2048, "icon_silhouette: size must be 8..2048");
    ICON_ARG(n_views >= 1 && n_views <= 4, "icon_silhouette: n_views must be 1..4");
    return ICON_OK;
}

// the checks both directions share, and the context over the caller's scratch
int sil_context(const float *d_verts, int64_t V, const void *d_faces, int64_t F, const int *cam_ids, int n_views, int size,
                void *d_scratch, int64_t scratch_bytes, SilCtx &c, SilLayout &L)
{
    ICON_ARG(d_verts && d_faces && cam_ids && d_scratch, "icon_silhouette: null argument");
    const int rc = sil_check_sizes(V, F, size, n_views);
    if (rc) return rc;
    int cams = 0;
    for (int k = 0; k < n_views; ++k) {
        ICON_ARG(cam_ids[k] >= 0 && cam_ids[k] <= 3, "icon_silhouette: cam_ids must be 0..3");
        cams |= cam_ids[k] << (2 * k);
    }
    ICON_ARG(((uintptr_t)d_scratch & 255) == 0, "icon_silhouette: the scratch must be 256-byte aligned");
    L = sil_layout(V, F, n_views);
    ICON_ARG(scratch_bytes >= (int64_t)L.total, "icon_silhouette: scratch smaller than icon_silhouette_bytes");
    char *s = static_cast<char *>(d_scratch);
    c = SilCtx{};
    c.verts = d_verts; c.faces = d_faces; c.V = V; c.F = F; c.S = size; c.n_views = n_views; c.cams = cams; c.flip = n_views == 2 ? 1 : 0;
    c.hdr = reinterpret_cast<SilHdr *>(s + L.hdr); c.bad_faces = &c.hdr->bad_faces; c.n_long = &c.hdr->n_long;
    c.deg = reinterpret_cast<int *>(s + L.deg); c.cur = reinterpret_cast<int *>(s + L.cur);
    c.loc = reinterpret_cast<int *>(s + L.loc); c.part = reinterpret_cast<int *>(s + L.part);
    c.inc = reinterpret_cast<int *>(s + L.inc); c.tmp = reinterpret_cast<int *>(s + L.tmp); c.longv = reinterpret_cast<int *>(s + L.longv);
    c.rec = reinterpret_cast<SilRec *>(s + L.rec); c.box = reinterpret_cast<SilBox *>(s + L.box); c.cg = reinterpret_cast<float *>(s + L.cg);
    return ICON_OK;
}

void sil_clear(const SilLayout &L, void *d_scratch, hipStream_t st)
{
    const size_t n = L.zero_end / 4;
    hipLaunchKernelGGL(k_sil_clear, dim3((unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), dim3(256), 0, st,
                       static_cast<uint32_t *>(d_scratch), n);
}

template <class IT>
void sil_backward_launch(const SilCtx &c, hipStream_t st)
{
    const unsigned gF = (unsigned)((c.F + 255) / 256), gV = (unsigned)((c.V + 255) / 256);
    const int nb = (int)((c.V + kScanItems - 1) / kScanItems);
    hipLaunchKernelGGL(k_sil_pre<IT>, dim3(gF, (unsigned)c.n_views), dim3(256), 0, st, c);
    hipLaunchKernelGGL(k_sil_bwd, dim3((unsigned)((c.F * kSilLanes + 255) / 256), (unsigned)c.n_views), dim3(256), 0, st, c);
    const S1Ctx &s1 = c;                                                   // the shared kernels take the base alone
    hipLaunchKernelGGL(k_s1_count<IT>, dim3(gF), dim3(256), 0, st, s1);
    hipLaunchKernelGGL(k_s1_scan_blocks, dim3((unsigned)nb), dim3(256), 0, st, s1);
    hipLaunchKernelGGL(k_s1_scan_parts, dim3(1), dim3(1024), 0, st, s1, nb);
    hipLaunchKernelGGL(k_s1_fill<IT>, dim3(gF), dim3(256), 0, st, s1);
    const SilTerm term{c.cg, c.F, c.cams};
    hipLaunchKernelGGL(k_sil_vertex, dim3(gV), dim3(256), 0, st, c, term);
    hipLaunchKernelGGL((k_s1_sum_long<SilTerm, SilStore>), dim3(kLongGrid), dim3(64), 0, st, s1, c.n_views, term, SilStore{c.grad_verts});
}

}  // namespace
}  // namespace icon

using namespace icon;

extern "C" int icon_silhouette_bytes(int64_t V, int64_t F, int size, int n_views, int64_t *bytes)
{
    ICON_ARG(bytes != nullptr, "icon_silhouette_bytes: null argument");
    const int rc = sil_check_sizes(V, F, size, n_views);
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
    SilLayout L;
    const int rc = sil_context(d_verts, V, d_faces, F, cam_ids, n_views, size, d_scratch, scratch_bytes, c, L);
    if (rc) return rc;
    c.alpha_out = d_alpha; c.count_bad = 1;
    hipStream_t st = (hipStream_t)stream;
    sil_clear(L, d_scratch, st);
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
    SilLayout L;
    const int rc = sil_context(d_verts, V, d_faces, F, cam_ids, n_views, size, d_scratch, scratch_bytes, c, L);
    if (rc) return rc;
    c.alpha = d_alpha; c.grad_alpha = d_grad_alpha; c.grad_verts = d_grad_verts; c.count_bad = 0;   // k_s1_count counts the bad faces here
    hipStream_t st = (hipStream_t)stream;
    sil_clear(L, d_scratch, st);
    if (faces_int64) sil_backward_launch<int64_t>(c, st); else sil_backward_launch<int32_t>(c, st);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

// render_normal_bwd.hip - the gradient of the normal maps of render_normal.hip with respect to the vertices (lib/common/render.py
// Render.get_rgb_image as the two optimisation loops of apps/infer.py differentiate it: :200-217 losses["normal"], :448-456
// losses["cloth"]; pytorch3d: TexturesVertex(verts_normals_padded()) interpolated by differentiable barycentrics).
//
// The rule (PARITY UNPINNED like 4.13): the forward rule is 4.13's - per channel the winner's
//   colour = sum_k b_k n_k + (sum_k b_k - 1),   b_k = c_k / max((c0 + c1) + c2, 1e-5),   c_k = clamp(w_k, 0, 1),   w_k = ef_k / (area + 1e-8).
// Winner, candidate set and clamp pattern are piecewise constant and carry no gradient; pix_to_face (as icon_render_normal wrote
// it) says which face owns a pixel.  Two paths:
//   1. barycentrics: d colour / d b_k = n_k + 1; b -> c passes through max(.., 1e-5) only where the sum exceeds 1e-5; c -> w only
//      where 0 < w_k < 1; w -> the NDC X, Y of the face's three corners (ef and area) -> world (X = -x, +z, +x, -z for cam 0..3, Y = y).
//   2. normals: d colour / d n_k = b_k; n = N / max(|N|, 1e-6): gN = (g - n (n . g)) / |N| where |N| > 1e-6, else g 1e6; N_v is the
//      S1 sum of (v1 - v0) x (v2 - v0) over the incident faces: a face's normal gets gN[v0] + gN[v1] + gN[v2], which goes back
//      through the cross product to its corners.  World-space, the same for every view: the views add up, and no coordinate is left out.
//
// Shape of the work: one stream-ordered call of kernel launches over the caller's scratch; nothing is allocated, read back or
// waited for; the clears are a kernel of the call's own.  The expressions of the per-pixel rule - projection, ef, den, the clipped box,
// the clamped barycentrics, the pixel address, the sweeps and the deferred list - are raster_device.h's, the very functions of render_normal.hip.
//   clear, count / scan / fill (s1_normals_device.h): one incidence list serves the normals and both gathers
//   N_v: the un-normalised S1 sums into the scratch - the forward's values recomputed, the same bytes
//   k_rnb_face: per (view, face) sweep the face's clipped pixel box, take the pixels pix_to_face gives to this face, accumulate
//     9 partials sum b_k g_c, 6 of d/dX, d/dY of the corners through the ef terms and 1 of d/d den (applied to the corners after
//     the sweep: its coefficients are the face's), add across the lanes by a fixed tree, write the per-corner record.  One thread per
//     face, eight lanes per face (the forward's choice, the forward's debug option) or, for a box above 64 pixels per lane, the
//     deferred list: k_rnb_face_big, one workgroup per entry with a fixed reduction tree
//   gather A: per vertex the normal-path terms of its corners, view by view in ascending 3 face + corner order, then the
//     normalisation backwards with N_v -> gN[v]
//   face pass: g_FN and its cross products per corner
//   gather B: per vertex the face-pass terms, then view by view the path-1 terms on the world's axes -> grad_verts
// No floating-point atomics anywhere: the order of every addition is fixed by keys (pixel index, lane, 3 face + corner, view) -
// equal bytes from run to run and from int32 and int64 faces.  Every index taken out of the scratch is range-checked before it is
// an address; pix_to_face is only ever COMPARED with a face id, never used as an address.
#pragma clang fp contract(off)

#include "raster_device.h"

namespace icon {
namespace {

constexpr int kRnbAcc = 16;           // 9: sum b_k g_c; 6: X0 Y0 X1 Y1 X2 Y2 through the ef terms; 1: d / d den

struct RnbCtx : RsCtx {
    int *n_big, *big;                // the deferred list (raster_device.h) [n_views F] and its length in the header
    float *Nv;                       // [V][3] un-normalised S1 sums
    float *gNv;                      // [V][3] d loss / d N_v
    float *gn;                       // [n_views][3 F][3] per corner: sum over the face's pixels of b_k g_c
    float *gxy;                      // [n_views][3 F][2] per corner: d loss / d (X, Y) through path 1
    float *fc;                       // [3 F][3] per corner: the normal path taken back through the face's cross product
    const int32_t *pix;              // [n_views][S][S]
    const float *gimg;               // [n_views][3][S][S]
    float *grad_verts;               // [V][3]
};

struct RnbFace {
    float X[3], Y[3], den;
    RsBox box;
    int64_t id[3];
};

// face f as camera `cam` sees it: the forward's projection, area, den and clipped box.  false: the forward drew nothing of it
template <class IT>
__device__ __forceinline__ bool rnb_setup(const RnbCtx &c, int cam, int64_t f, RnbFace &r)
{
    if (!s1_face<IT>(c, f, r.id)) return false;
    float D[3];                                                            // never read: no depth here
    rs_project(c, cam, r.id, r.X, r.Y, D);
    const float area = rs_area(r.X, r.Y);
    if (!rs_drawn(area)) return false;
    r.den = area + kRsEps;
    r.box = rs_box(rs_bounds(r.X, r.Y, kRsNormalBlurR), c.S);
    return !r.box.empty();
}

// the S1 normals of the face's corners, as the forward's RnStore left them: N / max(|N|, 1e-6)
__device__ __forceinline__ void rnb_normals(const RnbCtx &c, const RnbFace &r, float nrm[9])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float *N = c.Nv + 3 * r.id[k];
        float x = N[0], y = N[1], z = N[2];
        s1_normalise(x, y, z);
        nrm[3 * k] = x; nrm[3 * k + 1] = y; nrm[3 * k + 2] = z;
    }
}

// mirrored pixel (i, j) of view `view`, both in [0, S): if pix_to_face gives it to face f and its gradient is not zero, its terms into a[]
__device__ __forceinline__ void rnb_pixel(const RnbCtx &c, const RnbFace &r, const float nrm[9], int view, int cam, int64_t f, int i, int j,
                                          float a[kRnbAcc])
{
    const size_t plane = (size_t)c.S * c.S, at = rs_at(c, cam, i, j);
    if ((int64_t)c.pix[(size_t)view * plane + at] != f) return;
    const float *gp = c.gimg + (size_t)view * 3 * plane + at;
    const float g0 = gp[0], g1 = gp[plane], g2 = gp[2 * plane];
    if (g0 == 0.0f && g1 == 0.0f && g2 == 0.0f) return;
    const float px = rs_centre(i, c.S), py = rs_centre(j, c.S);
    float w[3];
    rs_weights(r.X, r.Y, r.den, px, py, w);
    const RsBary q = rs_bary(w);
    const float w0 = w[0], w1 = w[1], w2 = w[2], b0 = q.b[0], b1 = q.b[1], b2 = q.b[2], s = q.s;
    // path 2: d loss / d n_k = b_k g
    a[0] += b0 * g0; a[1] += b0 * g1; a[2] += b0 * g2;
    a[3] += b1 * g0; a[4] += b1 * g1; a[5] += b1 * g2;
    a[6] += b2 * g0; a[7] += b2 * g1; a[8] += b2 * g2;
    // path 1: d loss / d b_k = sum_c g_c (n_kc + 1), back to c_k, w_k
    const float B0 = (g0 * (nrm[0] + 1.0f) + g1 * (nrm[1] + 1.0f)) + g2 * (nrm[2] + 1.0f);
    const float B1 = (g0 * (nrm[3] + 1.0f) + g1 * (nrm[4] + 1.0f)) + g2 * (nrm[5] + 1.0f);
    const float B2 = (g0 * (nrm[6] + 1.0f) + g1 * (nrm[7] + 1.0f)) + g2 * (nrm[8] + 1.0f);
    const float dot = q.sraw > kRsMinSum ? (B0 * b0 + B1 * b1) + B2 * b2 : 0.0f;   // the max passes gradient only where the sum exceeds it
    const float W0 = (w0 > 0.0f && w0 < 1.0f) ? (B0 - dot) / s : 0.0f;        // the clamp only where 0 < w_k < 1
    const float W1 = (w1 > 0.0f && w1 < 1.0f) ? (B1 - dot) / s : 0.0f;
    const float W2 = (w2 > 0.0f && w2 < 1.0f) ? (B2 - dot) / s : 0.0f;
    const float E0 = W0 / r.den, E1 = W1 / r.den, E2 = W2 / r.den;            // d loss / d ef_k
    a[15] += -((W0 * w0 + W1 * w1) + W2 * w2) / r.den;                        // d loss / d den
    // ef(p; a, b): d/d ax = py - by, d/d bx = -(py - ay), d/d ay = bx - px, d/d by = px - ax.  ef_0: (v1, v2), ef_1: (v2, v0), ef_2: (v0, v1)
    a[9] += E2 * (py - r.Y[1]) - E1 * (py - r.Y[2]);                           // X0
    a[10] += E2 * (r.X[1] - px) + E1 * (px - r.X[2]);                          // Y0
    a[11] += E0 * (py - r.Y[2]) - E2 * (py - r.Y[0]);                          // X1
    a[12] += E0 * (r.X[2] - px) + E2 * (px - r.X[0]);                          // Y1
    a[13] += E1 * (py - r.Y[0]) - E0 * (py - r.Y[1]);                          // X2
    a[14] += E1 * (r.X[0] - px) + E0 * (px - r.X[1]);                          // Y2
}

// the face's record: den = ef(v2; v0, v1) + eps is taken back to the corners here, once
__device__ __forceinline__ void rnb_write(const RnbCtx &c, const RnbFace &r, bool drawn, int view, int64_t f, const float a[kRnbAcc])
{
    float *on = c.gn + ((size_t)view * 3 * c.F + 3 * f) * 3;
    float *oxy = c.gxy + ((size_t)view * 3 * c.F + 3 * f) * 2;
#pragma unroll
    for (int q = 0; q < 9; ++q) on[q] = a[q];
    float x[6] = { a[9], a[10], a[11], a[12], a[13], a[14] };
    if (drawn) {
        const float gd = a[15];
        x[0] += gd * (r.Y[2] - r.Y[1]); x[1] += gd * (r.X[1] - r.X[2]);
        x[2] += -(gd * (r.Y[2] - r.Y[0])); x[3] += gd * (r.X[2] - r.X[0]);
        x[4] += gd * (r.Y[1] - r.Y[0]); x[5] += -(gd * (r.X[1] - r.X[0]));
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) oxy[q] = x[q];
}

// the un-normalised S1 sum into the scratch
struct RnbStoreN {
    float *Nv;
    __device__ void operator()(int64_t v, float x, float y, float z) const { Nv[3 * v] = x; Nv[3 * v + 1] = y; Nv[3 * v + 2] = z; }
};

// one thread per vertex: N_v of a short incidence list; a long one goes to the long list, which every later gather walks too
template <class IT>
__global__ __launch_bounds__(256) void k_rnb_normals(RnbCtx c)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= c.V) return;
    const int n = c.deg[v];
    if (n > kShort) { s1_defer_long(c, v); return; }
    float s[3];
    s1_sum_short<IT>(c, v, n, s);
    RnbStoreN{c.Nv}(v, s[0], s[1], s[2]);
}

// G lanes per face, 256 / G faces per workgroup; blockIdx.y: the view.  Every (view, face) gets its record written (zeros for a
// face that draws nothing and for a deferred one, whose record k_rnb_face_big then overwrites)
template <class IT, int G>
__global__ __launch_bounds__(256) void k_rnb_face(RnbCtx c)
{
    const int64_t f = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x % G;
    const int view = blockIdx.y, cam = c.cam(view);
    if (f >= c.F) return;                                                  // whole groups of G lanes
    RnbFace r;
    float a[kRnbAcc];
#pragma unroll
    for (int q = 0; q < kRnbAcc; ++q) a[q] = 0.0f;
    const bool drawn = rnb_setup<IT>(c, cam, f, r);
    const bool big = drawn && r.box.n() > kRsBigPerLane * G;
    if (big) {
        if (sub == 0) rs_defer(c, c.n_big, c.big, view, f);
    } else if (drawn) {
        float nrm[9];
        rnb_normals(c, r, nrm);
        rs_sweep<G>(r.box, sub, [&](int i, int j) { rnb_pixel(c, r, nrm, view, cam, f, i, j, a); });
    }
    if (G > 1) {
#pragma unroll
        for (int q = 0; q < kRnbAcc; ++q) {                                // a fixed tree over the G lanes: the same sum every run
            float s = a[q];
            for (int d = G / 2; d >= 1; d >>= 1) s += __shfl_down(s, d, G);
            a[q] = s;                                                      // complete in lane 0 of the group
        }
    }
    if (sub == 0) rnb_write(c, r, drawn && !big, view, f, a);
}

// the deferred faces: a workgroup per entry, as many rounds as the list (read from device memory) needs.  Thread t takes pixels
// t, t + 256, ...; the 256 partial sums are added by a fixed tree (inside a wavefront by halving distances, then the four wavefronts in order)
template <class IT>
__global__ __launch_bounds__(256) void k_rnb_face_big(RnbCtx c)
{
    __shared__ float s_part[4][kRnbAcc];
    const int nb = rs_deferred_count(c, c.n_big);
    for (int e = blockIdx.x; e < nb; e += gridDim.x) {                     // uniform over the workgroup
        int view;
        int64_t f;
        if (!rs_deferred(c, c.big, e, view, f)) continue;
        const int cam = c.cam(view);
        RnbFace r;
        if (!rnb_setup<IT>(c, cam, f, r)) continue;
        float nrm[9], a[kRnbAcc];
        rnb_normals(c, r, nrm);
#pragma unroll
        for (int q = 0; q < kRnbAcc; ++q) a[q] = 0.0f;
        rs_sweep_block(r.box, [&](int i, int j) { rnb_pixel(c, r, nrm, view, cam, f, i, j, a); });
#pragma unroll
        for (int q = 0; q < kRnbAcc; ++q) {
            float s = a[q];
            for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d);
            a[q] = s;
        }
        __syncthreads();                                                   // the previous entry's s_part has been read
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int q = 0; q < kRnbAcc; ++q) s_part[threadIdx.x >> 6][q] = a[q];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int q = 0; q < kRnbAcc; ++q) a[q] = ((s_part[0][q] + s_part[1][q]) + s_part[2][q]) + s_part[3][q];
            rnb_write(c, r, true, view, f, a);
        }
    }
}

// gather A.  The addends of incidence key 3 f + corner in view `pass`: that corner's sum of b_k g_c
struct RnbTermA {
    const float *gn; int64_t F;
    __device__ void operator()(int pass, int key, float o[3]) const
    {
        o[0] = o[1] = o[2] = 0.0f;
        if (key < 0 || key / 3 >= F) return;
        const float *g = gn + ((size_t)pass * 3 * F + key) * 3;
        o[0] = g[0]; o[1] = g[1]; o[2] = g[2];
    }
};
// ... and the normalisation backwards: n = N / max(|N|, 1e-6) with s1_normalise's length
struct RnbStoreA {
    const float *Nv; float *gNv;
    __device__ void operator()(int64_t v, float gx, float gy, float gz) const
    {
        const float x = Nv[3 * v], y = Nv[3 * v + 1], z = Nv[3 * v + 2];
        const float len = sqrtf(fmaf(z, z, fmaf(y, y, x * x)));
        float ox, oy, oz;
        if (len > 1e-6f) {
            const float nx = x / len, ny = y / len, nz = z / len;
            const float d = (nx * gx + ny * gy) + nz * gz;
            ox = (gx - nx * d) / len; oy = (gy - ny * d) / len; oz = (gz - nz * d) / len;
        } else {
            ox = gx * 1e6f; oy = gy * 1e6f; oz = gz * 1e6f;
        }
        gNv[3 * v] = ox; gNv[3 * v + 1] = oy; gNv[3 * v + 2] = oz;
    }
};

// gather B.  Pass 0: the corner's term of the face pass; pass 1 + view: (d/dX, d/dY) of that corner taken back to the world's axes
struct RnbTermB {
    const float *fc, *gxy; int64_t F; int cams;
    __device__ void operator()(int pass, int key, float o[3]) const
    {
        if (pass == 0) {
            o[0] = o[1] = o[2] = 0.0f;
            if (key < 0 || key / 3 >= F) return;
            const float *g = fc + (size_t)key * 3;
            o[0] = g[0]; o[1] = g[1]; o[2] = g[2];
            return;
        }
        rs_world_term(gxy, F, cams, pass - 1, key, o);
    }
};
struct RnbStoreB {
    float *out;
    __device__ void operator()(int64_t v, float x, float y, float z) const { out[3 * v] = x; out[3 * v + 1] = y; out[3 * v + 2] = z; }
};

// one thread per vertex: the ordered sum of a short incidence list (a vertex of no good face: 0); the long ones are k_s1_sum_long's,
// from the list k_rnb_normals made
template <class Term, class Store>
__global__ __launch_bounds__(256) void k_rnb_vertex(RnbCtx c, int passes, Term term, Store store)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= c.V) return;
    const int n = c.deg[v];
    if (n > kShort) return;
    float s[3];
    s1_sum_short_terms(c, v, n, passes, term, s);
    store(v, s[0], s[1], s[2]);
}

// one thread per face: g_FN = (gN[v0] + gN[v1]) + gN[v2] through FN = u x w, u = v1 - v0, w = v2 - v0
template <class IT>
__global__ __launch_bounds__(256) void k_rnb_face_pass(RnbCtx c)
{
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= c.F) return;
    float o[9] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    int64_t id[3];
    if (s1_face<IT>(c, f, id)) {
        const float *p0 = c.verts + 3 * id[0], *p1 = c.verts + 3 * id[1], *p2 = c.verts + 3 * id[2];
        const float *a0 = c.gNv + 3 * id[0], *a1 = c.gNv + 3 * id[1], *a2 = c.gNv + 3 * id[2];
        const float gx = (a0[0] + a1[0]) + a2[0], gy = (a0[1] + a1[1]) + a2[1], gz = (a0[2] + a1[2]) + a2[2];
        const float ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
        const float wx = p2[0] - p0[0], wy = p2[1] - p0[1], wz = p2[2] - p0[2];
        o[3] = wy * gz - wz * gy; o[4] = wz * gx - wx * gz; o[5] = wx * gy - wy * gx;      // g_v1 = w x g_FN
        o[6] = gy * uz - gz * uy; o[7] = gz * ux - gx * uz; o[8] = gx * uy - gy * ux;      // g_v2 = g_FN x u
        o[0] = -(o[3] + o[6]); o[1] = -(o[4] + o[7]); o[2] = -(o[5] + o[8]);               // g_v0 = -(g_v1 + g_v2)
        // a face that repeats a vertex (FN is exactly 0 then): the vertex's two corners are added HERE, where they cancel exactly -
        // taken apart into the vertex's ordered sum, s + a - a would leave a rounding residue of a face that contributes nothing
        if (id[0] == id[1]) { o[0] += o[3]; o[1] += o[4]; o[2] += o[5]; o[3] = o[4] = o[5] = 0.0f; }
        if (id[0] == id[2]) { o[0] += o[6]; o[1] += o[7]; o[2] += o[8]; o[6] = o[7] = o[8] = 0.0f; }
        else if (id[1] == id[2]) { o[3] += o[6]; o[4] += o[7]; o[5] += o[8]; o[6] = o[7] = o[8] = 0.0f; }
    }
    float *out = c.fc + (size_t)f * 9;
#pragma unroll
    for (int q = 0; q < 9; ++q) out[q] = o[q];
}

struct RnbLayout { S1Layout s1; size_t big, Nv, gNv, gn, gxy, fc, total; };

RnbLayout rnb_layout(int64_t V, int64_t F, int n_views)
{
    RnbLayout L{};
    ScratchTake take;
    L.s1 = s1_layout(take, V, F);
    L.big = take((size_t)F * 4 * n_views);
    L.Nv = take((size_t)V * 12); L.gNv = take((size_t)V * 12);
    L.gn = take((size_t)F * n_views * 36); L.gxy = take((size_t)F * n_views * 24); L.fc = take((size_t)F * 36);
    L.total = take.o;
    return L;
}

template <class IT>
void rnb_launch(const RnbCtx &c, hipStream_t st)
{
    const unsigned gF = (unsigned)((c.F + 255) / 256), gV = (unsigned)((c.V + 255) / 256);
    const S1Ctx &s1 = c;                                                   // the shared kernels take the base alone
    s1_launch_lists<IT>(s1, st);
    hipLaunchKernelGGL(k_rnb_normals<IT>, dim3(gV), dim3(256), 0, st, c);
    hipLaunchKernelGGL((k_s1_normals_long<IT, RnbStoreN>), dim3(kLongGrid), dim3(64), 0, st, s1, RnbStoreN{c.Nv});
    const dim3 gR((unsigned)((c.F * rs_lanes(c) + 255) / 256), (unsigned)c.n_views);   // the forward's mapping
    if (rs_lanes(c) == 1) hipLaunchKernelGGL((k_rnb_face<IT, 1>), gR, dim3(256), 0, st, c);
    else hipLaunchKernelGGL((k_rnb_face<IT, 8>), gR, dim3(256), 0, st, c);
    hipLaunchKernelGGL(k_rnb_face_big<IT>, dim3(kRsBigGrid), dim3(256), 0, st, c);
    const RnbTermA ta{c.gn, c.F};
    const RnbStoreA sa{c.Nv, c.gNv};
    hipLaunchKernelGGL((k_rnb_vertex<RnbTermA, RnbStoreA>), dim3(gV), dim3(256), 0, st, c, c.n_views, ta, sa);
    hipLaunchKernelGGL((k_s1_sum_long<RnbTermA, RnbStoreA>), dim3(kLongGrid), dim3(64), 0, st, s1, c.n_views, ta, sa);
    hipLaunchKernelGGL(k_rnb_face_pass<IT>, dim3(gF), dim3(256), 0, st, c);
    const RnbTermB tb{c.fc, c.gxy, c.F, c.cams};
    const RnbStoreB sb{c.grad_verts};
    hipLaunchKernelGGL((k_rnb_vertex<RnbTermB, RnbStoreB>), dim3(gV), dim3(256), 0, st, c, 1 + c.n_views, tb, sb);
    hipLaunchKernelGGL((k_s1_sum_long<RnbTermB, RnbStoreB>), dim3(kLongGrid), dim3(64), 0, st, s1, 1 + c.n_views, tb, sb);
}

}  // namespace
}  // namespace icon

using namespace icon;

extern "C" int icon_render_normal_backward_bytes(int64_t V, int64_t F, int size, int n_views, int64_t *bytes)
{
    ICON_ARG(bytes != nullptr, "icon_render_normal_backward_bytes: null argument");
    const int rc = rs_check_sizes("icon_render_normal_backward", V, F, size, n_views);
    if (rc) return rc;
    *bytes = (int64_t)rnb_layout(V, F, n_views).total;
    return ICON_OK;
}

extern "C" int icon_render_normal_backward(const float *d_verts, int64_t V, const void *d_faces, int64_t F, int faces_int64,
                                           const int *cam_ids, int n_views, int size, const int32_t *d_pix_to_face,
                                           const float *d_grad_images, float *d_grad_verts,
                                           void *d_scratch, int64_t scratch_bytes, void *stream)
{
    ICON_ARG(d_verts && d_faces && cam_ids && d_pix_to_face && d_grad_images && d_grad_verts && d_scratch, "icon_render_normal_backward: null argument");
    const RnbLayout L = rnb_layout(V, F, n_views);
    RnbCtx c{};
    const int rc = rs_context("icon_render_normal_backward", "icon_render_normal_backward_bytes", d_verts, V, d_faces, F, cam_ids, n_views, size,
                              d_scratch, scratch_bytes, L.total, c);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    char *s = static_cast<char *>(d_scratch);
    c.pix = d_pix_to_face; c.gimg = d_grad_images; c.grad_verts = d_grad_verts;
    c.n_big = &s1_bind(c, s, L.s1)->n_big; c.big = reinterpret_cast<int *>(s + L.big);
    c.Nv = reinterpret_cast<float *>(s + L.Nv); c.gNv = reinterpret_cast<float *>(s + L.gNv);
    c.gn = reinterpret_cast<float *>(s + L.gn); c.gxy = reinterpret_cast<float *>(s + L.gxy); c.fc = reinterpret_cast<float *>(s + L.fc);
    rs_clear(s, L.s1, nullptr, 0, st);
    if (faces_int64) rnb_launch<int64_t>(c, st); else rnb_launch<int32_t>(c, st);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

// cloth.hip - the cloth refinement step of apps/infer.py:405-476 without the renderer: the LocalAffine deformation with its
// stiffness and rigidity means (lib/net/local_affine.py) and the three mesh shape priors of update_mesh_shape_prior_losses
// (lib/dataset/mesh_util.py:63-106, :168-176: edge length, normal consistency, uniform Laplacian), forwards and backwards.
// The rule is DESIGN.md 4.16 (PARITY UNPINNED): every expression is evaluated in float64 from the float32 inputs and rounded to
// float32 once, where it is stored.
//
// Shape of every call: one lane per item (vertex, edge, face pair - the three lists share one launch), no floating-point
// atomics.  A scalar is summed per wave (shuffles), per workgroup (LDS), and a second one-workgroup kernel adds the workgroups'
// partials in a fixed order.  A per-vertex gradient is a GATHER over that vertex's CSR row in the row's order: the neighbour
// row for the stiffness, edge and Laplacian terms; for the normal consistency the pass before stores each pair's four
// gradients once ([P,4,3] float32) and the vertex sums its row of the vertex -> (pair, slot) incidence list.  Topology arrays
// are the caller's (icon_amd/cloth.py: ClothTopology), int32 or int64, read in place; an entry that names nothing is skipped,
// so no index is ever used as an address unchecked.
#include "common.h"

namespace icon {
namespace {

constexpr int kClBlock = 256;
constexpr double kCosEps = 1e-8;         // torch.cosine_similarity's eps: each norm is clamped from below before the division

template <class IT>
__device__ __forceinline__ bool in_range(IT j, int64_t n) { return (uint64_t)(int64_t)j < (uint64_t)n; }

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 ld3(const float *p) { return D3{(double)p[0], (double)p[1], (double)p[2]}; }
__device__ __forceinline__ D3 sub(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 add(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 mul(D3 a, double s) { return D3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ D3 quot(D3 a, double s) { return D3{a.x / s, a.y / s, a.z / s}; }   // a true division: v / |v| of an axis vector is exact
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ void st3(float *p, D3 a) { p[0] = (float)a.x; p[1] = (float)a.y; p[2] = (float)a.z; }

// sums v[0..N) over the workgroup: shuffles inside a wave, LDS across the four waves; the result is thread 0's
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double *lds)
{
#pragma unroll
    for (int k = 0; k < N; ++k)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0)
        for (int k = 0; k < N; ++k) lds[w * N + k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < N; ++k) v[k] = ((lds[k] + lds[N + k]) + lds[2 * N + k]) + lds[3 * N + k];
}

// the workgroups' partials, N per workgroup: thread t adds those of workgroups t, t + 256, ... in that order, then block_sum
template <int N>
__device__ __forceinline__ void partial_sum(const double *part, int n_wg, double (&v)[N], double *lds)
{
    for (int k = 0; k < N; ++k) v[k] = 0.0;
    for (int w = threadIdx.x; w < n_wg; w += kClBlock)
        for (int k = 0; k < N; ++k) v[k] += part[(size_t)w * N + k];
    block_sum<N>(v, lds);
}

// ---- LocalAffine ------------------------------------------------------------------------------------------------------------
struct LaCtx {
    const float *x, *A, *b;                 // [B,V,3], [B,V,3,3], [B,V,3,1]
    const void *edges;                      // [E,2]
    const void *nbr_off, *nbr;              // [V+1], [2E]: backward
    int64_t B, V, E;
    float *y, *stiff, *rigid;               // forward out
    const float *gy, *g_stiff, *g_rigid;    // backward in
    float *gA, *gb;                         // backward out
    double *part;                           // [n_wg][2]
    int n_wg;
};

struct Mat { double a[9]; };
__device__ __forceinline__ Mat ld9(const float *p)
{
    Mat m;
#pragma unroll
    for (int k = 0; k < 9; ++k) m.a[k] = (double)p[k];
    return m;
}
__device__ __forceinline__ double det3(const Mat &m)
{
    const double *a = m.a;
    return a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
}

template <class IT>
__global__ __launch_bounds__(kClBlock) void k_la_forward(LaCtx c)
{
    __shared__ double lds[8];
    const int64_t i = (int64_t)blockIdx.x * kClBlock + threadIdx.x;
    double acc[2] = {0.0, 0.0};                                            // stiffness, rigidity
    if (i < c.B * c.V) {
        const Mat m = ld9(c.A + i * 9);
        const D3 x = ld3(c.x + i * 3), b = ld3(c.b + i * 3);
        const double *a = m.a;
        st3(c.y + i * 3, D3{(a[0] * x.x + a[1] * x.y + a[2] * x.z) + b.x, (a[3] * x.x + a[4] * x.y + a[5] * x.z) + b.y,
                            (a[6] * x.x + a[7] * x.y + a[8] * x.z) + b.z});
        const double d = det3(m) - 1.0;
        acc[1] = d * d;
    }
    if (i < c.B * c.E) {
        const int64_t bb = i / c.E, e = i - bb * c.E;
        const IT *ed = static_cast<const IT *>(c.edges) + e * 2;
        const IT p = ed[0], q = ed[1];
        if (in_range(p, c.V) && in_range(q, c.V)) {
            const int64_t ip = bb * c.V + (int64_t)p, iq = bb * c.V + (int64_t)q;
            const float *Ap = c.A + ip * 9, *Aq = c.A + iq * 9, *bp = c.b + ip * 3, *bq = c.b + iq * 3;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) { const double d = (double)Ap[k] - (double)Aq[k]; s += d * d; }
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double d = (double)bp[k] - (double)bq[k]; s += d * d; }
            acc[0] = s;
        }
    }
    block_sum<2>(acc, lds);
    if (threadIdx.x == 0) { c.part[(size_t)blockIdx.x * 2] = acc[0]; c.part[(size_t)blockIdx.x * 2 + 1] = acc[1]; }
}

__global__ __launch_bounds__(kClBlock) void k_la_finish(LaCtx c)
{
    __shared__ double lds[8];
    double acc[2];
    partial_sum<2>(c.part, c.n_wg, acc, lds);
    if (threadIdx.x == 0) {
        *c.stiff = c.E > 0 ? (float)(acc[0] / ((double)c.B * (double)c.E * 12.0)) : 0.0f;
        *c.rigid = (float)(acc[1] / ((double)c.B * (double)c.V));
    }
}

// one lane per (mesh, vertex): grad A = gy x^T + g_rigid 2 (det - 1) / (B V) cof(A) + g_stiff 2 / (12 B E) sum over the neighbour
// row of (w_v - w_n), grad b = gy + the same sum's last column
template <class IT>
__global__ __launch_bounds__(kClBlock) void k_la_backward(LaCtx c)
{
    const int64_t i = (int64_t)blockIdx.x * kClBlock + threadIdx.x;
    if (i >= c.B * c.V) return;
    const int64_t bb = i / c.V, v = i - bb * c.V;
    const Mat m = ld9(c.A + i * 9);
    const D3 b = ld3(c.b + i * 3), x = ld3(c.x + i * 3), gy = ld3(c.gy + i * 3);
    const double *a = m.a;
    double sa[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, sb[3] = {0, 0, 0};
    if (c.E > 0) {
        const IT *off = static_cast<const IT *>(c.nbr_off), *nbr = static_cast<const IT *>(c.nbr);
        int64_t k0 = (int64_t)off[v], k1 = (int64_t)off[v + 1];
        if (k0 < 0) k0 = 0;
        if (k1 > 2 * c.E) k1 = 2 * c.E;
        for (int64_t k = k0; k < k1; ++k) {
            const IT n = nbr[k];
            if (!in_range(n, c.V)) continue;
            const float *An = c.A + (bb * c.V + (int64_t)n) * 9, *bn = c.b + (bb * c.V + (int64_t)n) * 3;
#pragma unroll
            for (int t = 0; t < 9; ++t) sa[t] += a[t] - (double)An[t];
            sb[0] += b.x - (double)bn[0]; sb[1] += b.y - (double)bn[1]; sb[2] += b.z - (double)bn[2];
        }
    }
    const double cs = c.E > 0 ? 2.0 * (double)*c.g_stiff / ((double)c.B * (double)c.E * 12.0) : 0.0;
    const double cr = 2.0 * (det3(m) - 1.0) * (double)*c.g_rigid / ((double)c.B * (double)c.V);
    const double cof[9] = {a[4] * a[8] - a[5] * a[7], -(a[3] * a[8] - a[5] * a[6]), a[3] * a[7] - a[4] * a[6],
                           -(a[1] * a[8] - a[2] * a[7]), a[0] * a[8] - a[2] * a[6], -(a[0] * a[7] - a[1] * a[6]),
                           a[1] * a[5] - a[2] * a[4], -(a[0] * a[5] - a[2] * a[3]), a[0] * a[4] - a[1] * a[3]};
    const double g[3] = {gy.x, gy.y, gy.z}, xs[3] = {x.x, x.y, x.z};
    float *gA = c.gA + i * 9, *gb = c.gb + i * 3;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int q = 0; q < 3; ++q) gA[r * 3 + q] = (float)(g[r] * xs[q] + cr * cof[r * 3 + q] + cs * sa[r * 3 + q]);
        gb[r] = (float)(g[r] + cs * sb[r]);
    }
}

// ---- the mesh shape priors --------------------------------------------------------------------------------------------------
constexpr int kTermEdge = 1, kTermNc = 2, kTermLap = 4;

struct MpCtx {
    const float *y;                          // [V,3]
    const void *edges, *nbr_off, *nbr;       // [E,2], [V+1], [2E]
    const void *pairs, *inc_off, *inc;       // [P,4] = (v0, v1, a, c); [V+1], [4P] entries pair * 4 + slot
    int64_t V, E, P;
    double target;
    int terms;
    float *o_edge, *o_nc, *o_lap;            // forward out
    const float *g_edge, *g_nc, *g_lap;      // backward in
    float *grad;                             // backward out [V,3]
    double *part;                            // [n_wg][3]
    double *W;                               // [V,3]: unit residual / max(deg, 1)
    float *GP;                               // [P,4,3]: d (1 - cos) / d (v0, v1, a, c)
    int n_wg;
};

// the uniform Laplacian's residual of vertex v: mean of the neighbour row - y_v (no neighbours: -y_v); -> the row's valid entries
template <class IT>
__device__ __forceinline__ int64_t lap_residual(const MpCtx &c, int64_t v, D3 &r)
{
    const IT *off = static_cast<const IT *>(c.nbr_off), *nbr = static_cast<const IT *>(c.nbr);
    int64_t k0 = (int64_t)off[v], k1 = (int64_t)off[v + 1];
    if (k0 < 0) k0 = 0;
    if (k1 > 2 * c.E) k1 = 2 * c.E;
    D3 s{0.0, 0.0, 0.0};
    int64_t deg = 0;                                                       // the entries that name a vertex: the others are skipped everywhere
    for (int64_t k = k0; k < k1; ++k) {
        const IT n = nbr[k];
        if (in_range(n, c.V)) { s = add(s, ld3(c.y + (int64_t)n * 3)); ++deg; }
    }
    const D3 yv = ld3(c.y + v * 3);
    r = deg > 0 ? sub(quot(s, (double)deg), yv) : D3{-yv.x, -yv.y, -yv.z};
    return deg;
}

// a face pair's two normals as the rule orients them and their cosine in torch.cosine_similarity's form; false: an index names nothing
struct PairGeo { D3 e, p, q, n0, n1; double l0, l1, m0, m1, cosv; };
template <class IT>
__device__ __forceinline__ bool pair_geo(const MpCtx &c, int64_t i, PairGeo &g)
{
    const IT *pr = static_cast<const IT *>(c.pairs) + i * 4;
    const IT v0 = pr[0], v1 = pr[1], va = pr[2], vc = pr[3];
    if (!(in_range(v0, c.V) && in_range(v1, c.V) && in_range(va, c.V) && in_range(vc, c.V))) return false;
    const D3 y0 = ld3(c.y + (int64_t)v0 * 3);
    g.e = sub(ld3(c.y + (int64_t)v1 * 3), y0);
    g.p = sub(ld3(c.y + (int64_t)va * 3), y0);
    g.q = sub(ld3(c.y + (int64_t)vc * 3), y0);
    g.n0 = cross(g.e, g.p);
    g.n1 = mul(cross(g.e, g.q), -1.0);
    g.l0 = sqrt(dot(g.n0, g.n0)); g.l1 = sqrt(dot(g.n1, g.n1));
    g.m0 = fmax(g.l0, kCosEps); g.m1 = fmax(g.l1, kCosEps);
    g.cosv = dot(quot(g.n0, g.m0), quot(g.n1, g.m1));
    return true;
}

template <class IT>
__global__ __launch_bounds__(kClBlock) void k_mp_forward(MpCtx c)
{
    __shared__ double lds[12];
    const int64_t i = (int64_t)blockIdx.x * kClBlock + threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};                                       // edge, nc, laplacian
    if ((c.terms & kTermEdge) && i < c.E) {
        const IT *ed = static_cast<const IT *>(c.edges) + i * 2;
        const IT p = ed[0], q = ed[1];
        if (in_range(p, c.V) && in_range(q, c.V)) {
            const D3 d = sub(ld3(c.y + (int64_t)p * 3), ld3(c.y + (int64_t)q * 3));
            const double t = sqrt(dot(d, d)) - c.target;
            acc[0] = t * t;
        }
    }
    if ((c.terms & kTermNc) && i < c.P) {
        PairGeo g;
        if (pair_geo<IT>(c, i, g)) acc[1] = 1.0 - g.cosv;
    }
    if ((c.terms & kTermLap) && i < c.V) {
        D3 r;
        lap_residual<IT>(c, i, r);
        acc[2] = sqrt(dot(r, r));
    }
    block_sum<3>(acc, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k) c.part[(size_t)blockIdx.x * 3 + k] = acc[k];
}

__global__ __launch_bounds__(kClBlock) void k_mp_finish(MpCtx c)
{
    __shared__ double lds[12];
    double acc[3];
    partial_sum<3>(c.part, c.n_wg, acc, lds);
    if (threadIdx.x == 0) {
        *c.o_edge = ((c.terms & kTermEdge) && c.E > 0) ? (float)(acc[0] / (double)c.E) : 0.0f;
        *c.o_nc = ((c.terms & kTermNc) && c.P > 0) ? (float)(acc[1] / (double)c.P) : 0.0f;
        *c.o_lap = (c.terms & kTermLap) ? (float)(acc[2] / (double)c.V) : 0.0f;
    }
}

// backward, first pass - what the vertex gather cannot compute from its own row: the unit Laplacian residual of every vertex
// (its neighbours need it, divided by ITS degree) and the four gradients of every face pair, each stored once
template <class IT>
__global__ __launch_bounds__(kClBlock) void k_mp_backward_items(MpCtx c)
{
    const int64_t i = (int64_t)blockIdx.x * kClBlock + threadIdx.x;
    if ((c.terms & kTermLap) && i < c.V) {
        D3 r;
        const int64_t deg = lap_residual<IT>(c, i, r);
        const double n = sqrt(dot(r, r));
        const double s = n * (double)(deg > 0 ? deg : 1);
        const D3 w = n > 0.0 ? quot(r, s) : D3{0, 0, 0};                    // |r| = 0: torch's subgradient of the norm, 0
        c.W[i * 3] = w.x; c.W[i * 3 + 1] = w.y; c.W[i * 3 + 2] = w.z;
    }
    if ((c.terms & kTermNc) && i < c.P) {
        PairGeo g;
        D3 gv0{0, 0, 0}, gv1{0, 0, 0}, ga{0, 0, 0}, gc{0, 0, 0};
        if (pair_geo<IT>(c, i, g)) {
            // cos = sum (n0 / m0)(n1 / m1), m = max(|n|, eps) with the clamp outside the graph, as torch has it:
            // d cos / d n0 = (n1 / m1) / m0 - (cos / m0) n0 / |n0|   (second term 0 at |n0| = 0), likewise for n1
            const D3 u0 = g.l0 > 0.0 ? quot(g.n0, g.l0) : D3{0, 0, 0}, u1 = g.l1 > 0.0 ? quot(g.n1, g.l1) : D3{0, 0, 0};
            const D3 g0 = quot(sub(quot(g.n1, g.m1), mul(u0, g.cosv)), -g.m0);   // d (1 - cos) / d n0
            const D3 g1 = quot(sub(quot(g.n0, g.m0), mul(u1, g.cosv)), -g.m1);   // d (1 - cos) / d n1
            const D3 h = mul(g1, -1.0);                                    // n1 = -(e x q)
            const D3 ge = add(cross(g.p, g0), cross(g.q, h));              // n0 = e x p
            ga = cross(g0, g.e);
            gc = cross(h, g.e);
            gv1 = ge;
            gv0 = mul(add(add(ge, ga), gc), -1.0);
        }
        float *o = c.GP + i * 12;
        st3(o, gv0); st3(o + 3, gv1); st3(o + 6, ga); st3(o + 9, gc);
    }
}

// backward, second pass: one lane per vertex, every term a sum over that vertex's rows in their order
template <class IT>
__global__ __launch_bounds__(kClBlock) void k_mp_backward_gather(MpCtx c)
{
    const int64_t v = (int64_t)blockIdx.x * kClBlock + threadIdx.x;
    if (v >= c.V) return;
    const D3 yv = ld3(c.y + v * 3);
    D3 acc{0.0, 0.0, 0.0};
    const bool do_edge = (c.terms & kTermEdge) && c.E > 0, do_lap = (c.terms & kTermLap) != 0;
    if (do_edge || do_lap) {
        const IT *off = static_cast<const IT *>(c.nbr_off), *nbr = static_cast<const IT *>(c.nbr);
        int64_t k0 = (int64_t)off[v], k1 = (int64_t)off[v + 1];
        if (k0 < 0) k0 = 0;
        if (k1 > 2 * c.E) k1 = 2 * c.E;
        const double ce = do_edge ? 2.0 * (double)*c.g_edge / (double)c.E : 0.0;
        D3 se{0.0, 0.0, 0.0}, sl{0.0, 0.0, 0.0};
        int64_t valid = 0;
        for (int64_t k = k0; k < k1; ++k) {
            const IT n = nbr[k];
            if (!in_range(n, c.V)) continue;
            ++valid;
            if (do_edge) {
                const D3 d = sub(yv, ld3(c.y + (int64_t)n * 3));
                const double len = sqrt(dot(d, d));
                if (len > 0.0) se = add(se, mul(d, (len - c.target) / len));   // a zero-length edge: gradient term 0
            }
            if (do_lap) sl = add(sl, D3{c.W[(int64_t)n * 3], c.W[(int64_t)n * 3 + 1], c.W[(int64_t)n * 3 + 2]});
        }
        acc = mul(se, ce);
        if (do_lap) {
            const double deg = (double)(valid > 0 ? valid : 1);             // lap_residual's count
            const D3 own{c.W[v * 3] * deg, c.W[v * 3 + 1] * deg, c.W[v * 3 + 2] * deg};
            acc = add(acc, mul(sub(sl, own), (double)*c.g_lap / (double)c.V));
        }
    }
    if ((c.terms & kTermNc) && c.P > 0) {
        const IT *off = static_cast<const IT *>(c.inc_off), *inc = static_cast<const IT *>(c.inc);
        int64_t k0 = (int64_t)off[v], k1 = (int64_t)off[v + 1];
        if (k0 < 0) k0 = 0;
        if (k1 > 4 * c.P) k1 = 4 * c.P;
        D3 sn{0.0, 0.0, 0.0};
        for (int64_t k = k0; k < k1; ++k) {
            const IT ent = inc[k];
            if (in_range(ent, 4 * c.P)) sn = add(sn, ld3(c.GP + (int64_t)ent * 3));
        }
        acc = add(acc, mul(sn, (double)*c.g_nc / (double)c.P));
    }
    st3(c.grad + v * 3, acc);
}

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }
inline int64_t blocks_for(int64_t items) { return items > 0 ? (items + kClBlock - 1) / kClBlock : 1; }
inline int64_t max3(int64_t a, int64_t b, int64_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }
constexpr int64_t kMaxItems = (int64_t)1 << 38;                             // 2^30 workgroups

struct MpLayout { size_t part, W, GP, total; };
MpLayout mp_layout(int64_t V, int64_t E, int64_t P)
{
    MpLayout L;
    size_t o = 0;
    L.part = o; o += up256((size_t)blocks_for(max3(V, E, P)) * 3 * sizeof(double));
    L.W = o; o += up256((size_t)V * 3 * sizeof(double));
    L.GP = o; o += up256((size_t)(P > 0 ? P : 1) * 12 * sizeof(float));
    L.total = o;
    return L;
}

int la_check(const char *who, int64_t B, int64_t V, int64_t E)
{
    ICON_ARG(B >= 1 && V >= 1 && E >= 0, std::string(who) + ": B and V must be positive, E not negative");
    ICON_ARG(B <= kMaxItems / V && (E == 0 || B <= kMaxItems / E), std::string(who) + ": B * V and B * E must not exceed 2^38");
    return ICON_OK;
}
int mp_check(const char *who, int64_t V, int64_t E, int64_t P)
{
    ICON_ARG(V >= 1 && E >= 0 && P >= 0, std::string(who) + ": V must be positive, E and P not negative");
    ICON_ARG(V <= kMaxItems && E <= kMaxItems && P <= kMaxItems / 4, std::string(who) + ": V, E and 4 P must not exceed 2^38");
    return ICON_OK;
}
int terms_check(const char *who, int terms, int64_t E, int64_t P, const void *edges, const void *nbr_off, const void *nbr, const void *pairs,
                bool need_inc, const void *inc_off, const void *inc)
{
    ICON_ARG(terms >= 1 && terms <= 7, std::string(who) + ": terms must be a non-empty mask of ICON_PRIOR_EDGE | ICON_PRIOR_NC | ICON_PRIOR_LAPLACIAN");
    ICON_ARG(!(terms & kTermEdge) || E == 0 || edges, std::string(who) + ": null edge list");
    ICON_ARG(!(terms & (kTermEdge | kTermLap)) || (nbr_off && (E == 0 || nbr)), std::string(who) + ": null neighbour list");
    ICON_ARG(!(terms & kTermNc) || P == 0 || (pairs && (!need_inc || (inc_off && inc))), std::string(who) + ": null face-pair list");
    return ICON_OK;
}

}  // namespace
}  // namespace icon

using namespace icon;

static_assert(ICON_PRIOR_EDGE == kTermEdge && ICON_PRIOR_NC == kTermNc && ICON_PRIOR_LAPLACIAN == kTermLap, "term bits");

extern "C" int icon_local_affine_bytes(int64_t B, int64_t V, int64_t E, int64_t *bytes)
{
    ICON_ARG(bytes != nullptr, "icon_local_affine_bytes: null argument");
    const int rc = la_check("icon_local_affine_bytes", B, V, E);
    if (rc) return rc;
    *bytes = (int64_t)up256((size_t)blocks_for(B * (V > E ? V : E)) * 2 * sizeof(double));
    return ICON_OK;
}

extern "C" int icon_local_affine_forward(const float *d_x, const float *d_A, const float *d_b, int64_t B, int64_t V,
                                         const void *d_edges, int64_t E, int index_int64, float *d_y, float *d_stiffness,
                                         float *d_rigid, void *d_scratch, int64_t scratch_bytes, void *stream)
{
    const char *who = "icon_local_affine_forward";
    ICON_ARG(d_x && d_A && d_b && d_y && d_stiffness && d_rigid && d_scratch, std::string(who) + ": null argument");
    int rc = la_check(who, B, V, E);
    if (rc) return rc;
    ICON_ARG(E == 0 || d_edges, std::string(who) + ": null edge list");
    int64_t need = 0;
    icon_local_affine_bytes(B, V, E, &need);
    rc = scratch_check(who, "icon_local_affine_bytes", d_scratch, scratch_bytes, (size_t)need);
    if (rc) return rc;
    LaCtx c{};
    c.x = d_x; c.A = d_A; c.b = d_b; c.edges = d_edges; c.B = B; c.V = V; c.E = E;
    c.y = d_y; c.stiff = d_stiffness; c.rigid = d_rigid;
    c.part = static_cast<double *>(d_scratch);
    c.n_wg = (int)blocks_for(B * (V > E ? V : E));
    hipStream_t st = (hipStream_t)stream;
    if (index_int64) hipLaunchKernelGGL(k_la_forward<int64_t>, dim3((unsigned)c.n_wg), dim3(kClBlock), 0, st, c);
    else hipLaunchKernelGGL(k_la_forward<int32_t>, dim3((unsigned)c.n_wg), dim3(kClBlock), 0, st, c);
    hipLaunchKernelGGL(k_la_finish, dim3(1), dim3(kClBlock), 0, st, c);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

extern "C" int icon_local_affine_backward(const float *d_x, const float *d_A, const float *d_b, int64_t B, int64_t V,
                                          const void *d_nbr_off, const void *d_nbr, int64_t E, int index_int64,
                                          const float *d_grad_y, const float *d_grad_stiffness, const float *d_grad_rigid,
                                          float *d_grad_A, float *d_grad_b, void *stream)
{
    const char *who = "icon_local_affine_backward";
    ICON_ARG(d_x && d_A && d_b && d_grad_y && d_grad_stiffness && d_grad_rigid && d_grad_A && d_grad_b, std::string(who) + ": null argument");
    const int rc = la_check(who, B, V, E);
    if (rc) return rc;
    ICON_ARG(E == 0 || (d_nbr_off && d_nbr), std::string(who) + ": null neighbour list");
    LaCtx c{};
    c.x = d_x; c.A = d_A; c.b = d_b; c.nbr_off = d_nbr_off; c.nbr = d_nbr; c.B = B; c.V = V; c.E = E;
    c.gy = d_grad_y; c.g_stiff = d_grad_stiffness; c.g_rigid = d_grad_rigid; c.gA = d_grad_A; c.gb = d_grad_b;
    const unsigned grid = (unsigned)blocks_for(B * V);
    hipStream_t st = (hipStream_t)stream;
    if (index_int64) hipLaunchKernelGGL(k_la_backward<int64_t>, dim3(grid), dim3(kClBlock), 0, st, c);
    else hipLaunchKernelGGL(k_la_backward<int32_t>, dim3(grid), dim3(kClBlock), 0, st, c);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

extern "C" int icon_mesh_priors_bytes(int64_t V, int64_t E, int64_t P, int64_t *bytes)
{
    ICON_ARG(bytes != nullptr, "icon_mesh_priors_bytes: null argument");
    const int rc = mp_check("icon_mesh_priors_bytes", V, E, P);
    if (rc) return rc;
    *bytes = (int64_t)mp_layout(V, E, P).total;
    return ICON_OK;
}

static int mp_context(const char *who, const float *d_verts, int64_t V, const void *d_edges, const void *d_nbr_off, const void *d_nbr, int64_t E,
                      const void *d_pairs, bool need_inc, const void *d_inc_off, const void *d_inc, int64_t P, float target_length, int terms,
                      void *d_scratch, int64_t scratch_bytes, MpCtx &c)
{
    ICON_ARG(d_verts && d_scratch, std::string(who) + ": null argument");
    int rc = mp_check(who, V, E, P);
    if (rc) return rc;
    rc = terms_check(who, terms, E, P, d_edges, d_nbr_off, d_nbr, d_pairs, need_inc, d_inc_off, d_inc);
    if (rc) return rc;
    const MpLayout L = mp_layout(V, E, P);
    rc = scratch_check(who, "icon_mesh_priors_bytes", d_scratch, scratch_bytes, L.total);
    if (rc) return rc;
    char *s = static_cast<char *>(d_scratch);
    c.y = d_verts; c.edges = d_edges; c.nbr_off = d_nbr_off; c.nbr = d_nbr; c.pairs = d_pairs; c.inc_off = d_inc_off; c.inc = d_inc;
    c.V = V; c.E = E; c.P = P; c.target = (double)target_length; c.terms = terms;
    c.part = reinterpret_cast<double *>(s + L.part); c.W = reinterpret_cast<double *>(s + L.W); c.GP = reinterpret_cast<float *>(s + L.GP);
    c.n_wg = (int)blocks_for(max3(V, E, P));
    return ICON_OK;
}

extern "C" int icon_mesh_priors_forward(const float *d_verts, int64_t V, const void *d_edges, const void *d_nbr_off, const void *d_nbr, int64_t E,
                                        const void *d_pairs, int64_t P, int index_int64, float target_length, int terms,
                                        float *d_edge, float *d_nc, float *d_laplacian, void *d_scratch, int64_t scratch_bytes, void *stream)
{
    const char *who = "icon_mesh_priors_forward";
    ICON_ARG(d_edge && d_nc && d_laplacian, std::string(who) + ": null argument");
    MpCtx c{};
    const int rc = mp_context(who, d_verts, V, d_edges, d_nbr_off, d_nbr, E, d_pairs, false, nullptr, nullptr, P, target_length, terms, d_scratch, scratch_bytes, c);
    if (rc) return rc;
    c.o_edge = d_edge; c.o_nc = d_nc; c.o_lap = d_laplacian;
    hipStream_t st = (hipStream_t)stream;
    if (index_int64) hipLaunchKernelGGL(k_mp_forward<int64_t>, dim3((unsigned)c.n_wg), dim3(kClBlock), 0, st, c);
    else hipLaunchKernelGGL(k_mp_forward<int32_t>, dim3((unsigned)c.n_wg), dim3(kClBlock), 0, st, c);
    hipLaunchKernelGGL(k_mp_finish, dim3(1), dim3(kClBlock), 0, st, c);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

extern "C" int icon_mesh_priors_backward(const float *d_verts, int64_t V, const void *d_edges, const void *d_nbr_off, const void *d_nbr, int64_t E,
                                         const void *d_pairs, const void *d_inc_off, const void *d_inc, int64_t P, int index_int64,
                                         float target_length, int terms, const float *d_grad_edge, const float *d_grad_nc,
                                         const float *d_grad_laplacian, float *d_grad_verts, void *d_scratch, int64_t scratch_bytes, void *stream)
{
    const char *who = "icon_mesh_priors_backward";
    ICON_ARG(d_grad_edge && d_grad_nc && d_grad_laplacian && d_grad_verts, std::string(who) + ": null argument");
    MpCtx c{};
    const int rc = mp_context(who, d_verts, V, d_edges, d_nbr_off, d_nbr, E, d_pairs, true, d_inc_off, d_inc, P, target_length, terms, d_scratch, scratch_bytes, c);
    if (rc) return rc;
    c.g_edge = d_grad_edge; c.g_nc = d_grad_nc; c.g_lap = d_grad_laplacian; c.grad = d_grad_verts;
    hipStream_t st = (hipStream_t)stream;
    const unsigned gV = (unsigned)blocks_for(V);
    if (index_int64) {
        hipLaunchKernelGGL(k_mp_backward_items<int64_t>, dim3((unsigned)blocks_for(V > P ? V : P)), dim3(kClBlock), 0, st, c);
        hipLaunchKernelGGL(k_mp_backward_gather<int64_t>, dim3(gV), dim3(kClBlock), 0, st, c);
    } else {
        hipLaunchKernelGGL(k_mp_backward_items<int32_t>, dim3((unsigned)blocks_for(V > P ? V : P)), dim3(kClBlock), 0, st, c);
        hipLaunchKernelGGL(k_mp_backward_gather<int32_t>, dim3(gV), dim3(kClBlock), 0, st, c);
    }
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

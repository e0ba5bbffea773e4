// smpl.hip - SMPL linear blend skinning with its gradients: lbs(..., pose2rot=False) of lib/smplx/lbs.py:152-252 on the device,
// the link between the body-fit loop's parameters (apps/infer.py:163-273) and the renderer.  The rule is DESIGN.md 4.17, pinned
// to the reference's own lbs() through tests/smpl_oracle.py.  Every expression is evaluated in float64 from the float32 inputs
// and rounded to float32 once, where it is stored - plain linear algebra on whatever matrices come in (they need not be
// orthonormal).
//
// Tables (icon_smpl_tables, built once per model by icon_amd/smpl.py: SmplModel): the joints are linear in betas, so the
// regressor is folded into J_template / J_shapedirs and no call reduces over vertices for them; the skin weights are K
// (joint, weight) entries per vertex; the blend-shape tables lie component-major ([..][3][V]) so that the lanes of a wave -
// consecutive vertices - read consecutive floats.
//
// Forward, two launches: k_smpl_chain - one wave per subject walks the kinematic chain j = 1..J-1 in index order (twelve
// lanes, one per entry of the 3x4 transform) and leaves joints and A; k_smpl_vertices - one lane per (subject, vertex): blend
// shapes and skinning, no cross-vertex reduction.  Backward, two launches: k_smpl_bwd_vertices recomputes v_posed and T_v per
// vertex and sums the 12 J + 9 (J - 1) + NB cross-vertex terms per wave (shuffles) and workgroup (LDS) into partials;
// k_smpl_bwd_finish - one workgroup per subject - adds the workgroups' partials in their order, walks the chain backwards
// (j = J-1..0) and folds the pose-feature gradient into grad_rot_mats[:, 1:].  No floating-point atomics: equal bytes from
// run to run.  A joint index outside 0..J-1 is skipped, a parent outside 0..j-1 is read as 0: no table entry is ever used as
// an address unchecked (the host layer refuses such tables before they get here).
#include "common.h"

namespace icon {
namespace {

constexpr int kSmBlock = 256;
constexpr int kSmMaxJ = 64, kSmMaxNB = 512;
constexpr int kSmMaxP = 9 * (kSmMaxJ - 1);
constexpr int kSmRed = 12 * kSmMaxJ;            // widest of the three groups of sums (12 J, 9 (J - 1), NB): one wave's row of the LDS staging

struct SmCtx {
    icon_smpl_tables m;
    const float *betas, *rot;               // [B,NB], [B,J,3,3]
    int64_t B;
    int n_vblk;                             // workgroups per subject of the vertex kernels
    float *verts, *joints;                  // forward out: [B,V,3], [B,J,3]
    float *A;                               // [B,J,3,4]: forward out, backward in
    const float *g_verts, *g_joints;        // backward in, either may be null
    float *g_betas, *g_rot;                 // backward out
    double *part;                           // [B][n_vblk][NS]
    int NS;                                 // 12 J + P + NB
};

// a subject's chain in LDS: the steps of the walk depend on each other, so what they read is staged first and no step waits for memory
struct SmChain {
    double R[kSmMaxJ * 9];                  // the subject's matrices
    double Jd[kSmMaxJ * 3];                 // rest joints
    double G[kSmMaxJ * 12];                 // chain transforms [J][3][4]
    int par[kSmMaxJ];                       // parents; one outside 0..j-1 reads as 0
};

// rest joints and chain transforms of subject b, by every thread of the workgroup
__device__ __forceinline__ void chain_forward(const SmCtx &c, int64_t b, SmChain &s)
{
    const int J = c.m.J, NB = c.m.NB, t = threadIdx.x;
    const float *beta = c.betas + b * NB;
    for (int e = t; e < J * 3; e += blockDim.x) {
        const float *row = c.m.J_shapedirs + (size_t)e * NB;
        double a = (double)c.m.J_template[e];
        for (int l = 0; l < NB; ++l) a += (double)row[l] * (double)beta[l];
        s.Jd[e] = a;
    }
    for (int e = t; e < J * 9; e += blockDim.x) s.R[e] = (double)c.rot[b * J * 9 + e];
    for (int j = t; j < J; j += blockDim.x) {
        const int p = c.m.parents[j];
        s.par[j] = (unsigned)p < (unsigned)j ? p : 0;
    }
    __syncthreads();
    double *G = s.G;
    const int r = t >> 2, cc = t & 3;
    if (t < 12) G[t] = cc < 3 ? s.R[r * 3 + cc] : s.Jd[r];
    __syncthreads();
    for (int j = 1; j < J; ++j) {
        const int p = s.par[j];
        if (t < 12) {
            const double *g = G + p * 12 + r * 4, *Rj = s.R + j * 9;
            double a;
            if (cc < 3) {
                a = (g[0] * Rj[cc] + g[1] * Rj[3 + cc]) + g[2] * Rj[6 + cc];
            } else {
                const double *x = s.Jd + j * 3, *q = s.Jd + p * 3;
                a = ((g[0] * (x[0] - q[0]) + g[1] * (x[1] - q[1])) + g[2] * (x[2] - q[2])) + g[3];
            }
            G[j * 12 + t] = a;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_smpl_chain(SmCtx c)
{
    __shared__ SmChain s;
    const int64_t b = blockIdx.x;
    const int J = c.m.J, t = threadIdx.x;
    chain_forward(c, b, s);
    const double *G = s.G, *Jd = s.Jd;
    for (int e = t; e < J * 3; e += 64) c.joints[b * J * 3 + e] = (float)G[(e / 3) * 12 + (e % 3) * 4 + 3];
    for (int e = t; e < J * 12; e += 64) {
        const int j = e / 12, r = (e % 12) >> 2, cc = e & 3;
        const double *g = G + j * 12 + r * 4, *a = Jd + j * 3;
        c.A[b * J * 12 + e] = (float)(cc < 3 ? g[cc] : g[3] - ((g[0] * a[0] + g[1] * a[1]) + g[2] * a[2]));
    }
}

// what a workgroup of the vertex kernels reads of its subject, staged once: betas, the pose features f = vec(R_j - I) over j >= 1
// (joint-major, then row-major) and A
struct SmStage { float beta[kSmMaxNB]; double f[kSmMaxP]; float A[kSmMaxJ * 12]; };

__device__ __forceinline__ void stage_subject(const SmCtx &c, int64_t b, SmStage &s)
{
    const int J = c.m.J, NB = c.m.NB, P = c.m.P, t = threadIdx.x;
    for (int l = t; l < NB; l += kSmBlock) s.beta[l] = c.betas[b * NB + l];
    for (int p = t; p < P; p += kSmBlock) {
        const int q = p % 9;
        s.f[p] = (double)c.rot[b * J * 9 + 9 + p] - ((q == 0 || q == 4 || q == 8) ? 1.0 : 0.0);
    }
    for (int e = t; e < J * 12; e += kSmBlock) s.A[e] = c.A[b * J * 12 + e];
    __syncthreads();
}

// v_posed and the blended transform T_v [3][4] of vertex v
__device__ __forceinline__ void vertex_eval(const SmCtx &c, int64_t v, const SmStage &s, double (&vp)[3], double (&T)[12])
{
    const size_t V = (size_t)c.m.V;
    const int NB = c.m.NB, P = c.m.P, K = c.m.K, J = c.m.J;
    const float *vt = c.m.v_template + v;
    double s0 = (double)vt[0], s1 = (double)vt[V], s2 = (double)vt[2 * V];
    const float *sd = c.m.shapedirs + v;
#pragma unroll 4
    for (int l = 0; l < NB; ++l) {
        const double bl = (double)s.beta[l];
        const float *q = sd + (size_t)l * 3 * V;
        s0 += (double)q[0] * bl; s1 += (double)q[V] * bl; s2 += (double)q[2 * V] * bl;
    }
    const float *pd = c.m.posedirs + v;
#pragma unroll 8
    for (int p = 0; p < P; ++p) {
        const double f = s.f[p];
        const float *q = pd + (size_t)p * 3 * V;
        s0 += (double)q[0] * f; s1 += (double)q[V] * f; s2 += (double)q[2 * V] * f;
    }
    vp[0] = s0; vp[1] = s1; vp[2] = s2;
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = 0.0;
    const int32_t *si = c.m.skin_idx + (size_t)v * K;
    const float *sw = c.m.skin_w + (size_t)v * K;
    for (int k = 0; k < K; ++k) {
        const int j = si[k];
        if ((unsigned)j >= (unsigned)J) continue;
        const double w = (double)sw[k];
        const float *a = s.A + j * 12;
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] += w * (double)a[e];
    }
}

__global__ __launch_bounds__(kSmBlock) void k_smpl_vertices(SmCtx c)
{
    __shared__ SmStage s;
    const int64_t b = blockIdx.x / c.n_vblk;
    const int64_t v = (int64_t)(blockIdx.x % c.n_vblk) * kSmBlock + threadIdx.x;
    stage_subject(c, b, s);
    if (v >= c.m.V) return;
    double vp[3], T[12];
    vertex_eval(c, v, s, vp, T);
    float *o = c.verts + (b * c.m.V + v) * 3;
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = (float)(((T[r * 4] * vp[0] + T[r * 4 + 1] * vp[1]) + T[r * 4 + 2] * vp[2]) + T[r * 4 + 3]);
}

// The wave's sums of 32 values per lane at once, in 32 exchanges instead of 32 x 6: with lane offset O the lanes whose bit O is
// clear keep the lower H of their 2 H values and take their partner's lower H, the others the upper H - so each exchange halves what a
// lane holds, and the sixteen exchanges of the first step are independent of each other.  A fixed tree: the same bytes every run.
template <int H, int O>
__device__ __forceinline__ void halve(double (&a)[32], int lane)
{
    const bool up = (lane & O) != 0;
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const double send = up ? a[i] : a[i + H], keep = up ? a[i + H] : a[i];
        a[i] = keep + __shfl_xor(send, O, 64);
    }
}
// -> the sum over the wave of value number lane >> 1 (both lanes of a pair hold it)
__device__ __forceinline__ double wave_sum32(double (&a)[32], int lane)
{
    halve<16, 32>(a, lane); halve<8, 16>(a, lane); halve<4, 8>(a, lane); halve<2, 4>(a, lane); halve<1, 2>(a, lane);
    return a[0] + __shfl_xor(a[0], 1, 64);
}

// rw[i] = the wave's sum over its vertices of  g . tab[i][:][v]  for i < n; 32 rows at a time: their loads are in flight together
__device__ __forceinline__ void wave_dots(const float *tab, size_t V, int n, const double (&g)[3], int lane, double *rw)
{
    for (int i0 = 0; i0 < n; i0 += 32) {
        double a[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            // no condition on the loads or on their use - a branch around each would make the 96 loads of a pass wait for each
            // other: a row past the end re-reads the last one and is not stored below; an inactive lane reads vertex 0's column
            // (the caller's `tab`) with g = 0
            const int i = i0 + u < n ? i0 + u : n - 1;
            const float *q = tab + (size_t)i * 3 * V;
            a[u] = (g[0] * (double)q[0] + g[1] * (double)q[V]) + g[2] * (double)q[2 * V];
        }
        const double sum = wave_sum32(a, lane);
        const int i = i0 + (lane >> 1);
        if (!(lane & 1) && i < n) rw[i] = sum;
    }
}

// the four waves' rows of `red`, n entries each, added in wave order into the workgroup's partials
__device__ __forceinline__ void flush_partials(const double *red, int n, double *out)
{
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += kSmBlock) out[e] = ((red[e] + red[kSmRed + e]) + red[2 * kSmRed + e]) + red[3 * kSmRed + e];
    __syncthreads();
}

// one lane per (subject, vertex): with g = grad_verts[b, v], grad T_v = g (v_posed, 1)^T, grad v_posed = T_v^R^T g; the workgroup's
// sums of  w_vj grad T_v  (grad A, 12 J),  grad v_posed . posedirs[p]  (grad f, P)  and  grad v_posed . shapedirs[l]  (NB)
__global__ __launch_bounds__(kSmBlock) void k_smpl_bwd_vertices(SmCtx c)
{
    __shared__ SmStage s;
    __shared__ double red[4 * kSmRed];
    const int64_t b = blockIdx.x / c.n_vblk;
    const int64_t v = (int64_t)(blockIdx.x % c.n_vblk) * kSmBlock + threadIdx.x;
    const size_t V = (size_t)c.m.V;
    const int J = c.m.J, NB = c.m.NB, P = c.m.P, K = c.m.K;
    const int lane = threadIdx.x & 63;
    const bool active = v < c.m.V;
    double *rw = red + (threadIdx.x >> 6) * kSmRed;
    double *out = c.part + (size_t)blockIdx.x * c.NS;
    stage_subject(c, b, s);
    double vp[3] = {0.0, 0.0, 0.0}, T[12], g[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = 0.0;
    uint64_t mine = 0;                                                     // the joints of this vertex's skin row
    if (active) {
        vertex_eval(c, v, s, vp, T);
        const float *gp = c.g_verts + (b * c.m.V + v) * 3;
        g[0] = (double)gp[0]; g[1] = (double)gp[1]; g[2] = (double)gp[2];
        for (int k = 0; k < K; ++k) {
            const int j = c.m.skin_idx[(size_t)v * K + k];
            if ((unsigned)j < (unsigned)J) mine |= (uint64_t)1 << j;
        }
    }
    double gvp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) gvp[k] = (T[k] * g[0] + T[4 + k] * g[1]) + T[8 + k] * g[2];

    // grad A, eight joints at a time: per row r of the transforms the 8 x 4 values  w_vj g_r (v_posed, 1)  are one wave_sum32
    const size_t row = (size_t)(active ? v : 0) * K;
    for (int j0 = 0; j0 < J; j0 += 8) {
        const bool hangs = ((mine >> j0) & 0xff) != 0;
        if (!__any((int)hangs)) {                                          // no vertex of this wave hangs on one of these joints
            for (int e = lane; e < 96; e += 64)
                if (j0 * 12 + e < J * 12) rw[j0 * 12 + e] = 0.0;
            continue;
        }
        double w8[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int k = 0; k < K; ++k) {                                      // no branch around the loads: an inactive lane reads row 0, with g = 0
            const int j = c.m.skin_idx[row + k];
            const double w = (double)c.m.skin_w[row + k];
#pragma unroll
            for (int u = 0; u < 8; ++u) w8[u] += j == j0 + u ? w : 0.0;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            double a[32];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const double wg = w8[u] * g[r];
                a[u * 4] = wg * vp[0]; a[u * 4 + 1] = wg * vp[1]; a[u * 4 + 2] = wg * vp[2]; a[u * 4 + 3] = wg;
            }
            const double sum = wave_sum32(a, lane);
            const int u = lane >> 1, j = j0 + (u >> 2);
            if (!(lane & 1) && j < J) rw[j * 12 + r * 4 + (u & 3)] = sum;
        }
    }
    flush_partials(red, 12 * J, out);

    wave_dots(c.m.posedirs + (active ? v : 0), V, P, gvp, lane, rw);
    flush_partials(red, P, out + 12 * J);
    wave_dots(c.m.shapedirs + (active ? v : 0), V, NB, gvp, lane, rw);
    flush_partials(red, NB, out + 12 * J + P);
}

// one workgroup per subject: the partials in workgroup order, then the chain backwards.  With G_j = G_p o [R_j | rel_j],
// posed joint j = G_j^t and A_j = [G_j^R | G_j^t - G_j^R J_j]:
//   grad G_j^R = grad A_j^R - grad A_j^t J_j^T,  grad G_j^t = grad A_j^t + grad_joints_j,  grad J_j = -G_j^R^T grad A_j^t;  then for j = J-1..1
//   grad R_j = G_p^R^T grad G_j^R,  grad G_p^R += grad G_j^R R_j^T + grad G_j^t rel_j^T,  grad G_p^t += grad G_j^t,
//   grad rel_j = G_p^R^T grad G_j^t  (-> +J_j, -J_p);  grad R_0 = grad G_0^R, grad J_0 += grad G_0^t.
// Waves 0, 1 and 2 each take one of the three updates of a step (12, 9 and 3 lanes).
__global__ __launch_bounds__(kSmBlock) void k_smpl_bwd_finish(SmCtx c)
{
    __shared__ SmChain s;
    __shared__ double gG[kSmMaxJ * 12], gJ[kSmMaxJ * 3], gS[kSmRed + kSmMaxP + kSmMaxNB];
    const int64_t b = blockIdx.x;
    const int J = c.m.J, NB = c.m.NB, P = c.m.P, t = threadIdx.x;
    chain_forward(c, b, s);
    const double *Jd = s.Jd, *G = s.G, *R = s.R;
    for (int e = t; e < c.NS; e += kSmBlock) {
        double a = 0.0;
        if (c.g_verts) {
            const double *p = c.part + (size_t)b * c.n_vblk * c.NS + e;
            for (int w = 0; w < c.n_vblk; ++w) a += p[(size_t)w * c.NS];
        }
        gS[e] = a;
    }
    __syncthreads();
    for (int e = t; e < J * 12; e += kSmBlock) {
        const int j = e / 12, r = (e % 12) >> 2, cc = e & 3;
        const double *ga = gS + j * 12 + r * 4;
        // an absent grad_joints is a zero that is still added: the same operations, the same bytes as with zeros given
        gG[e] = cc < 3 ? ga[cc] - ga[3] * Jd[j * 3 + cc] : ga[3] + (c.g_joints ? (double)c.g_joints[(b * J + j) * 3 + r] : 0.0);
    }
    for (int e = t; e < J * 3; e += kSmBlock) {
        const int j = e / 3, cc = e % 3;
        const double *g = G + j * 12, *ga = gS + j * 12;
        gJ[e] = -((g[cc] * ga[3] + g[4 + cc] * ga[7]) + g[8 + cc] * ga[11]);
    }
    __syncthreads();
    float *gR = c.g_rot + b * J * 9;
    for (int j = J - 1; j >= 1; --j) {
        const int p = s.par[j];
        const double *gj = gG + j * 12, *gp = G + p * 12;
        if (t < 12) {
            const int r = t >> 2, cc = t & 3;
            const double *row = gj + r * 4;
            double a;
            if (cc < 3) {
                const double *Rc = R + j * 9 + cc * 3;
                a = ((row[0] * Rc[0] + row[1] * Rc[1]) + row[2] * Rc[2]) + row[3] * (Jd[j * 3 + cc] - Jd[p * 3 + cc]);
            } else {
                a = row[3];
            }
            gG[p * 12 + t] += a;
        } else if (t >= 64 && t < 73) {
            const int q = t - 64, r = q / 3, cc = q % 3;
            const double a = (gp[r] * gj[cc] + gp[4 + r] * gj[4 + cc]) + gp[8 + r] * gj[8 + cc];
            gR[j * 9 + q] = (float)(a + gS[12 * J + (j - 1) * 9 + q]);
        } else if (t >= 128 && t < 131) {
            const int cc = t - 128;
            const double a = (gp[cc] * gj[3] + gp[4 + cc] * gj[7]) + gp[8 + cc] * gj[11];
            gJ[j * 3 + cc] += a;
            gJ[p * 3 + cc] -= a;
        }
        __syncthreads();
    }
    if (t < 9) gR[t] = (float)gG[(t / 3) * 4 + t % 3];
    else if (t >= 64 && t < 67) gJ[t - 64] += gG[(t - 64) * 4 + 3];
    __syncthreads();
    for (int l = t; l < NB; l += kSmBlock) {
        double a = gS[12 * J + P + l];
        for (int e = 0; e < J * 3; ++e) a += gJ[e] * (double)c.m.J_shapedirs[(size_t)e * NB + l];
        c.g_betas[b * NB + l] = (float)a;
    }
}

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

int sm_check(const char *who, int64_t B, int64_t V, int64_t J, int64_t NB, int64_t K)
{
    ICON_ARG(B >= 1 && V >= 1, std::string(who) + ": B and V must be positive");
    if (J < 1 || J > kSmMaxJ) return fail(ICON_ERR_UNSUPPORTED, std::string(who) + ": J must lie in 1..64");
    if (NB < 0 || NB > kSmMaxNB) return fail(ICON_ERR_UNSUPPORTED, std::string(who) + ": NB must lie in 0..512");
    ICON_ARG(K >= 1 && K <= J, std::string(who) + ": K must lie in 1..J");
    if (B > (((int64_t)1 << 31) - 1) / V) return fail(ICON_ERR_UNSUPPORTED, std::string(who) + ": B * V must stay below 2^31");
    return ICON_OK;
}

int sm_context(const char *who, const icon_smpl_tables *m, const float *d_betas, const float *d_rot, int64_t B, SmCtx &c)
{
    ICON_ARG(m != nullptr && d_rot != nullptr, std::string(who) + ": null argument");
    const int rc = sm_check(who, B, m->V, m->J, m->NB, m->K);
    if (rc) return rc;
    ICON_ARG(m->P == 9 * (m->J - 1), std::string(who) + ": posedirs must have exactly 9 (J - 1) rows");
    ICON_ARG(m->v_template && m->J_template && m->parents && m->skin_idx && m->skin_w, std::string(who) + ": null table");
    ICON_ARG(m->NB == 0 || (m->shapedirs && m->J_shapedirs && d_betas), std::string(who) + ": null shape table or betas");
    ICON_ARG(m->P == 0 || m->posedirs, std::string(who) + ": null posedirs");
    c.m = *m; c.betas = d_betas; c.rot = d_rot; c.B = B;
    c.n_vblk = (int)((m->V + kSmBlock - 1) / kSmBlock);
    c.NS = 12 * m->J + m->P + m->NB;
    return ICON_OK;
}

}  // namespace
}  // namespace icon

using namespace icon;

extern "C" int icon_smpl_bytes(int64_t B, int64_t V, int J, int NB, int K, int64_t *bytes)
{
    ICON_ARG(bytes != nullptr, "icon_smpl_bytes: null argument");
    const int rc = sm_check("icon_smpl_bytes", B, V, J, NB, K);
    if (rc) return rc;
    const size_t n_vblk = (size_t)((V + kSmBlock - 1) / kSmBlock), NS = (size_t)(12 * J + 9 * (J - 1) + NB);
    *bytes = (int64_t)up256((size_t)B * n_vblk * NS * sizeof(double));
    return ICON_OK;
}

extern "C" int icon_smpl_forward(const icon_smpl_tables *tables, const float *d_betas, const float *d_rot_mats, int64_t B,
                                 float *d_verts, float *d_joints, float *d_A, void *stream)
{
    const char *who = "icon_smpl_forward";
    SmCtx c{};
    const int rc = sm_context(who, tables, d_betas, d_rot_mats, B, c);
    if (rc) return rc;
    ICON_ARG(d_verts && d_joints && d_A, std::string(who) + ": null output");
    c.verts = d_verts; c.joints = d_joints; c.A = d_A;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_smpl_chain, dim3((unsigned)B), dim3(64), 0, st, c);
    hipLaunchKernelGGL(k_smpl_vertices, dim3((unsigned)(B * c.n_vblk)), dim3(kSmBlock), 0, st, c);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

extern "C" int icon_smpl_backward(const icon_smpl_tables *tables, const float *d_betas, const float *d_rot_mats, int64_t B,
                                  const float *d_A, const float *d_grad_verts, const float *d_grad_joints,
                                  float *d_grad_betas, float *d_grad_rot_mats, void *d_scratch, int64_t scratch_bytes, void *stream)
{
    const char *who = "icon_smpl_backward";
    SmCtx c{};
    const int rc = sm_context(who, tables, d_betas, d_rot_mats, B, c);
    if (rc) return rc;
    ICON_ARG(d_A && d_grad_rot_mats && (tables->NB == 0 || d_grad_betas) && d_scratch, std::string(who) + ": null argument");
    int64_t need = 0;
    icon_smpl_bytes(B, tables->V, tables->J, tables->NB, tables->K, &need);
    if (const int e = scratch_check(who, "icon_smpl_bytes", d_scratch, scratch_bytes, (size_t)need)) return e;
    c.A = const_cast<float *>(d_A); c.g_verts = d_grad_verts; c.g_joints = d_grad_joints;
    c.g_betas = d_grad_betas; c.g_rot = d_grad_rot_mats; c.part = static_cast<double *>(d_scratch);
    hipStream_t st = (hipStream_t)stream;
    if (d_grad_verts) hipLaunchKernelGGL(k_smpl_bwd_vertices, dim3((unsigned)(B * c.n_vblk)), dim3(kSmBlock), 0, st, c);
    hipLaunchKernelGGL(k_smpl_bwd_finish, dim3((unsigned)B), dim3(kSmBlock), 0, st, c);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

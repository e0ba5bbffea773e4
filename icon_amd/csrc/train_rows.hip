// train_rows.hip - the regressor's input rows of HGPIFuNet.query in TRAINING (lib/net/HGPIFuNet.py:268-359) for every feature
// stack of a call from ONE geometry pass, and the gradient of those rows back into the feature planes.  The rule is DESIGN.md
// 4.22, restated in numpy by tests/train_oracle.py.
//
// Forward (icon_train_rows_forward): the B*N points in subject-major order, as the batched query takes them.
//   icon : call_geometry (the batched search, sign pass, batch-global outlier list - the launches of icon_query_points_batch),
//          k_tr_point (SMPL channels of a point by sdf_attrs, its in_cube flag, its tap record), the existing cmap patch over those
//          channels (outlier_patch), k_tr_rows (a lane per point and stack: the bilinear tap of S7 from the caller's [B,C,H,W] planes)
//   pifu : k_tr_point (z, in_cube, tap record), k_tr_rows
// The SMPL channels live in the workspace's row buffer ([B*N][16], slots 0 .. 6 = sdf | cmap | norm), which is what outlier_patch
// patches; every stack's rows copy them, so two stacks share them bit for bit.
//
// Backward (icon_train_rows_backward): no floating-point atomics.  k_tr_keys gives every point the key of its north-west cell
// (subject, y0 + 1, x0 + 1) - a sentinel when none of its taps lies inside -, one stable radix sort orders the points by cell
// (ascending point index inside a cell), and k_tr_gather runs one wavefront per texel: the texel is the nw / ne / sw / se tap of
// the points of four cells, found by binary search; 16 channel lanes x 4 point lanes sum weight * grad in float64 (the product in
// float32) in a fixed order and the four point lanes are combined by a fixed shuffle tree.  Every texel is written.
//
// pamir (tests/train_pamir_oracle.py): icon_train_pamir_forward = k_tr_point<PAMIR> (no mesh, no search, no outlier list:
// projection, in_cube, the tap record with the projected z in its fourth word) + k_tr_rows<PAMIR> (channels 0 .. C-1 the bilinear tap of
// the planes, C .. C+Cv-1 trilinear_taps' sample of the caller's [B,Cv,D,H,W] volume of that stack, read in place).  The planes' gradient
// is icon_train_rows_backward with Cin = C + Cv, n_select = 1; the volumes' is icon_train_vol_backward (k_tv_keys, one radix sort,
// k_tv_starts, k_tv_gather - stated above those kernels).
#pragma clang fp contract(off)

#include "query_device.h"

#include <rocprim/rocprim.hpp>

namespace icon {
namespace {

constexpr int kTrMaxStacks = 8;
constexpr int kTrChanLanes = 16, kTrPointLanes = 64 / kTrChanLanes;

// 16 bytes per point, forward -> backward: the projected x, y the taps are formed from (bilinear_taps gives the north-west texel, the
// weights and which taps lie inside from them, in the forward's own operations), the sort key of the north-west cell, the feature half
struct alignas(16) TrTap { float x, y; uint32_t key; uint32_t half; };
static_assert(sizeof(TrTap) == 16, "TrTap must be 16 bytes");

struct TrShape {
    int B, C, H, W, S, csel, n_select, smpl_mask, cin;
    int64_t n;                       // points per subject
    uint32_t cells, sentinel;        // (H + 1) (W + 1) cells per subject; key of a point without a tap inside
    int Cv, Dv, Hv, Wv;              // pamir: every stack's volume is [B][Cv][Dv][Hv][Wv], read in place
};

struct TrStacks { const float *p[kTrMaxStacks]; };

__device__ __forceinline__ uint32_t tr_key(const TrShape &q, int64_t b, const BilinearTaps &t)
{
    const bool any = (t.bx0 || t.bx1) && (t.by0 || t.by1);       // then x0 in [-1, W - 1], y0 in [-1, H - 1]
    return any ? (uint32_t)b * q.cells + (uint32_t)(t.y0 + 1) * (uint32_t)(q.W + 1) + (uint32_t)(t.x0 + 1) : q.sentinel;
}

// a lane per point: what does not depend on the stack.  X: the workspace's rows [B*n][kXRow]
template <int PRIOR>
__global__ __launch_bounds__(kBlock) void k_tr_point(TrShape q, BatchDev bd, const float *__restrict__ pts, float sdf_clip, int cmap_local,
                                                     NearRef near, const uint8_t *__restrict__ code8, float *__restrict__ X,
                                                     float *__restrict__ in_cube, TrTap *__restrict__ taps)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= q.n * q.B) return;
    const int64_t b = i / q.n;
    const f3 p = project(batch_calib(bd, b), mk3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
    float *row = X + i * kXRow;
    uint32_t half = 0;
    if (PRIOR == ICON_PRIOR_ICON) {
        // the feature phase of k_features (query_device.h) without the planes: the geometry pre-pass left slot, code byte and d^2
        const uint32_t code = code8[i];
        Nearest nr;
        nr.slot = near_slot_of(near, i); nr.face = 0;
        nr.d2 = (code & kCodeOutlier) ? 0.0f : near_d2(near, i);
        const SdfOut o = sdf_attrs(bd.meshes[b], p, nr, (code & kCodeInside) != 0);
        float s = o.sdf;
        f3 cmv = o.cm;
        if (code & kCodeOutlier) {            // HGPIFuNet.py:298-305
            s = (float)code_sign(code);
            if (cmap_local) cmv = mk3(s, s, s);   // reference mode: patched from the sign list (outlier_patch)
        }
        half = (q.n_select == 2 && o.vis == 0.0f) ? 1u : 0u;     // feat_select: vis == 1 -> front half
        row[0] = s;
        row[1] = cmv.x; row[2] = cmv.y; row[3] = cmv.z;
        row[4] = o.nrm.x; row[5] = o.nrm.y; row[6] = o.nrm.z;
    } else if (PRIOR == ICON_PRIOR_PAMIR) {
        half = __float_as_uint(p.z);          // no feat_select: the fourth word carries the z the trilinear tap is formed from; no row (X is null)
    } else {
        row[0] = p.z;
    }
    in_cube[i] = in_cube_bit(p) ? 1.0f : 0.0f;
    const BilinearTaps t = bilinear_taps(p.x, p.y, q.H, q.W);
    TrTap r;
    r.x = p.x; r.y = p.y; r.key = tr_key(q, b, t); r.half = half;
    taps[i] = r;
}

// a lane per point and stack (blockIdx.y): rows [S][B][cin][n]; the tap is gather_planes' statement over [B][C][H][W] planes
template <int PRIOR>
__global__ __launch_bounds__(kBlock) void k_tr_rows(TrShape q, TrStacks st, TrStacks vols, const TrTap *__restrict__ taps,
                                                    const float *__restrict__ X, float *__restrict__ rows)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= q.n * q.B) return;
    const int s = blockIdx.y;
    const int64_t b = i / q.n, pn = i - b * q.n;
    const TrTap r = taps[i];
    const BilinearTaps t = bilinear_taps(r.x, r.y, q.H, q.W);
    const int x1 = t.x0 + 1, y1 = t.y0 + 1;
    const bool v00 = t.bx0 && t.by0, v01 = t.bx1 && t.by0, v10 = t.bx0 && t.by1, v11 = t.bx1 && t.by1;
    const int64_t hw = (int64_t)q.H * q.W;
    const int64_t o00 = v00 ? (int64_t)t.y0 * q.W + t.x0 : 0, o01 = v01 ? (int64_t)t.y0 * q.W + x1 : 0;
    const int64_t o10 = v10 ? (int64_t)y1 * q.W + t.x0 : 0, o11 = v11 ? (int64_t)y1 * q.W + x1 : 0;
    const int64_t half = PRIOR == ICON_PRIOR_PAMIR ? 0 : (int64_t)r.half;
    const float *plane = st.p[s] + ((int64_t)b * q.C + half * q.csel) * hw;
    float *out = rows + (((int64_t)s * q.B + b) * q.cin) * q.n + pn;
    for (int c = 0; c < q.csel; ++c, plane += hw, out += q.n) {
        const float t00 = v00 ? plane[o00] : 0.0f, t01 = v01 ? plane[o01] : 0.0f;
        const float t10 = v10 ? plane[o10] : 0.0f, t11 = v11 ? plane[o11] : 0.0f;
        float acc = t00 * t.nw; acc += t01 * t.ne; acc += t10 * t.sw; acc += t11 * t.se;
        *out = acc;
    }
    if (PRIOR == ICON_PRIOR_PAMIR) {                             // [img | vol], HGPIFuNet.py:348-359: index(vol_feat, xyz) of this stack's volume
        const TrilinearTaps t3 = trilinear_taps(r.x, r.y, __uint_as_float(r.half), q.Dv, q.Hv, q.Wv);
        const int64_t dhw = (int64_t)q.Dv * q.Hv * q.Wv;
        const float *vol = vols.p[s] + (int64_t)b * q.Cv * dhw;
        for (int c = 0; c < q.Cv; ++c, vol += dhw, out += q.n) *out = trilinear_sample(t3, vol, q.Hv, q.Wv);
        return;
    }
    const float *row = X + i * kXRow;
    *out = row[0]; out += q.n;                                   // sdf (icon) / z (pifu)
    if (PRIOR == ICON_PRIOR_ICON) {                              // [img | sdf | cmap (if) | norm (if)], HGPIFuNet.py:301-311
        if (q.smpl_mask & kSmplCmap) { out[0] = row[1]; out[q.n] = row[2]; out[2 * q.n] = row[3]; out += 3 * q.n; }
        if (q.smpl_mask & kSmplNorm) { out[0] = row[4]; out[q.n] = row[5]; out[2 * q.n] = row[6]; }
    }
}

__global__ __launch_bounds__(kBlock) void k_tr_keys(const TrTap *__restrict__ taps, int64_t NB, uint32_t *__restrict__ keys, int32_t *__restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= NB) return;
    keys[i] = taps[i].key; idx[i] = (int32_t)i;
}

// first position of the sorted keys that is >= key
__device__ __forceinline__ int tr_lower_bound(const uint32_t *__restrict__ keys, int n, uint32_t key)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a wavefront per texel (b, y, x): no barrier, no LDS
__global__ __launch_bounds__(kBlock) void k_tr_gather(TrShape q, uint32_t stack_mask, const TrTap *__restrict__ taps, const uint32_t *__restrict__ keys,
                                                      const int32_t *__restrict__ idx, const float *__restrict__ grad_rows, float *__restrict__ grad_planes)
{
    const int lane = threadIdx.x & 63;
    const int64_t hw = (int64_t)q.H * q.W;
    const int64_t t = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (t >= hw * q.B) return;                                   // wave-uniform
    const int b = (int)(t / hw);
    const int yx = (int)(t - (int64_t)b * hw), y = yx / q.W, x = yx - y * q.W;
    const int NB = (int)(q.n * q.B);
    // the texel is tap k = 0 nw, 1 ne, 2 sw, 3 se of the points whose north-west cell is (y - (k >> 1), x - (k & 1)): lanes 2k and
    // 2k + 1 find that cell's segment of the sorted list
    const int j = lane & 7, kj = j >> 1;
    const uint32_t key = (uint32_t)b * q.cells + (uint32_t)(y + 1 - (kj >> 1)) * (uint32_t)(q.W + 1) + (uint32_t)(x + 1 - (kj & 1)) + (uint32_t)(j & 1);
    const int found = tr_lower_bound(keys, NB, key);
    int lo[4], hi[4], total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { lo[k] = __shfl(found, 2 * k); hi[k] = __shfl(found, 2 * k + 1); total += hi[k] - lo[k]; }
    const int cl = lane & (kTrChanLanes - 1), pl = lane / kTrChanLanes;
    const int nch = q.S * q.C;
    for (int base = 0; base < nch; base += kTrChanLanes) {
        const int ch = base + cl;
        const bool active = ch < nch;
        const int s = active ? ch / q.C : 0, c = active ? ch - s * q.C : 0;
        const uint32_t half = (uint32_t)(c / q.csel);
        const int cp = c - (int)half * q.csel;
        const bool wanted = active && ((stack_mask >> s) & 1u);
        double acc = 0.0;
        if (wanted && total > 0) {
            const float *g = grad_rows + (((int64_t)s * q.B + b) * q.cin + cp) * q.n - (int64_t)b * q.n;   // + i: the point's own column
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                for (int p = lo[k] + pl; p < hi[k]; p += kTrPointLanes) {
                    const int i = idx[p];
                    const TrTap r = taps[i];
                    if (q.n_select == 2 && r.half != half) continue;   // one half: the word is 0 (icon, pifu) or the point's z (pamir)
                    const BilinearTaps bt = bilinear_taps(r.x, r.y, q.H, q.W);
                    const float w = k == 0 ? bt.nw : (k == 1 ? bt.ne : (k == 2 ? bt.sw : bt.se));
                    const float prod = w * g[i];
                    acc += (double)prod;
                }
            }
        }
        acc += __shfl_xor(acc, kTrChanLanes);
        acc += __shfl_xor(acc, 2 * kTrChanLanes);
        if (wanted && pl == 0) grad_planes[(((int64_t)s * q.B + b) * q.C + c) * hw + yx] = (float)acc;
    }
}

struct TrLayout { size_t keys, idx, tmp, tmp_bytes, total; int end_bit; };

int tr_layout(int64_t NB, uint32_t sentinel, TrLayout *L)
{
    int end_bit = 1;
    while (end_bit < 32 && (sentinel >> end_bit) != 0) ++end_bit;
    size_t tmp = 0;
    ICON_HIP(rocprim::radix_sort_pairs(nullptr, tmp, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr,
                                       (size_t)NB, 0, end_bit, (hipStream_t)nullptr));
    ScratchTake take;
    L->keys = take(2 * (size_t)NB * sizeof(uint32_t)); L->idx = take(2 * (size_t)NB * sizeof(int32_t));
    L->tmp = take(tmp); L->tmp_bytes = tmp;
    L->total = take.o; L->end_bit = end_bit;
    return ICON_OK;
}

int tr_shape(int B, int64_t N, int S, int C, int H, int W, int n_select, const char *what, TrShape *q)
{
    ICON_ARG(B >= 1 && N >= 1 && S >= 1 && C >= 1 && H >= 1 && W >= 1, std::string(what) + ": B, N, S, C, H, W must be positive");
    ICON_ARG((int64_t)B * N < (1ll << 31), std::string(what) + ": B * N must be below 2^31");
    if (S > kTrMaxStacks) return fail(ICON_ERR_UNSUPPORTED, std::string(what) + ": more than 8 feature stacks");
    ICON_ARG(n_select == 1 || (n_select == 2 && C % 2 == 0), std::string(what) + ": feat_select needs an even channel count");
    const int64_t cells = (int64_t)(H + 1) * (W + 1);
    if (cells * B >= (1ll << 32) - 1 || (int64_t)B * H * W >= (1ll << 31) * (kBlock / 64))
        return fail(ICON_ERR_UNSUPPORTED, std::string(what) + ": B (H + 1) (W + 1) must stay below 2^32 - 1");
    *q = TrShape{};
    q->B = B; q->C = C; q->H = H; q->W = W; q->S = S; q->n = N; q->n_select = n_select; q->csel = C / n_select;
    q->cells = (uint32_t)cells; q->sentinel = (uint32_t)(cells * B);
    return ICON_OK;
}

// ---- pamir: the gradient of the rows' volume channels into the volumes -------------------------------------------
// grad_vols (s,b,c,z,y,x) = sum of w * grad_rows[s,b,C + c,p] over the points p of subject b that have the voxel among their eight
// taps: w and the product in float32 (trilinear_taps' own statement), the sum in float64 - source cells in corner order, ascending
// point index inside a cell -, rounded once.  k_tv_keys gives every point the key of its north-west-front cell (subject, z0 + 1,
// y0 + 1, x0 + 1), one stable radix sort orders the points by cell, k_tv_starts writes every cell's first sorted position (one
// binary search per cell, once, instead of sixteen per voxel), and k_tv_gather runs one wavefront per run of kTvRun voxels along x:
// its lanes read the 4 x (kTvRun + 2) table entries the run needs with ONE load; then, voxel by voxel, 16 channel lanes x 4 point
// lanes walk the eight cells (point lane l takes the terms lo + l, lo + l + 4, ... of a cell: a cell of thousands of points is
// walked by four lanes) and a fixed shuffle tree (xor 16, then xor 32) combines the point lanes.  Every voxel is written; no LDS.
struct TvShape {
    int B, S, C, Cv, cin, D, H, W;
    int64_t n;                       // points per subject
    uint32_t cells, sentinel;        // (D + 1) (H + 1) (W + 1) cells per subject; key of a point without a tap inside
};
constexpr int kTvRun = 8;            // voxels of one x-run per wavefront

__global__ __launch_bounds__(kBlock) void k_tv_keys(TvShape q, const TrTap *__restrict__ taps, int64_t NB, uint32_t *__restrict__ keys,
                                                    int32_t *__restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= NB) return;
    const TrTap r = taps[i];
    const TrilinearTaps t = trilinear_taps(r.x, r.y, __uint_as_float(r.half), q.D, q.H, q.W);
    const uint32_t b = (uint32_t)(i / q.n);
    const uint32_t cell = ((uint32_t)(t.z0 + 1) * (uint32_t)(q.H + 1) + (uint32_t)(t.y0 + 1)) * (uint32_t)(q.W + 1) + (uint32_t)(t.x0 + 1);
    keys[i] = t.any ? b * q.cells + cell : q.sentinel;
    idx[i] = (int32_t)i;
}

// start[e] = first sorted position whose key is >= e, for e = 0 .. B * cells (the last entry: where the sentinels begin)
__global__ __launch_bounds__(kBlock) void k_tv_starts(const uint32_t *__restrict__ keys, int NB, int64_t entries, int32_t *__restrict__ start)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= entries) return;
    start[e] = tr_lower_bound(keys, NB, (uint32_t)e);
}

// a wavefront per run of kTvRun voxels (b, z, y, xc .. xc + kTvRun - 1): no barrier, no LDS
__global__ __launch_bounds__(kBlock) void k_tv_gather(TvShape q, uint32_t stack_mask, const TrTap *__restrict__ taps, const int32_t *__restrict__ start,
                                                      const int32_t *__restrict__ idx, const float *__restrict__ grad_rows, float *__restrict__ grad_vols)
{
    const int lane = threadIdx.x & 63;
    const int chunks = (q.W + kTvRun - 1) / kTvRun;
    const int64_t t = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (t >= (int64_t)q.B * q.D * q.H * chunks) return;          // wave-uniform
    int64_t u = t / chunks;
    const int xc = (int)(t - u * chunks) * kTvRun;
    const int y = (int)(u % q.H);
    u /= q.H;
    const int z = (int)(u % q.D), b = (int)(u / q.D);
    // lane 16 r + j, r = 2 dz + dy: the start of cell (z + 1 - dz, y + 1 - dy, xc + j), j = 0 .. kTvRun + 1; a row's entry W + 1 is the
    // next row's first (the table has B * cells + 1 entries).  Voxel x = xc + v is tap k = 4 dz + 2 dy + dx of the points of cell
    // (.., .., x + 1 - dx): entries j = v + 1 - dx and j + 1 bound its segment of the sorted list
    const int er = lane >> 4, ej = lane & 15;
    const int64_t row = (int64_t)b * q.cells + ((int64_t)(z + 1 - (er >> 1)) * (q.H + 1) + (y + 1 - (er & 1))) * (q.W + 1);
    const int ex = xc + ej;
    const int ent = start[row + (ex < q.W + 1 ? ex : q.W + 1)];
    const int cl = lane & (kTrChanLanes - 1), pl = lane / kTrChanLanes;
    const int nch = q.S * q.Cv;
    const int64_t dhw = (int64_t)q.D * q.H * q.W;
    for (int base = 0; base < nch; base += kTrChanLanes) {
        const int ch = base + cl;
        const bool active = ch < nch;
        const int s = active ? ch / q.Cv : 0, c = active ? ch - s * q.Cv : 0;
        const bool wanted = active && ((stack_mask >> s) & 1u);
        const float *g = grad_rows + (((int64_t)s * q.B + b) * q.cin + q.C + c) * q.n - (int64_t)b * q.n;   // + i: the point's own column
        float res[kTvRun];
#pragma unroll
        for (int v = 0; v < kTvRun; ++v) {
            double acc = 0.0;
            if (xc + v < q.W) {                                  // wave-uniform
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int src = 16 * (k >> 1) + v + 1 - (k & 1);
                    const int lo = __shfl(ent, src), hi = __shfl(ent, src + 1);
                    if (wanted) {
                        for (int p = lo + pl; p < hi; p += kTrPointLanes) {
                            const int i = idx[p];
                            const TrTap r = taps[i];
                            const TrilinearTaps tt = trilinear_taps(r.x, r.y, __uint_as_float(r.half), q.D, q.H, q.W);
                            const float prod = tt.w[k] * g[i];
                            acc += (double)prod;
                        }
                    }
                }
                acc += __shfl_xor(acc, kTrChanLanes);
                acc += __shfl_xor(acc, 2 * kTrChanLanes);
            }
            res[v] = (float)acc;
        }
        // point lane l stores voxels l and l + 4 of the run: 16 bytes side by side per channel and store
#pragma unroll
        for (int h = 0; h < kTvRun / kTrPointLanes; ++h) {
            const int v = pl + kTrPointLanes * h;
            float val = 0.0f;
#pragma unroll
            for (int m = 0; m < kTvRun; ++m) val = m == v ? res[m] : val;
            if (wanted && xc + v < q.W)
                grad_vols[(((int64_t)s * q.B + b) * q.Cv + c) * dhw + ((int64_t)z * q.H + y) * q.W + xc + v] = val;
        }
    }
}

struct TvLayout { size_t keys, idx, tmp, tmp_bytes, start, total; int end_bit; };

int tv_layout(int64_t NB, const TvShape &q, TvLayout *L)
{
    int end_bit = 1;
    while (end_bit < 32 && (q.sentinel >> end_bit) != 0) ++end_bit;
    size_t tmp = 0;
    ICON_HIP(rocprim::radix_sort_pairs(nullptr, tmp, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr,
                                       (size_t)NB, 0, end_bit, (hipStream_t)nullptr));
    ScratchTake take;
    L->keys = take(2 * (size_t)NB * sizeof(uint32_t)); L->idx = take(2 * (size_t)NB * sizeof(int32_t));
    L->tmp = take(tmp); L->tmp_bytes = tmp;
    L->start = take(((size_t)q.sentinel + 1) * sizeof(int32_t));
    L->total = take.o; L->end_bit = end_bit;
    return ICON_OK;
}

int tv_shape(int B, int64_t N, int S, int Cv, int D, int H, int W, const char *what, TvShape *q)
{
    ICON_ARG(B >= 1 && N >= 1 && S >= 1 && Cv >= 1 && D >= 1 && H >= 1 && W >= 1, std::string(what) + ": B, N, S, Cv, D, H, W must be positive");
    ICON_ARG((int64_t)B * N < (1ll << 31), std::string(what) + ": B * N must be below 2^31");
    if (S > kTrMaxStacks) return fail(ICON_ERR_UNSUPPORTED, std::string(what) + ": more than 8 feature stacks");
    const int64_t rows = (int64_t)(D + 1) * (H + 1);             // < 2^63; below 2^32 before the next product is formed
    const int64_t cells = rows < (1ll << 32) ? rows * (W + 1) : (1ll << 32);
    if (cells >= (1ll << 32) || cells * B >= (1ll << 32) - 1)
        return fail(ICON_ERR_UNSUPPORTED, std::string(what) + ": B (D + 1) (H + 1) (W + 1) must stay below 2^32 - 1 (the sort key has 32 bits)");
    *q = TvShape{};
    q->B = B; q->S = S; q->Cv = Cv; q->D = D; q->H = H; q->W = W; q->n = N;
    q->cells = (uint32_t)cells; q->sentinel = (uint32_t)(cells * B);
    return ICON_OK;
}

}  // namespace
}  // namespace icon

using namespace icon;

extern "C" int icon_train_rows_bytes(int B, int64_t N, int S, int C, int H, int W, int64_t *bytes)
{
    ICON_ARG(bytes != nullptr, "icon_train_rows_bytes: null argument");
    TrShape q;
    int rc;
    if ((rc = tr_shape(B, N, S, C, H, W, 1, "icon_train_rows_bytes", &q))) return rc;
    TrLayout L;
    if ((rc = tr_layout(N * (int64_t)B, q.sentinel, &L))) return rc;
    *bytes = (int64_t)L.total;
    return ICON_OK;
}

extern "C" int icon_train_rows_forward(const icon_mesh_batch_t *mb, int prior_type, float sdf_clip, int cmap_mode, int has_vis,
                                       int has_cmap, int has_norm, const float *const *d_stacks, const int32_t *stack_shapes, int S,
                                       const float *d_calibs, const float *d_points, int64_t N, float *d_rows, float *d_in_cube,
                                       void *d_taps, int search, icon_work_t *work, void *stream)
{
    const char *what = "icon_train_rows_forward";
    ICON_ARG(d_stacks && stack_shapes && d_calibs && d_points && d_rows && d_in_cube && d_taps && work, std::string(what) + ": null argument");
    ICON_ARG(S >= 1, std::string(what) + ": no feature stack");
    if (prior_type == ICON_PRIOR_PAMIR)
        return fail(ICON_ERR_UNSUPPORTED, std::string(what) + ": the pamir prior is not trained here (its rows take the volumes: icon_train_pamir_forward)");
    ICON_ARG(prior_type == ICON_PRIOR_ICON || prior_type == ICON_PRIOR_PIFU, std::string(what) + ": unknown prior_type");
    if (search == ICON_SEARCH_BRUTE) return fail(ICON_ERR_UNSUPPORTED, std::string(what) + ": search 'brute' is evaluated at batch size 1 only");
    if (work->tie_rule != 0) return fail(ICON_ERR_UNSUPPORTED, std::string(what) + ": tie rules are evaluated at batch size 1 only");
    for (int s = 0; s < S; ++s) {
        ICON_ARG(s >= kTrMaxStacks || d_stacks[s] != nullptr, std::string(what) + ": a feature stack is null");
        for (int k = 0; k < 4; ++k)
            ICON_ARG(stack_shapes[4 * s + k] == stack_shapes[k], std::string(what) + ": the feature stacks differ in shape (all must be one [B,C,H,W])");
    }
    const int B = stack_shapes[0], C = stack_shapes[1], H = stack_shapes[2], W = stack_shapes[3];
    const bool icon_prior = prior_type == ICON_PRIOR_ICON;
    TrShape q;
    int rc;
    if ((rc = tr_shape(B, N, S, C, H, W, (icon_prior && has_vis) ? 2 : 1, what, &q))) return rc;
    q.smpl_mask = icon_prior ? ((has_cmap ? kSmplCmap : 0) | (has_norm ? kSmplNorm : 0)) : 0;
    ICON_ARG(((uintptr_t)d_taps & 15) == 0, std::string(what) + ": the tap records must be 16-byte aligned");
    // the call as the common steps see it: its rows in the workspace hold the SMPL channels alone ([sdf | cmap | norm] from slot 0 - a
    // feature layout without image channels); the planes' channels are added per stack by k_tr_rows, so the width of a row of the
    // result, q.cin, is not bounded by a workspace row
    FeatDev smpl_rows{};
    smpl_rows.n_select = 1; smpl_rows.csel = 0; smpl_rows.smpl_mask = q.smpl_mask;
    QueryCall c = query_call(what, Src::Batch, nullptr, prior_type, sdf_clip, cmap_mode, search);
    c.mb = mb; c.points = d_points; c.N = N * (int64_t)B;
    c.bd.calibs = d_calibs; c.bd.n = N; c.bd.B = B;
    if ((rc = describe_call(c, smpl_rows))) return rc;
    q.cin = q.csel + c.c0;
    const int64_t NB = c.N;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = begin_call(work, c, true))) return rc;
    const BatchDev &bd = c.bd;
    const int local = (cmap_mode == ICON_CMAP_LOCAL) ? 1 : 0;
    if ((rc = call_geometry(c, nullptr, work, st))) return rc;
    work->flag_clean = false;                                    // no fused kernel follows the sign pass here: the next one clears its own flag
    TrStacks stacks{};
    for (int s = 0; s < S; ++s) stacks.p[s] = d_stacks[s];
    TrTap *taps = static_cast<TrTap *>(d_taps);
    const unsigned nb = (unsigned)((NB + kBlock - 1) / kBlock);
    const NearRef near = work_near(work, c);
    if (icon_prior)
        hipLaunchKernelGGL(k_tr_point<ICON_PRIOR_ICON>, dim3(nb), dim3(kBlock), 0, st, q, bd, d_points, sdf_clip, local, near,
                           (const uint8_t *)work->d_code8, work->d_x, d_in_cube, taps);
    else
        hipLaunchKernelGGL(k_tr_point<ICON_PRIOR_PIFU>, dim3(nb), dim3(kBlock), 0, st, q, bd, d_points, sdf_clip, local, near,
                           (const uint8_t *)work->d_code8, work->d_x, d_in_cube, taps);
    ICON_HIP(hipGetLastError());
    if ((rc = outlier_patch(work, NB, c.cmap_slot, self_signs(work, c.needs_patch), st))) return rc;
    if (icon_prior)
        hipLaunchKernelGGL(k_tr_rows<ICON_PRIOR_ICON>, dim3(nb, (unsigned)S), dim3(kBlock), 0, st, q, stacks, TrStacks{}, (const TrTap *)taps, (const float *)work->d_x, d_rows);
    else
        hipLaunchKernelGGL(k_tr_rows<ICON_PRIOR_PIFU>, dim3(nb, (unsigned)S), dim3(kBlock), 0, st, q, stacks, TrStacks{}, (const TrTap *)taps, (const float *)work->d_x, d_rows);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

extern "C" int icon_train_rows_backward(const float *d_grad_rows, const void *d_taps, int S, uint32_t stack_mask, int B, int Cin, int C,
                                        int H, int W, int n_select, int64_t N, float *d_grad_planes, void *d_scratch,
                                        int64_t scratch_bytes, void *stream)
{
    const char *what = "icon_train_rows_backward";
    ICON_ARG(d_grad_rows && d_taps && d_grad_planes && d_scratch, std::string(what) + ": null argument");
    TrShape q;
    int rc;
    if ((rc = tr_shape(B, N, S, C, H, W, n_select, what, &q))) return rc;
    ICON_ARG(Cin > q.csel, std::string(what) + ": the rows hold fewer channels than the feature half");
    q.cin = Cin;
    const int64_t NB = N * (int64_t)B;
    TrLayout L;
    if ((rc = tr_layout(NB, q.sentinel, &L))) return rc;
    if ((rc = scratch_check(what, "icon_train_rows_bytes", d_scratch, scratch_bytes, L.total))) return rc;
    char *s = static_cast<char *>(d_scratch);
    uint32_t *k0 = reinterpret_cast<uint32_t *>(s + L.keys), *k1 = k0 + NB;
    int32_t *i0 = reinterpret_cast<int32_t *>(s + L.idx), *i1 = i0 + NB;
    const TrTap *taps = static_cast<const TrTap *>(d_taps);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_tr_keys, dim3((unsigned)((NB + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, taps, NB, k0, i0);
    ICON_HIP(hipGetLastError());
    size_t tmp = L.tmp_bytes;
    ICON_HIP(rocprim::radix_sort_pairs(s + L.tmp, tmp, k0, k1, i0, i1, (size_t)NB, 0, L.end_bit, st));
    const int64_t texels = (int64_t)B * H * W, per = kBlock / 64;
    hipLaunchKernelGGL(k_tr_gather, dim3((unsigned)((texels + per - 1) / per)), dim3(kBlock), 0, st, q, stack_mask, taps, (const uint32_t *)k1,
                       (const int32_t *)i1, d_grad_rows, d_grad_planes);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

// ---- pamir --------------------------------------------------------------------------------------------------------
extern "C" int icon_train_pamir_forward(const float *const *d_stacks, const int32_t *stack_shapes, const float *const *d_vols,
                                        const int32_t *vol_shapes, int S, const float *d_calibs, const float *d_points, int64_t N,
                                        float *d_rows, float *d_in_cube, void *d_taps, void *stream)
{
    const char *what = "icon_train_pamir_forward";
    ICON_ARG(d_stacks && stack_shapes && d_vols && vol_shapes && d_calibs && d_points && d_rows && d_in_cube && d_taps, std::string(what) + ": null argument");
    ICON_ARG(S >= 1, std::string(what) + ": no feature stack");
    if (S > kTrMaxStacks) return fail(ICON_ERR_UNSUPPORTED, std::string(what) + ": more than 8 feature stacks");
    for (int s = 0; s < S; ++s) {
        ICON_ARG(d_stacks[s] != nullptr, std::string(what) + ": a feature stack is null");
        ICON_ARG(d_vols[s] != nullptr, std::string(what) + ": a volume is null");
        for (int k = 0; k < 4; ++k)
            ICON_ARG(stack_shapes[4 * s + k] == stack_shapes[k], std::string(what) + ": the feature stacks differ in shape (all must be one [B,C,H,W])");
        for (int k = 0; k < 5; ++k)
            ICON_ARG(vol_shapes[5 * s + k] == vol_shapes[k], std::string(what) + ": the volumes differ in shape (all must be one [B,Cv,D,H,W])");
    }
    const int B = stack_shapes[0], C = stack_shapes[1], H = stack_shapes[2], W = stack_shapes[3];
    ICON_ARG(vol_shapes[0] == B, std::string(what) + ": the volumes hold another number of subjects than the planes");
    TrShape q;
    TvShape qv;
    int rc;
    if ((rc = tr_shape(B, N, S, C, H, W, 1, what, &q))) return rc;
    if ((rc = tv_shape(B, N, S, vol_shapes[1], vol_shapes[2], vol_shapes[3], vol_shapes[4], what, &qv))) return rc;
    q.Cv = qv.Cv; q.Dv = qv.D; q.Hv = qv.H; q.Wv = qv.W;
    q.cin = C + q.Cv;
    ICON_ARG(((uintptr_t)d_taps & 15) == 0, std::string(what) + ": the tap records must be 16-byte aligned");
    const int64_t NB = N * (int64_t)B;
    hipStream_t st = (hipStream_t)stream;
    BatchDev bd{};
    bd.calibs = d_calibs; bd.n = N; bd.B = B;
    TrStacks stacks{}, vols{};
    for (int s = 0; s < S; ++s) { stacks.p[s] = d_stacks[s]; vols.p[s] = d_vols[s]; }
    TrTap *taps = static_cast<TrTap *>(d_taps);
    const unsigned nb = (unsigned)((NB + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_tr_point<ICON_PRIOR_PAMIR>, dim3(nb), dim3(kBlock), 0, st, q, bd, d_points, 0.0f, 0, NearRef{}, (const uint8_t *)nullptr,
                       (float *)nullptr, d_in_cube, taps);
    ICON_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_tr_rows<ICON_PRIOR_PAMIR>, dim3(nb, (unsigned)S), dim3(kBlock), 0, st, q, stacks, vols, (const TrTap *)taps, (const float *)nullptr, d_rows);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

extern "C" int icon_train_vol_bytes(int B, int64_t N, int S, int Cv, int D, int H, int W, int64_t *bytes)
{
    ICON_ARG(bytes != nullptr, "icon_train_vol_bytes: null argument");
    TvShape q;
    int rc;
    if ((rc = tv_shape(B, N, S, Cv, D, H, W, "icon_train_vol_bytes", &q))) return rc;
    TvLayout L;
    if ((rc = tv_layout(N * (int64_t)B, q, &L))) return rc;
    *bytes = (int64_t)L.total;
    return ICON_OK;
}

extern "C" int icon_train_vol_backward(const float *d_grad_rows, const void *d_taps, int S, uint32_t stack_mask, int B, int Cin, int C,
                                       int Cv, int D, int H, int W, int64_t N, float *d_grad_vols, void *d_scratch,
                                       int64_t scratch_bytes, void *stream)
{
    const char *what = "icon_train_vol_backward";
    ICON_ARG(d_grad_rows && d_taps && d_grad_vols && d_scratch, std::string(what) + ": null argument");
    TvShape q;
    int rc;
    if ((rc = tv_shape(B, N, S, Cv, D, H, W, what, &q))) return rc;
    ICON_ARG(C >= 1 && Cin >= C + Cv, std::string(what) + ": the rows hold fewer channels than the planes' and the volumes' together");
    q.C = C; q.cin = Cin;
    const int64_t NB = N * (int64_t)B;
    TvLayout L;
    if ((rc = tv_layout(NB, q, &L))) return rc;
    if ((rc = scratch_check(what, "icon_train_vol_bytes", d_scratch, scratch_bytes, L.total))) return rc;
    char *s = static_cast<char *>(d_scratch);
    uint32_t *k0 = reinterpret_cast<uint32_t *>(s + L.keys), *k1 = k0 + NB;
    int32_t *i0 = reinterpret_cast<int32_t *>(s + L.idx), *i1 = i0 + NB;
    int32_t *start = reinterpret_cast<int32_t *>(s + L.start);
    const TrTap *taps = static_cast<const TrTap *>(d_taps);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_tv_keys, dim3((unsigned)((NB + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, q, taps, NB, k0, i0);
    ICON_HIP(hipGetLastError());
    size_t tmp = L.tmp_bytes;
    ICON_HIP(rocprim::radix_sort_pairs(s + L.tmp, tmp, k0, k1, i0, i1, (size_t)NB, 0, L.end_bit, st));
    const int64_t entries = (int64_t)q.sentinel + 1;
    hipLaunchKernelGGL(k_tv_starts, dim3((unsigned)((entries + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, (const uint32_t *)k1, (int)NB, entries, start);
    ICON_HIP(hipGetLastError());
    const int64_t runs = (int64_t)B * D * H * ((W + kTvRun - 1) / kTvRun), per = kBlock / 64;
    hipLaunchKernelGGL(k_tv_gather, dim3((unsigned)((runs + per - 1) / per)), dim3(kBlock), 0, st, q, stack_mask, taps, (const int32_t *)start,
                       (const int32_t *)i1, d_grad_rows, d_grad_vols);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

// mesh_rules.h - the decisions of the per-image BVH / ray-bin build that the device builder (mesh_device.hip)
// and the host builder (mesh_build.cpp: the checker of the device build, and the path for ICON_AMD_MESH_BUILD=host)
// must make IDENTICALLY, so that both emit the same arrays bit for bit (tests/test_gpu_mesh_build.py compares them).
//
// float32 / float64 arithmetic without contraction (both translation units are compiled with -ffp-contract=off).
#pragma once
#include "common.h"

namespace icon {

// ---- depth bound ------------------------------------------------------------------------------------------
// The traversal stacks (one LDS word per level per wave; 64 frontier entries per level in the one-wave-per-point
// search) are sized on the host BEFORE the tree exists, so the builder guarantees a bound that depends on F only:
// a node of n triangles at depth d may take a SAH split only if, with median splits from there on, no leaf would
// end up deeper than depth_bound(F); otherwise it is halved by position.
__host__ __device__ inline int ilog2_ceil(int64_t n) { int l = 0; while (((int64_t)1 << l) < n) ++l; return l; }
__host__ __device__ inline int median_levels(int n) { int l = 0; while (n > kLeafMax) { n = (n + 1) / 2; ++l; } return l; }
__host__ __device__ inline int depth_bound(int64_t F)
{
    const int b = ilog2_ceil(F < 2 ? 2 : F) + 10;
    return b < kStackDepth - 2 ? b : kStackDepth - 2;
}
__host__ __device__ inline bool force_median(int depth, int n, int bound) { return depth + 1 + median_levels(n - 1) > bound; }

// ---- input hygiene ------------------------------------------------------------------------------------------
// a coordinate the builder refuses (host build: error; device build: status bit, the coordinate counts as 0)
__host__ __device__ inline bool bad_coord(float v) { return !(v >= -1e6f && v <= 1e6f); }
// -0 -> +0: min / max then give the same bits whatever the order of the operands
__host__ __device__ inline float canon(float v) { return v + 0.0f; }

// ---- binned SAH ------------------------------------------------------------------------------------------
constexpr int kSahBins = 16;
__host__ __device__ inline int sah_bin(float c, float lo, float ext)
{
    int b = (int)((c - lo) / ext * (float)kSahBins);
    return b < 0 ? 0 : (b > kSahBins - 1 ? kSahBins - 1 : b);
}
struct BoxD { float lo[3], hi[3]; };
__host__ __device__ inline double box_area(const float lo[3], const float hi[3])
{
    const double dx0 = (double)hi[0] - lo[0], dy0 = (double)hi[1] - lo[1], dz0 = (double)hi[2] - lo[2];
    const double dx = dx0 > 0.0 ? dx0 : 0.0, dy = dy0 > 0.0 ? dy0 : 0.0, dz = dz0 > 0.0 ? dz0 : 0.0;
    return 2.0 * (dx * dy + dy * dz + dz * dx);
}

// ---- (y,z) ray bins: square cells, about two per triangle, float32 throughout (IEEE sqrt / divide on both sides) ----
struct BinGrid { float y0, z0, y1, z1, inv_y, inv_z; int gy, gz; };
constexpr float kBinEps = 1e-5f;
__host__ __device__ inline BinGrid bin_grid(const float box_lo[3], const float box_hi[3], int64_t F)
{
    BinGrid g;
    g.y0 = box_lo[1] - 4 * kBinEps; g.y1 = box_hi[1] + 4 * kBinEps;
    g.z0 = box_lo[2] - 4 * kBinEps; g.z1 = box_hi[2] + 4 * kBinEps;
    const float ey = g.y1 - g.y0, ez = g.z1 - g.z0;
    float a = ey * ez;
    if (!(a > 1e-12f)) a = 1e-12f;
    const float cell = sqrtf(a / (2.0f * (float)F));
    int gy = (int)ceilf(ey / cell), gz = (int)ceilf(ez / cell);
    g.gy = gy < 1 ? 1 : (gy > 2048 ? 2048 : gy);
    g.gz = gz < 1 ? 1 : (gz > 2048 ? 2048 : gz);
    g.inv_y = (float)g.gy / ey; g.inv_z = (float)g.gz / ez;
    return g;
}
__host__ __device__ inline int bin_cell_of(float v, float v0, float inv, int g)
{
    const int c = (int)floorf((v - v0) * inv);
    return c < 0 ? 0 : (c > g - 1 ? g - 1 : c);
}
// cells and list entries the arena reserves (gy * gz <= 2 F + gy + gz + 1; entries: 48 per triangle on average
// is ~3x what a body mesh needs - beyond it the inside tests fall back to the brute-force parity count)
__host__ __device__ inline int64_t bin_cells_cap(int64_t F) { return 2 * F + 4100; }
__host__ __device__ inline int64_t bin_entries_cap(int64_t F) { return 48 * F + 2 * bin_cells_cap(F); }

// S2 per-triangle constants (same float32 operation sequence as the checker's orc_tri_setup)
__host__ __device__ inline float dot3r(const float *a, const float *b) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }
__host__ __device__ inline void tri_setup(const float *a, const float *b, const float *c, int32_t face, TriPre &t)
{
    for (int k = 0; k < 3; ++k) { t.a[k] = a[k]; t.b[k] = b[k]; t.ab[k] = b[k] - a[k]; t.ac[k] = c[k] - a[k]; t.bc[k] = c[k] - b[k]; }
    t.a00 = dot3r(t.ab, t.ab); t.a01 = dot3r(t.ab, t.ac); t.a11 = dot3r(t.ac, t.ac);
    const float b11 = dot3r(t.bc, t.bc);
    t.i00 = (t.a00 > 0.0f) ? 1.0f / t.a00 : 0.0f;
    t.i11 = (t.a11 > 0.0f) ? 1.0f / t.a11 : 0.0f;
    t.ibc = (b11 > 0.0f) ? 1.0f / b11 : 0.0f;
    const float nn = fmaf(t.a00, t.a11, -(t.a01 * t.a01));
    // zero area (or a sliver whose Gram determinant rounds to <= 0): NaN makes both barycentrics NaN, every
    // comparison of the inside test false, and the distance the minimum over the three edge segments - exact
    t.inn = (nn > 0.0f) ? 1.0f / nn : __builtin_nanf("");
    t.face = face; t.pad = 0;
}

// ---- oriented box of a leaf pair (PairBox, common.h) ----------------------------------------------------------------------
// A lower bound of the squared distance from a point to two triangles that the packet walk evaluates before the distance test
// itself.  Frame: n = the normalised sum of the two area-weighted normals, u1 = the pair's longest edge with its n component
// removed, u2 = n x u1 - tight along the normal, where an axis-aligned box of a slanted patch is not.  ANY orthonormal frame
// gives a valid bound, so every doubtful case (zero area, collinear slivers, duplicates, opposed normals, a frame whose Gram
// matrix is off by more than kPairBoxGram) takes the identity frame: the pair's AABB.  A pair with a non-finite corner, or
// whose box overflows float32, gets infinite extents and is never culled.
// The contract (DESIGN.md "BVH conservativeness"): the float32 value of pair_box_bound never exceeds the real squared distance
// from the point to either triangle.  What pays for the rounding: the stored axes are the unit vectors TIMES kPairBoxScale (the
// sum of squares comes out 2e-4 low - the frame's non-orthonormality, the sum's own rounding, and the rounding of the
// projections of a point that is far from the box relative to its size), and the half extents are inflated by kPairBoxEps
// times their sum (the rounding of the projections of a point nearer than that, and of the extents themselves).
constexpr float kPairBoxScale = 0.9999f;
constexpr float kPairBoxGram = 4e-6f;
constexpr float kPairBoxEps = 4e-6f;
constexpr float kPairBoxFloor = 1e-15f;
enum { kPairBoxOriented = 0, kPairBoxAabb = 1, kPairBoxNever = 2 };

__host__ __device__ inline bool pb_finite(float v)
{
    uint32_t u; __builtin_memcpy(&u, &v, 4);
    return (u & 0x7f800000u) != 0x7f800000u;
}
__host__ __device__ inline void pb_cross(const float *a, const float *b, float *r)
{
    r[0] = fmaf(a[1], b[2], -(a[2] * b[1])); r[1] = fmaf(a[2], b[0], -(a[0] * b[2])); r[2] = fmaf(a[0], b[1], -(a[1] * b[0]));
}
// v: the six corners (triangle 0: v[0..2], triangle 1: v[3..5]; a pair of one triangle passes it twice).
// out[15]: centre, the three scaled axes, the inflated half extents (PairBox fields 0..14).  Returns kPairBox*.
__host__ __device__ inline int pair_box_setup(const float v[6][3], float out[15])
{
    bool fin = true;
    for (int i = 0; i < 6; ++i) for (int k = 0; k < 3; ++k) fin = fin && pb_finite(v[i][k]);
    float ax[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}};
    int kind = kPairBoxAabb;
    if (fin) {
        // the frame
        float e[6][3], l2[6];
        for (int t = 0; t < 2; ++t)
            for (int k = 0; k < 3; ++k) {
                e[3 * t][k] = v[3 * t + 1][k] - v[3 * t][k]; e[3 * t + 1][k] = v[3 * t + 2][k] - v[3 * t][k];
                e[3 * t + 2][k] = v[3 * t + 2][k] - v[3 * t + 1][k];
            }
        int best = 0;
        for (int i = 0; i < 6; ++i) { l2[i] = dot3r(e[i], e[i]); if (l2[i] > l2[best]) best = i; }
        const float L2 = l2[best];
        float n0[3], n1[3], n[3];
        pb_cross(e[0], e[1], n0); pb_cross(e[3], e[4], n1);
        for (int k = 0; k < 3; ++k) n[k] = n0[k] + n1[k];
        const float nn = dot3r(n, n);
        if (nn > 1e-10f * (L2 * L2)) {
            const float ln = sqrtf(nn);
            float a0[3], u[3], a1[3], a2[3];
            for (int k = 0; k < 3; ++k) a0[k] = n[k] / ln;
            const float en = dot3r(e[best], a0);
            for (int k = 0; k < 3; ++k) u[k] = fmaf(-en, a0[k], e[best][k]);
            const float uu = dot3r(u, u);
            if (uu > 1e-10f * L2) {
                const float lu = sqrtf(uu);
                for (int k = 0; k < 3; ++k) a1[k] = u[k] / lu;
                pb_cross(a0, a1, a2);
                const float g[6] = {dot3r(a0, a0) - 1.0f, dot3r(a1, a1) - 1.0f, dot3r(a2, a2) - 1.0f, dot3r(a0, a1), dot3r(a0, a2), dot3r(a1, a2)};
                bool ok = true;
                for (int i = 0; i < 6; ++i) ok = ok && (fabsf(g[i]) <= kPairBoxGram);      // (a NaN fails)
                if (ok) {
                    for (int k = 0; k < 3; ++k) { ax[0][k] = a0[k]; ax[1][k] = a1[k]; ax[2][k] = a2[k]; }
                    kind = kPairBoxOriented;
                }
            }
        }
    }
    for (int attempt = 0; attempt < 2 && fin; ++attempt) {
        // centre: the middle of the corners' AABB, moved to the middle of their extent along every axis
        float c[3];
        for (int k = 0; k < 3; ++k) {
            float lo = v[0][k], hi = v[0][k];
            for (int i = 1; i < 6; ++i) { lo = fminf(lo, v[i][k]); hi = fmaxf(hi, v[i][k]); }
            c[k] = canon(0.5f * (lo + hi));
        }
        float mid[3];
        for (int a = 0; a < 3; ++a) {
            float lo = 0.f, hi = 0.f;
            for (int i = 0; i < 6; ++i) {
                const float d[3] = {v[i][0] - c[0], v[i][1] - c[1], v[i][2] - c[2]};
                const float t = dot3r(ax[a], d);
                lo = i ? fminf(lo, t) : t; hi = i ? fmaxf(hi, t) : t;
            }
            mid[a] = 0.5f * (lo + hi);
        }
        for (int k = 0; k < 3; ++k) c[k] = canon(fmaf(mid[2], ax[2][k], fmaf(mid[1], ax[1][k], fmaf(mid[0], ax[0][k], c[k]))));
        // the stored axes and the extents of the corners along THEM, about the stored centre
        float h[3];
        for (int a = 0; a < 3; ++a) {
            for (int k = 0; k < 3; ++k) out[3 + 3 * a + k] = canon(ax[a][k] * kPairBoxScale);
            float m = 0.f;
            for (int i = 0; i < 6; ++i) {
                const float d[3] = {v[i][0] - c[0], v[i][1] - c[1], v[i][2] - c[2]};
                m = fmaxf(m, fabsf(dot3r(out + 3 + 3 * a, d)));
            }
            h[a] = m;
        }
        const float pad = fmaf(kPairBoxEps, (h[0] + h[1]) + h[2], kPairBoxFloor);
        bool ok = true;
        for (int k = 0; k < 3; ++k) { out[k] = c[k]; out[12 + k] = h[k] + pad; ok = ok && pb_finite(c[k]) && pb_finite(out[12 + k]); }
        if (ok) return kind;
        if (kind == kPairBoxAabb) break;
        kind = kPairBoxAabb;                                         // (the oriented frame overflowed: once more with the identity)
        for (int a = 0; a < 3; ++a) for (int k = 0; k < 3; ++k) ax[a][k] = (a == k) ? 1.f : 0.f;
    }
    for (int k = 0; k < 3; ++k) { out[k] = 0.f; out[12 + k] = __builtin_inff(); }
    for (int a = 0; a < 3; ++a) for (int k = 0; k < 3; ++k) out[3 + 3 * a + k] = (a == k) ? kPairBoxScale : 0.f;
    return kPairBoxNever;
}

// ---- oriented box of a slot range (the node boxes: PairBox records indexed by node id) ----------------------------------------------------------
// pair_box_setup's rule for the n >= 1 triangles of a slot range instead of the two of a pair: a parent whose two children both hold
// at most kNodeBoxMaxTris triangles (an "oriented parent"; a child may be a leaf or an inner node) tests its children by one such
// box each instead of their AABBs - from distance D the AABB of a slanted patch of thickness t admits everything within
// sqrt(2 D t), at every small subtree just as at a leaf.  tri: corner k of triangle i at tri[i * stride + 3 * k ..]
// (TriRec: stride 12).  Sums and searches run in slot order, then corner / edge order (ab, ac, bc), and take the FIRST maximum.
// Same frame (n = normalised sum of the area normals, u1 = the longest edge less its n part, u2 = n x u1), same fall-backs, same
// scale and inflation as the pair box: the argument for the contract does not depend on the number of corners.
constexpr int kNodeBoxMaxTris = 16;
constexpr int kNodeBoxFlag = 1 << 30;      // set in a child reference >= 0: that inner node is an oriented parent (node ids are < 2^23)
__host__ __device__ inline int range_box_setup(const float *tri, int stride, int n, float out[15])
{
    bool fin = true;
    for (int i = 0; i < n; ++i) for (int k = 0; k < 9; ++k) fin = fin && pb_finite(tri[(size_t)i * stride + k]);
    float ax[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}};
    int kind = kPairBoxAabb;
    if (fin) {
        // the frame
        float eb[3] = {0.f, 0.f, 0.f}, nsum[3] = {0.f, 0.f, 0.f}, L2 = 0.f;
        for (int i = 0; i < n; ++i) {
            const float *a = tri + (size_t)i * stride, *b = a + 3, *c = a + 6;
            float e[3][3];
            for (int k = 0; k < 3; ++k) { e[0][k] = b[k] - a[k]; e[1][k] = c[k] - a[k]; e[2][k] = c[k] - b[k]; }
            for (int j = 0; j < 3; ++j) {
                const float l2 = dot3r(e[j], e[j]);
                if ((i == 0 && j == 0) || l2 > L2) { L2 = l2; for (int k = 0; k < 3; ++k) eb[k] = e[j][k]; }
            }
            float nt[3];
            pb_cross(e[0], e[1], nt);
            for (int k = 0; k < 3; ++k) nsum[k] = i ? nsum[k] + nt[k] : nt[k];
        }
        const float nn = dot3r(nsum, nsum);
        if (nn > 1e-10f * (L2 * L2)) {
            const float ln = sqrtf(nn);
            float a0[3], u[3], a1[3], a2[3];
            for (int k = 0; k < 3; ++k) a0[k] = nsum[k] / ln;
            const float en = dot3r(eb, a0);
            for (int k = 0; k < 3; ++k) u[k] = fmaf(-en, a0[k], eb[k]);
            const float uu = dot3r(u, u);
            if (uu > 1e-10f * L2) {
                const float lu = sqrtf(uu);
                for (int k = 0; k < 3; ++k) a1[k] = u[k] / lu;
                pb_cross(a0, a1, a2);
                const float g[6] = {dot3r(a0, a0) - 1.0f, dot3r(a1, a1) - 1.0f, dot3r(a2, a2) - 1.0f, dot3r(a0, a1), dot3r(a0, a2), dot3r(a1, a2)};
                bool ok = true;
                for (int i = 0; i < 6; ++i) ok = ok && (fabsf(g[i]) <= kPairBoxGram);      // (a NaN fails)
                if (ok) {
                    for (int k = 0; k < 3; ++k) { ax[0][k] = a0[k]; ax[1][k] = a1[k]; ax[2][k] = a2[k]; }
                    kind = kPairBoxOriented;
                }
            }
        }
    }
    const int nc = 3 * n;
    for (int attempt = 0; attempt < 2 && fin; ++attempt) {
        // centre: the middle of the corners' AABB, moved to the middle of their extent along every axis
        float c[3];
        for (int k = 0; k < 3; ++k) {
            float lo = tri[k], hi = tri[k];
            for (int i = 1; i < nc; ++i) { const float v = tri[(size_t)(i / 3) * stride + 3 * (i % 3) + k]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
            c[k] = canon(0.5f * (lo + hi));
        }
        float mid[3];
        for (int a = 0; a < 3; ++a) {
            float lo = 0.f, hi = 0.f;
            for (int i = 0; i < nc; ++i) {
                const float *v = tri + (size_t)(i / 3) * stride + 3 * (i % 3);
                const float d[3] = {v[0] - c[0], v[1] - c[1], v[2] - c[2]};
                const float t = dot3r(ax[a], d);
                lo = i ? fminf(lo, t) : t; hi = i ? fmaxf(hi, t) : t;
            }
            mid[a] = 0.5f * (lo + hi);
        }
        for (int k = 0; k < 3; ++k) c[k] = canon(fmaf(mid[2], ax[2][k], fmaf(mid[1], ax[1][k], fmaf(mid[0], ax[0][k], c[k]))));
        // the stored axes and the extents of the corners along THEM, about the stored centre
        float h[3];
        for (int a = 0; a < 3; ++a) {
            for (int k = 0; k < 3; ++k) out[3 + 3 * a + k] = canon(ax[a][k] * kPairBoxScale);
            float m = 0.f;
            for (int i = 0; i < nc; ++i) {
                const float *v = tri + (size_t)(i / 3) * stride + 3 * (i % 3);
                const float d[3] = {v[0] - c[0], v[1] - c[1], v[2] - c[2]};
                m = fmaxf(m, fabsf(dot3r(out + 3 + 3 * a, d)));
            }
            h[a] = m;
        }
        const float pad = fmaf(kPairBoxEps, (h[0] + h[1]) + h[2], kPairBoxFloor);
        bool ok = true;
        for (int k = 0; k < 3; ++k) { out[k] = c[k]; out[12 + k] = h[k] + pad; ok = ok && pb_finite(c[k]) && pb_finite(out[12 + k]); }
        if (ok) return kind;
        if (kind == kPairBoxAabb) break;
        kind = kPairBoxAabb;                                         // (the oriented frame overflowed: once more with the identity)
        for (int a = 0; a < 3; ++a) for (int k = 0; k < 3; ++k) ax[a][k] = (a == k) ? 1.f : 0.f;
    }
    for (int k = 0; k < 3; ++k) { out[k] = 0.f; out[12 + k] = __builtin_inff(); }
    for (int a = 0; a < 3; ++a) for (int k = 0; k < 3; ++k) out[3 + 3 * a + k] = (a == k) ? kPairBoxScale : 0.f;
    return kPairBoxNever;
}

// The node-box record of inner node `id` (its split point is slot id + 1), or false: not an oriented parent.  Shared by both builders
// so that they cannot disagree: nodes / tris = the finished tree and the slot-ordered triangle records, F = the slot count.
//   rec: fields 0..14 = the two children's boxes, field-interleaved like a PairBox ([field][child]); field 15 = the two child
//        references as the walk follows them (bit patterns): a leaf code, or an inner node's id | kNodeBoxFlag - an inner child of
//        an oriented parent holds at most kNodeBoxMaxTris triangles, so it is an oriented parent itself.
//   The children's slot ranges are [b0, id + 1) and [id + 1, e1): b0 / e1 are found down the left / right spine of the children.
__host__ __device__ inline bool node_child_range(const BvhNode *nodes, int F, int child, int side, int bound, int &edge)
{
    int c = child;
    for (int it = 0; it <= bound && c >= 0; ++it) { if (c >= F) return false; c = side ? nodes[c].child1 : nodes[c].child0; }
    if (c >= 0) return false;
    const int code = ~c, leaf = code >> 2, cnt = (code & 3) + 1;
    edge = side ? leaf + cnt : leaf;
    return leaf >= 0 && leaf + cnt <= F;
}
__host__ __device__ inline int node_ref_flagged(int ref, int begin, int end)
{
    // ref >= 0 owns [begin, end) and splits it at ref + 1
    if (ref < 0) return ref;
    return (ref + 1 - begin <= kNodeBoxMaxTris && end - (ref + 1) <= kNodeBoxMaxTris) ? (ref | kNodeBoxFlag) : ref;
}

// what both builders do for inner node `id` once the tree and the slot-ordered triangle records exist: nb = its two child references
// as the node-box walk follows them (BvhNode::nb_child), and, for an oriented parent, its record.  Returns 0: the tree is malformed
// (a bug), 1: an AABB parent (rec untouched), 2: an oriented parent.  At most 2 * kNodeBoxMaxTris triangles are read, in slot order.
__host__ __device__ inline int node_box_make(const BvhNode *nodes, const TriRec *tris, int F, int id, int nb[2], PairBox &rec)
{
    const int c0 = nodes[id].child0, c1 = nodes[id].child1, mid = id + 1;
    int b0 = 0, e1 = 0;
    if (!node_child_range(nodes, F, c0, 0, kStackDepth, b0) || !node_child_range(nodes, F, c1, 1, kStackDepth, e1) || !(b0 < mid && mid < e1)) return 0;
    nb[0] = node_ref_flagged(c0, b0, mid); nb[1] = node_ref_flagged(c1, mid, e1);
    if (mid - b0 > kNodeBoxMaxTris || e1 - mid > kNodeBoxMaxTris) return 1;
    for (int s = 0; s < 2; ++s) {
        float r[15];
        range_box_setup(reinterpret_cast<const float *>(tris + (s ? mid : b0)), (int)(sizeof(TriRec) / 4), s ? e1 - mid : mid - b0, r);
        for (int fld = 0; fld < 15; ++fld) rec.f[fld][s] = r[fld];
        __builtin_memcpy(&rec.f[15][s], &nb[s], 4);
    }
    return 2;
}

// Both pair boxes of a leaf at once (packed f32: the operand shape of v_pk_add / v_pk_mul / v_pk_fma): q = the 16 two-float
// fields of a PairBox, (px, py, pz) the point.  Component i = lower bound of the squared distance to the triangles of pair i:
// the squared distance to the box in its own frame.  No square root; NaN projections (a NaN point) give 0 = "not culled".
typedef float pbf2 __attribute__((ext_vector_type(2)));
template <class Ptr>
__host__ __device__ inline pbf2 pair_box_bound(Ptr q, float px, float py, float pz)
{
    pbf2 bx, by, bz; bx.x = px; bx.y = px; by.x = py; by.y = py; bz.x = pz; bz.y = pz;
    const pbf2 dx = bx - q[0], dy = by - q[1], dz = bz - q[2];
    const pbf2 t0 = __builtin_elementwise_fma(q[5], dz, __builtin_elementwise_fma(q[4], dy, q[3] * dx));
    const pbf2 t1 = __builtin_elementwise_fma(q[8], dz, __builtin_elementwise_fma(q[7], dy, q[6] * dx));
    const pbf2 t2 = __builtin_elementwise_fma(q[11], dz, __builtin_elementwise_fma(q[10], dy, q[9] * dx));
    const pbf2 h0 = q[12], h1 = q[13], h2 = q[14];
    pbf2 e0, e1, e2;
    e0.x = fmaxf(fabsf(t0.x) - h0.x, 0.0f); e0.y = fmaxf(fabsf(t0.y) - h0.y, 0.0f);
    e1.x = fmaxf(fabsf(t1.x) - h1.x, 0.0f); e1.y = fmaxf(fabsf(t1.y) - h1.y, 0.0f);
    e2.x = fmaxf(fabsf(t2.x) - h2.x, 0.0f); e2.y = fmaxf(fabsf(t2.y) - h2.y, 0.0f);
    return __builtin_elementwise_fma(e2, e2, __builtin_elementwise_fma(e1, e1, e0 * e0));
}

// The same records evaluated in HALF units ("box_clamp"): (hx, hy, hz) = the point times 0.5 (exact; the caller holds it per lane),
// every length comes out halved, the result is pair_box_bound / 4.  Halving commutes with every rounding above the subnormal range,
// so while no axis excess passes 2.0 the value is pair_box_bound's divided by 4, bit for bit; an excess beyond 2.0 stops at 1.0 in
// half units and the value is SMALLER than a quarter of pair_box_bound's - the vote `bound' <= thr / 4` culls what `bound <= thr`
// culls, or less (DESIGN.md "BVH conservativeness").  What it is for: both limits of min(max(., 0), 1) are the clamp bit of the
// subtraction that produces the excess (one v_fma_f32 |t'|, h, -0.5 clamp per component instead of v_sub_f32 + v_max_f32).
// NaN projections give 0 like pair_box_bound's: fmaxf(NaN, 0) = 0, and the clamp bit turns NaN into 0 as well.
__host__ __device__ inline float pair_box_excess_half(float t, float h)
{
    return fminf(fmaxf(fmaf(h, -0.5f, fabsf(t)), 0.0f), 1.0f);
}
template <class Ptr>
__host__ __device__ inline pbf2 pair_box_bound_half(Ptr q, float hx, float hy, float hz)
{
    pbf2 bx, by, bz, mh; bx.x = hx; bx.y = hx; by.x = hy; by.y = hy; bz.x = hz; bz.y = hz; mh.x = -0.5f; mh.y = -0.5f;
    const pbf2 dx = __builtin_elementwise_fma(q[0], mh, bx), dy = __builtin_elementwise_fma(q[1], mh, by), dz = __builtin_elementwise_fma(q[2], mh, bz);
    const pbf2 t0 = __builtin_elementwise_fma(q[5], dz, __builtin_elementwise_fma(q[4], dy, q[3] * dx));
    const pbf2 t1 = __builtin_elementwise_fma(q[8], dz, __builtin_elementwise_fma(q[7], dy, q[6] * dx));
    const pbf2 t2 = __builtin_elementwise_fma(q[11], dz, __builtin_elementwise_fma(q[10], dy, q[9] * dx));
    const pbf2 h0 = q[12], h1 = q[13], h2 = q[14];
    pbf2 e0, e1, e2;
    e0.x = pair_box_excess_half(t0.x, h0.x); e0.y = pair_box_excess_half(t0.y, h0.y);
    e1.x = pair_box_excess_half(t1.x, h1.x); e1.y = pair_box_excess_half(t1.y, h1.y);
    e2.x = pair_box_excess_half(t2.x, h2.x); e2.y = pair_box_excess_half(t2.y, h2.y);
    return __builtin_elementwise_fma(e2, e2, __builtin_elementwise_fma(e1, e1, e0 * e0));
}

// ---- arena layout (one device allocation per mesh) ------------------------------------------------------------
constexpr int kTopLevels = 7;          // BVH levels 0..6 are split by multi-workgroup kernels (k_bvh_bin / k_bvh_part)
constexpr int kSubMax = 256;           // subtrees of at most this many triangles are finished by ONE workgroup in LDS (k_bvh_sub)
// (measured on the SMPL-size body, MI355X: 5 levels / 1024 -> k_bvh_sub 257 us, the top levels 75 us; 7 / 256 -> 84 + 122 us:
//  the subtree kernel pays a few microseconds per node PER WAVEFRONT, more, smaller subtrees spread the nodes over more CUs)
constexpr int kChunk = 256;            // triangles per workgroup of the top-level kernels
constexpr int kAdjCap = 16;            // incident (face, corner) entries kept per vertex (more: the vertex scans all faces)
constexpr int kHistWords = 3 * kSahBins * 13;   // per node: [axis][bin][count, lo xyz, hi xyz (triangle boxes), lo xyz, hi xyz (centroids)] as ordered-uint codes
constexpr int kTaskSlots = (1 << (kTopLevels + 1)) - 1;   // task records of levels 0..kTopLevels

struct BTask {                         // one node of the top of the tree while it is being built
    int32_t begin, end, depth, parent, side, kind, buf, from_atomics;
    float box[6], cb[6];               // lo xyz, hi xyz of the triangle boxes / of the centroids
    uint32_t ubox[12];                 // the same as ordered-uint maxima (positional splits: accumulated by every chunk)
};
static_assert(sizeof(BTask) == 128, "BTask layout");

struct BuildHdr {                      // zeroed before every build
    int32_t n_sub;                     // entries of the subtree queue
    int32_t pad[3];
};

struct MeshLayout {
    size_t dyn, hdr, valence, leaf_cnt, tasks, hist, cell_count, cell_cursor, zero_end;   // [dyn, zero_end) is zeroed per build
    size_t vnormals, nodes, leaves, pbox, nbox, tris, attr, slot2face, face2slot, bin_start, bin_slots;
    size_t tbox, cen, order0, order1, adj, chunkcnt, subq, sublist, bounds_part, total;
    int64_t nck;                       // chunk records per top level
};
inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
inline MeshLayout mesh_layout(int64_t V, int64_t F)
{
    MeshLayout L{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes); return at; };
    const int64_t cells = bin_cells_cap(F);
    L.nck = F / kChunk + (1 << kTopLevels) + 2;
    L.dyn = take(sizeof(MeshDyn));
    L.hdr = take(sizeof(BuildHdr));
    L.valence = take(sizeof(int32_t) * V);
    L.leaf_cnt = take((size_t)F);
    L.tasks = take(sizeof(BTask) * kTaskSlots);
    L.hist = take(sizeof(uint32_t) * kHistWords * ((1 << kTopLevels) - 1));
    L.cell_count = take(sizeof(int32_t) * (cells + 1));
    L.cell_cursor = take(sizeof(int32_t) * cells);
    L.zero_end = o;
    L.vnormals = take(sizeof(float) * 3 * V);
    L.nodes = take(sizeof(BvhNode) * F);
    L.leaves = take(sizeof(LeafRec) * F);
    L.pbox = take(sizeof(PairBox) * F);                        // behind the leaves it is indexed like (icon_debug_mesh_layout: part of entry 3's range)
    L.nbox = take(sizeof(PairBox) * F);                        // the node boxes, indexed by node id (part of entry 3's range as well)
    L.tris = take(sizeof(TriRec) * F);
    L.attr = take(sizeof(TriAttr) * F);
    L.slot2face = take(sizeof(int32_t) * F);
    L.face2slot = take(sizeof(int32_t) * F);
    L.bin_start = take(sizeof(int32_t) * (cells + 1));
    L.bin_slots = take(sizeof(int32_t) * bin_entries_cap(F));
    L.tbox = take(sizeof(float) * 6 * F);
    L.cen = take(sizeof(float) * 3 * F);
    L.order0 = take(sizeof(int32_t) * F);
    L.order1 = take(sizeof(int32_t) * F);
    L.adj = take(sizeof(int32_t) * kAdjCap * V);
    L.chunkcnt = take(sizeof(int32_t) * 3 * kSahBins * L.nck * kTopLevels);
    L.subq = take(sizeof(int32_t) * (kTaskSlots + 1));
    L.sublist = take((size_t)80 * 2 * (F / 5 + 4));            // task lists of subtrees too large for LDS (mesh_device.hip: STask, 80 B)
    L.bounds_part = take(sizeof(uint32_t) * 12 * ((size_t)F / 256 + 1));   // per-workgroup mesh bounds of k_face_prep
    L.total = o;
    return L;
}

}  // namespace icon

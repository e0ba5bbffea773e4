// raster_gl_device.h - the raster rule of the reference's EVALUATOR, stated once for evaluator.hip:
// lib/renderer/gl/normal_render.py + render2.py + data/normal.vs/.fs as lib/dataset/Evaluator.py drives them (one sample per pixel,
// GL_LESS depth test, clear colour (1,1,1,0)), and trimesh's angle-weighted vertex_normals.  PARITY UNPINNED, like 4.13: neither
// OpenGL nor trimesh is installed where this was written - the rasteriser is restated from the OpenGL specification's rules
// (fixed-point snapping, top-left fill rule), trimesh's normals FROM MEMORY.  It is NOT raster_device.h's pytorch3d rule: no blur
// radius, no clamped barycentrics, near / far clipping, another background, another vertex normal.
//   A view carries a float32 affine model matrix M [3][4] (row-major) and a float32 normal multiplier [3].  Per vertex, float32,
//   in this order:  p_r = ((M_r0 x + M_r1 y) + M_r2 z) + M_r3;  clip = (p_0, p_1, -p_2)  (the evaluator passes a view matrix with
//   [2][2] = -1 as the projection);  camera normal n'_r = ((M_r0 nx + M_r1 ny) + M_r2 nz) * mul_r.
//   Coverage is decided in exact integers, as rasterising hardware decides it: a vertex snaps to 1/256 pixel,
//   xi = rint(((double)x * 0.5 + 0.5) * (256 S)) (ties to even), yi likewise with y UP; pixel (column c, window row w) has its
//   centre at (256 c + 128, 256 w + 128).  A2 = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) in int64; a face is drawn when A2 != 0 (no
//   culling); corners 1 and 2 change places when A2 < 0, so that the corners run counter-clockwise.  For the edge a -> b,
//   d = b - a: E = d.x (p.y - a.y) - d.y (p.x - a.x); the centre is covered when every E > 0, or E = 0 on an edge with d.y < 0 or
//   (d.y = 0 and d.x < 0) - every point of a shared edge or vertex belongs to exactly one of the faces around it.
//   A face with a clip x or y that is not finite or above 64 in magnitude is NOT DRAWN (OpenGL would clip it); S <= 2048, so every
//   product above stays below 2^53.
//   Fragment: b_k = (float)((double)E_k / (double)A2), E_k the edge opposite corner k; z = (b0 z0 + b1 z1) + b2 z2, kept iff
//   -1 <= z <= 1; the smallest (z, face id) wins a pixel (GL_LESS, faces drawn in index order; -0 counts as +0).
//   Colour: c = (b0 n'0 + b1 n'1) + b2 n'2 per component, len = sqrt((cx cx + cy cy) + cz cz), rgb = (c / len + 1) * 0.5 (0.5 when
//   len = 0), alpha 1; background (1, 1, 1, 0).  Image row r is window row S - 1 - r.
//   Vertex normals when the caller gives none: float64 throughout; per incidence key 3 face + corner, ascending: (corner angle) x
//   (unit face normal), the face normal (v1 - v0) x (v2 - v0) over its length (a face whose length is not > 0 adds nothing), the
//   angle acos of the clamped dot product of the two unit edge vectors leaving the corner; the sum over its length where that is
//   > 0, else 0; rounded once to float32.
// Everything lives in the including file's anonymous namespace, is forced inline and keeps the order its expression is evaluated in
// (compiled with -ffp-contract=off); tests/gl_checker.py states the same expressions in numpy.
#pragma once
#pragma clang fp contract(off)

#include "raster_device.h"

namespace icon {
namespace {

constexpr float kGlGuard = 64.0f;    // a face with a larger |clip x| or |clip y| is not drawn

struct GlView { float m[12], mul[3]; };

__device__ __forceinline__ GlView gl_view(const float *mats, const float *muls, int view)
{
    GlView w;
#pragma unroll
    for (int i = 0; i < 12; ++i) w.m[i] = mats[12 * view + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) w.mul[i] = muls[3 * view + i];
    return w;
}

__device__ __forceinline__ void gl_clip(const GlView &w, const float *p, float c[3])
{
    c[0] = ((w.m[0] * p[0] + w.m[1] * p[1]) + w.m[2] * p[2]) + w.m[3];
    c[1] = ((w.m[4] * p[0] + w.m[5] * p[1]) + w.m[6] * p[2]) + w.m[7];
    c[2] = -(((w.m[8] * p[0] + w.m[9] * p[1]) + w.m[10] * p[2]) + w.m[11]);
}
__device__ __forceinline__ void gl_cam_normal(const GlView &w, const float *n, float o[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = ((w.m[4 * r] * n[0] + w.m[4 * r + 1] * n[1]) + w.m[4 * r + 2] * n[2]) * w.mul[r];
}

// |v| <= kGlGuard: at most 32.5 * 256 * 2048 < 2^25
__device__ __forceinline__ int64_t gl_snap(float v, int S) { return (int64_t)rint(((double)v * 0.5 + 0.5) * (double)(256 * S)); }

// a face as a view sees it: snapped corners (counter-clockwise), their clip z, the doubled area, the pixel box (i: column, j: window row)
struct GlFace {
    int64_t id[3], x[3], y[3], A2;
    float z[3];
    RsBox box;
};
// after id is filled (every id a vertex of `verts`).  false: nothing to rasterise
__device__ __forceinline__ bool gl_setup(const float *verts, const GlView &w, int S, GlFace &r)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float c[3];
        gl_clip(w, verts + 3 * r.id[k], c);
        if (!(fabsf(c[0]) <= kGlGuard && fabsf(c[1]) <= kGlGuard)) return false;          // NaN and inf fail too
        r.x[k] = gl_snap(c[0], S); r.y[k] = gl_snap(c[1], S); r.z[k] = c[2];
    }
    r.A2 = (r.x[1] - r.x[0]) * (r.y[2] - r.y[0]) - (r.y[1] - r.y[0]) * (r.x[2] - r.x[0]);
    if (r.A2 == 0) return false;
    if (r.A2 < 0) {
        const int64_t ti = r.id[1], tx = r.x[1], ty = r.y[1];
        const float tz = r.z[1];
        r.id[1] = r.id[2]; r.x[1] = r.x[2]; r.y[1] = r.y[2]; r.z[1] = r.z[2];
        r.id[2] = ti; r.x[2] = tx; r.y[2] = ty; r.z[2] = tz;
        r.A2 = -r.A2;
    }
    const int64_t xlo = min(r.x[0], min(r.x[1], r.x[2])), xhi = max(r.x[0], max(r.x[1], r.x[2]));
    const int64_t ylo = min(r.y[0], min(r.y[1], r.y[2])), yhi = max(r.y[0], max(r.y[1], r.y[2]));
    // centres 256 c + 128 inside [lo, hi]: ceil((lo - 128) / 256) <= c <= floor((hi - 128) / 256), clamped to the image as int64
    r.box.i0 = (int)max((int64_t)0, (xlo + 127) >> 8); r.box.i1 = (int)min((int64_t)S - 1, (xhi - 128) >> 8);
    r.box.j0 = (int)max((int64_t)0, (ylo + 127) >> 8); r.box.j1 = (int)min((int64_t)S - 1, (yhi - 128) >> 8);
    return !r.box.empty();
}

// the edge a -> b at p: its function E, and whether p is on the face's side of it by the fill rule
__device__ __forceinline__ bool gl_edge(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py, int64_t &E)
{
    const int64_t dx = bx - ax, dy = by - ay;
    E = dx * (py - ay) - dy * (px - ax);
    return E > 0 || (E == 0 && (dy < 0 || (dy == 0 && dx < 0)));
}

struct GlFrag { float b[3], z; };
// the fragment of face r at pixel (column c, window row w); false: not covered, or clipped by the near / far planes
__device__ __forceinline__ bool gl_fragment(const GlFace &r, int c, int w, GlFrag &q)
{
    const int64_t px = 256 * (int64_t)c + 128, py = 256 * (int64_t)w + 128;
    int64_t E0, E1, E2;
    const bool in0 = gl_edge(r.x[1], r.y[1], r.x[2], r.y[2], px, py, E0);
    const bool in1 = gl_edge(r.x[2], r.y[2], r.x[0], r.y[0], px, py, E1);
    const bool in2 = gl_edge(r.x[0], r.y[0], r.x[1], r.y[1], px, py, E2);
    if (!(in0 && in1 && in2)) return false;
    const double a2 = (double)r.A2;
    q.b[0] = (float)((double)E0 / a2); q.b[1] = (float)((double)E1 / a2); q.b[2] = (float)((double)E2 / a2);
    q.z = (q.b[0] * r.z[0] + q.b[1] * r.z[1]) + q.b[2] * r.z[2];
    if (!(q.z >= -1.0f && q.z <= 1.0f)) return false;
    if (q.z == 0.0f) q.z = 0.0f;                                       // -0 and +0 are one depth
    return true;
}
// (z, face id) as one word whose unsigned order is the pair's
__device__ __forceinline__ unsigned long long gl_key(float z, int64_t f)
{
    const uint32_t u = __float_as_uint(z);
    const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)o << 32) | (unsigned long long)(uint32_t)f;
}

// the winner's colour from its corners' vertex normals
__device__ __forceinline__ void gl_colour(const GlView &w, const GlFrag &q, const float *n0, const float *n1, const float *n2, float rgba[4])
{
    float a[3], b[3], d[3], c[3];
    gl_cam_normal(w, n0, a); gl_cam_normal(w, n1, b); gl_cam_normal(w, n2, d);
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = (q.b[0] * a[i] + q.b[1] * b[i]) + q.b[2] * d[i];
    const float len = sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) rgba[i] = (len == 0.0f) ? 0.5f : (c[i] / len + 1.0f) * 0.5f;
    rgba[3] = 1.0f;
}

// the addend of a face (corners pa, pb, pc as given) to the angle-weighted normal of its corner `corner`: angle x unit face normal
__device__ __forceinline__ void gl_angle_term(const float *pa, const float *pb, const float *pc, int corner, double o[3])
{
    double e01[3], e02[3], e12[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        e01[i] = (double)pb[i] - (double)pa[i]; e02[i] = (double)pc[i] - (double)pa[i]; e12[i] = (double)pc[i] - (double)pb[i];
    }
    const double cx = e01[1] * e02[2] - e01[2] * e02[1], cy = e01[2] * e02[0] - e01[0] * e02[2], cz = e01[0] * e02[1] - e01[1] * e02[0];
    const double L = sqrt((cx * cx + cy * cy) + cz * cz);
    o[0] = o[1] = o[2] = 0.0;
    if (!(L > 0.0)) return;
    const double l01 = sqrt((e01[0] * e01[0] + e01[1] * e01[1]) + e01[2] * e01[2]);
    const double l02 = sqrt((e02[0] * e02[0] + e02[1] * e02[1]) + e02[2] * e02[2]);
    const double l12 = sqrt((e12[0] * e12[0] + e12[1] * e12[1]) + e12[2] * e12[2]);
    double u[3], v[3];                                                  // the two unit edges of the corner (signs: see below)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        u[i] = corner == 2 ? e02[i] / l02 : e01[i] / l01;
        v[i] = corner == 0 ? e02[i] / l02 : e12[i] / l12;
    }
    double dot = (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
    if (corner == 1) dot = -dot;                                        // corner 1 leaves along -e01 and +e12
    dot = dot > 1.0 ? 1.0 : (dot < -1.0 ? -1.0 : dot);
    const double ang = acos(dot);
    o[0] = ang * (cx / L); o[1] = ang * (cy / L); o[2] = ang * (cz / L);
}

// sum / |sum| where |sum| > 0, else 0; rounded once
__device__ __forceinline__ void gl_store_normal(float *nrm, int64_t v, double x, double y, double z)
{
    const double len = sqrt((x * x + y * y) + z * z);
    if (len > 0.0) { x = x / len; y = y / len; z = z / len; } else { x = y = z = 0.0; }
    nrm[3 * v] = (float)x; nrm[3 * v + 1] = (float)y; nrm[3 * v + 2] = (float)z;
}

}  // namespace
}  // namespace icon

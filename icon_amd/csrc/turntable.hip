// turntable.hip - the frames of ICON's turntable video: normal maps of a mesh from a camera at any azimuth, as video bytes
// (lib/common/render.py:327-374 Render.get_rendered_video: 360 cameras on a circle around the y axis, one pytorch3d render per
// camera and mesh, each ending in .detach().cpu().numpy(); call site apps/infer.py:547-563, --export_video).
//
// The rule (PARITY UNPINNED like 4.13): the camera of azimuth a has its eye at (100 cos a, 0, 100 sin a), looks at the
// origin with +y up, under the FoVOrthographicCameras(+-100, scale 100) of the four fixed cameras.  With (cs, sn) the float32 pair of
// a (icon_amd.render.turntable_cos_sin; exact at whole multiples of 90 degrees):  X = z cs - x sn,  Y = y,  D = (100 - x cs) - z sn
// (raster_device.h rs_project_turn).  Everything after the projection is render_normal.hip's rule, raster_device.h's rs_normal_*:
// pixel centres, |area| > 1e-8, the box grown by the blur radius, the candidate test, the winner of smallest (depth bits, face id), the
// S1 vertex normals; no view is mirrored.  A frame's byte per channel: t = (b0 t0 + b1 t1) + b2 t2, t_k = (n_k + 1) * 0.5,
// (uint8) min(max(t * 255, 0), 255) - truncated, as astype(np.uint8) does; background 127; channels in the normal's x, y, z order.
// tests/turntable_checker.py states the same expressions in numpy; faces, depths, colours and bytes are compared for equality.
//
// Shape of the work: one stream-ordered call of kernel launches only, every buffer in the caller's scratch
// (icon_render_turntable_bytes); nothing is allocated, read back or waited for.  The S1 normals are computed ONCE per call.  The
// views are then taken in chunks of kTtChunk ("tt_chunk"): the z-buffer and the deferred lists exist for one chunk only, so the
// scratch does not grow with the number of frames.  Per chunk three launches: the raster sweep (blockIdx.y: the view of the chunk),
// the deferred faces (one list per view), and the resolve pass - which writes the frame's bytes into the caller's canvas and hands
// the z-buffer and the lists' lengths back CLEARED, so that the next chunk starts without a clear pass of its own.
// The resolve pass: a lane owns four neighbouring pixels of a row, chosen so that their 12 bytes in the canvas start on a dword
// boundary whatever the canvas' width and the panel's column are, and stores them as three dwords; the up to three pixels before the
// first such group of a row, and those after the last, are stored byte by byte.  The float planes are written only when asked for.
#pragma clang fp contract(off)

#include "raster_device.h"

namespace icon {

int g_tt_chunk = 0;       // icon_debug_set_option("tt_chunk"): 0 = kTtChunk; 1..32 = that many views per chunk

namespace {

constexpr int kTtChunk = 32;         // views per chunk: 64 MiB of z-buffer at 512^2 - the largest allowed measured fastest
constexpr int kTtMaxChunk = 32;
constexpr int kTtMaxViews = 1024;

// the first 256 bytes of the scratch (s1_layout's header piece, inside what the call's clear sets to 0): S1's counters, then the
// length of each view's deferred list
struct TtHdr { S1Hdr s1; int n_big[kTtMaxChunk]; };
static_assert(sizeof(TtHdr) <= 256, "the header piece of s1_layout is 256 bytes");

struct TtCtx : RsCtx {               // n_views: the call's; cams / flip are not used.  vis null: every vertex gets a normal
    const float *cos_sin;            // [n_views][2]
    int v0, nc;                      // the chunk: views v0 .. v0 + nc - 1
    int *n_big, *big;                // the deferred lists (raster_device.h rs_defer_view) [chunk][F] and their lengths [chunk]
    float *nrm;                      // [V][3] S1 normals
    unsigned long long *zb;          // [chunk][S][S], image orientation; all ~0 between the chunks
    uint8_t *canvas;                 // [n_views][S][W][3], the panel at column x0 - or null
    int64_t W, x0;
    float *images, *depth; int *pix; // as render_normal.hip's, each may be null
};

// face f as the camera of view `view` (of the call) sees it.  false: nothing to rasterise
template <class IT>
__device__ __forceinline__ bool tt_setup(const TtCtx &c, int view, int64_t f, RsNormalFace &r)
{
    if (!s1_face<IT>(c, f, r.id)) return false;
    rs_project_turn(c, c.cos_sin[2 * view], c.cos_sin[2 * view + 1], r.id, r.X, r.Y, r.D);
    return rs_normal_setup(r, c.S);
}

__device__ __forceinline__ unsigned long long *tt_plane(const TtCtx &c, int lv) { return c.zb + (size_t)lv * c.S * c.S; }

// G lanes per face, 256 / G faces per workgroup; blockIdx.y: the view of the chunk
template <class IT, int G>
__global__ __launch_bounds__(256) void k_tt_raster(TtCtx c)
{
    const int64_t f = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x % G;
    const int lv = blockIdx.y;
    if (f >= c.F || lv >= c.nc) return;
    RsNormalFace r;
    if (!tt_setup<IT>(c, c.v0 + lv, f, r)) return;
    if (r.box.n() > kRsBigPerLane * G) {
        if (sub == 0) rs_defer_view(c.n_big, c.big, c.F, lv, f);
        return;
    }
    unsigned long long *zb = tt_plane(c, lv);
    rs_sweep<G>(r.box, sub, [&](int i, int j) { rs_normal_pixel(zb, c.S, r, f, i, j); });
}

// the deferred faces of view blockIdx.y: a workgroup per entry, as many rounds as the list (read from device memory) needs
template <class IT>
__global__ __launch_bounds__(256) void k_tt_raster_big(TtCtx c)
{
    const int lv = blockIdx.y;
    if (lv >= c.nc) return;
    const int nb = rs_deferred_view_count(c.n_big, c.F, lv);
    unsigned long long *zb = tt_plane(c, lv);
    for (int e = blockIdx.x; e < nb; e += gridDim.x) {
        int64_t f;
        RsNormalFace r;
        if (!rs_deferred_view(c.big, c.F, lv, e, f) || !tt_setup<IT>(c, c.v0 + lv, f, r)) continue;
        rs_sweep_block(r.box, [&](int i, int j) { rs_normal_pixel(zb, c.S, r, f, i, j); });
    }
}

__device__ __forceinline__ uint32_t tt_byte(float t) { return (uint32_t)(uint8_t)fminf(fmaxf(t * 255.0f, 0.0f), 255.0f); }

struct TtDwords { uint32_t w[3]; };  // four pixels of a frame

// lanes of a row: the (up to three) pixels before the first dword-aligned group, then the groups of four, the last one short
__device__ __host__ __forceinline__ int tt_row_lanes(int S) { return (S + 3) / 4 + 1; }

// one lane per group of four pixels of a row; blockIdx.y: the view of the chunk
template <class IT>
__global__ __launch_bounds__(256) void k_tt_resolve(TtCtx c)
{
    const int lpr = tt_row_lanes(c.S), npx = c.S * c.S;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int lv = blockIdx.y;
    if (lv >= c.nc) return;
    if (t == 0) c.n_big[lv] = 0;                                             // every list of the chunk has been consumed
    if (t >= c.S * lpr) return;
    const int view = c.v0 + lv;
    const int row = t / lpr, g = t - row * lpr;
    uint8_t *line = c.canvas ? c.canvas + (((size_t)view * c.S + row) * (size_t)c.W + (size_t)c.x0) * 3 : nullptr;
    // the address of pixel k is line + 3 k: a multiple of 4 exactly when k = line (mod 4)
    const int p0 = (int)((uintptr_t)line & 3) + 4 * (g - 1);
    const int lo = p0 < 0 ? 0 : p0, hi = p0 + 4 < c.S ? p0 + 4 : c.S;
    if (lo >= hi) return;
    unsigned long long *zb = tt_plane(c, lv) + (size_t)row * c.S;
    const int j = c.S - 1 - row;
    TtDwords out = { { 0u, 0u, 0u } };
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int col = p0 + k;
        if (col < lo || col >= hi) continue;
        const int i = c.S - 1 - col;
        const unsigned long long key = zb[col];
        zb[col] = ~0ull;                                                     // the next chunk's clear
        const int64_t f = (int64_t)(uint32_t)(key & 0xffffffffull);
        float tx[3] = { 0.5f, 0.5f, 0.5f }, pz = -1.0f;
        int face = -1;
        RsNormalFace r;
        RsBary q;
        // a face in the z-buffer passed tt_setup and rs_normal_eval at this pixel: the same expressions give the same answer
        if (key != ~0ull && f < c.F && tt_setup<IT>(c, view, f, r) && rs_normal_eval(r, rs_centre(i, c.S), rs_centre(j, c.S), q, pz)) {
            face = (int)f;
            const float *n0 = c.nrm + 3 * r.id[0], *n1 = c.nrm + 3 * r.id[1], *n2 = c.nrm + 3 * r.id[2];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) tx[ch] = rs_normal_texel(q, n0, n1, n2, ch);
        } else {
            pz = -1.0f;
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out.w[(3 * k + ch) >> 2] |= tt_byte(tx[ch]) << (8 * ((3 * k + ch) & 3));
        const size_t at = (size_t)row * c.S + col;
        if (c.images) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c.images[((size_t)view * 3 + ch) * npx + at] = (tx[ch] - 0.5f) * 2.0f;
        }
        if (c.depth) c.depth[(size_t)view * npx + at] = pz;
        if (c.pix) c.pix[(size_t)view * npx + at] = face;
    }
    if (!line) return;
    if (hi - lo == 4) {
        *reinterpret_cast<TtDwords *>(line + 3 * (size_t)p0) = out;          // dword-aligned by the choice of p0
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int col = p0 + k;
            if (col < lo || col >= hi) continue;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) line[3 * (size_t)col + ch] = (uint8_t)(out.w[(3 * k + ch) >> 2] >> (8 * ((3 * k + ch) & 3)));
        }
    }
}

// a normal into the scratch: n = s / max(|s|, 1e-6)
struct TtStore {
    float *nrm;
    __device__ void operator()(int64_t v, float x, float y, float z) const
    {
        s1_normalise(x, y, z);
        nrm[3 * v] = x; nrm[3 * v + 1] = y; nrm[3 * v + 2] = z;
    }
};

// one thread per vertex: the normal of a short incidence list; a long one goes to k_s1_normals_long's list
template <class IT>
__global__ __launch_bounds__(256) void k_tt_normals(TtCtx c)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= c.V) return;
    const int n = c.deg[v];
    if (n > kShort) { s1_defer_long(c, v); return; }
    float s[3];
    s1_sum_short<IT>(c, v, n, s);
    TtStore{c.nrm}(v, s[0], s[1], s[2]);
}

// views per chunk of a call of n_views
int tt_chunk(int n_views)
{
    const int k = g_tt_chunk ? g_tt_chunk : kTtChunk;
    return k < n_views ? k : n_views;
}

struct TtLayout { S1Layout s1; size_t nrm, zb, total; };            // the deferred lists: s1.mid

TtLayout tt_layout(int64_t V, int64_t F, int S, int chunk)
{
    TtLayout L{};
    ScratchTake take;
    L.s1 = s1_layout(take, V, F, (size_t)F * 4 * chunk);
    L.nrm = take((size_t)V * 12);
    L.zb = take((size_t)chunk * S * S * 8);
    L.total = take.o;
    return L;
}

template <class IT>
void tt_launch(TtCtx c, int chunk, hipStream_t st)
{
    const S1Ctx &s1 = c;                                                   // the shared kernels take the base alone
    s1_launch_lists<IT>(s1, st);
    hipLaunchKernelGGL(k_tt_normals<IT>, dim3((unsigned)((c.V + 255) / 256)), dim3(256), 0, st, c);
    hipLaunchKernelGGL((k_s1_normals_long<IT, TtStore>), dim3(kLongGrid), dim3(64), 0, st, s1, TtStore{c.nrm});
    const int lanes = rs_lanes(c);
    for (c.v0 = 0; c.v0 < c.n_views; c.v0 += chunk) {
        c.nc = c.n_views - c.v0 < chunk ? c.n_views - c.v0 : chunk;
        const dim3 gR((unsigned)((c.F * lanes + 255) / 256), (unsigned)c.nc);
        if (lanes == 1) hipLaunchKernelGGL((k_tt_raster<IT, 1>), gR, dim3(256), 0, st, c);
        else hipLaunchKernelGGL((k_tt_raster<IT, 8>), gR, dim3(256), 0, st, c);
        hipLaunchKernelGGL(k_tt_raster_big<IT>, dim3((unsigned)((kRsBigGrid + c.nc - 1) / c.nc), (unsigned)c.nc), dim3(256), 0, st, c);
        hipLaunchKernelGGL(k_tt_resolve<IT>, dim3((unsigned)((c.S * tt_row_lanes(c.S) + 255) / 256), (unsigned)c.nc), dim3(256), 0, st, c);
    }
}

}  // namespace
}  // namespace icon

using namespace icon;

extern "C" int icon_render_turntable_bytes(int64_t V, int64_t F, int size, int n_views, int64_t *bytes)
{
    ICON_ARG(bytes != nullptr, "icon_render_turntable_bytes: null argument");
    const int rc = rs_check_sizes("icon_render_turntable", V, F, size, n_views, kTtMaxViews);
    if (rc) return rc;
    *bytes = (int64_t)tt_layout(V, F, size, tt_chunk(n_views)).total;
    return ICON_OK;
}

extern "C" int icon_render_turntable(const float *d_verts, int64_t V, const void *d_faces, int64_t F, int faces_int64,
                                     const float *d_cos_sin, int n_views, int size, uint8_t *d_canvas, int64_t canvas_width, int64_t x0,
                                     float *d_images, float *d_depth, int32_t *d_pix_to_face,
                                     void *d_scratch, int64_t scratch_bytes, void *stream)
{
    ICON_ARG(d_verts && d_faces && d_cos_sin && d_scratch, "icon_render_turntable: null argument");
    ICON_ARG(d_canvas || d_images, "icon_render_turntable: null argument (d_canvas and d_images are both null)");
    const int rc = rs_check_sizes("icon_render_turntable", V, F, size, n_views, kTtMaxViews);
    if (rc) return rc;
    ICON_ARG(!d_canvas || (x0 >= 0 && canvas_width <= (1ll << 31) && x0 + size <= canvas_width),
             "icon_render_turntable: the panel must lie inside the canvas: 0 <= x0, x0 + size <= canvas_width <= 2^31");
    const int chunk = tt_chunk(n_views);
    const TtLayout L = tt_layout(V, F, size, chunk);
    if (const int e = scratch_check("icon_render_turntable", "icon_render_turntable_bytes", d_scratch, scratch_bytes, L.total)) return e;
    hipStream_t st = (hipStream_t)stream;
    char *s = static_cast<char *>(d_scratch);
    TtCtx c{};
    c.verts = d_verts; c.faces = d_faces; c.V = V; c.F = F; c.S = size; c.n_views = n_views;
    c.cos_sin = d_cos_sin; c.canvas = d_canvas; c.W = canvas_width; c.x0 = x0;
    c.images = d_images; c.depth = d_depth; c.pix = d_pix_to_face;
    s1_bind(c, s, L.s1);
    c.n_big = reinterpret_cast<TtHdr *>(s + L.s1.hdr)->n_big; c.big = reinterpret_cast<int *>(s + L.s1.mid);
    c.nrm = reinterpret_cast<float *>(s + L.nrm); c.zb = reinterpret_cast<unsigned long long *>(s + L.zb);
    rs_clear(s, L.s1, c.zb, (size_t)chunk * size * size, st);
    if (faces_int64) tt_launch<int64_t>(c, chunk, st); else tt_launch<int32_t>(c, chunk, st);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

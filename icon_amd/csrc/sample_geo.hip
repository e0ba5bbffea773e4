// sample_geo.hip - the training samples of PIFuDataset.get_sampling_geo (lib/dataset/PIFuDataset.py:483-607, is_sdf=False) on
// the device: surface samples along the vertex normals, uniform samples of the image cube, z-ray samples, shuffled, labelled by
// the library's inside test of the scan and truncated to balanced labels.  The rule is DESIGN.md 4.21, restated in numpy by
// tests/sampling_oracle.py.
//
// Every draw is a pure function of (seed, stream, index): Philox4x32-10 keyed by the seed, one stream per kind of draw, and the
// shuffle is a keyed bijection (a balanced Feistel network with cycle walking) that a lane evaluates for its own slot - no
// sort, no second buffer, and a z-ray lane recomputes the surface sample it perturbs from the same counters.  The arithmetic
// is float64 in the stated operation order, rounded once to float32 (this file is compiled with -ffp-contract=off).
//
// Three launches: k_sg_draw (a lane per slot of the shuffled list), k_sg_inside (the ray-parity test of geom_device.h, as
// icon_sdf_query runs it) and k_sg_balance (one workgroup: the stable ranks of scan_device.h give the output row directly).
#pragma clang fp contract(off)

#include "query_device.h"
#include "scan_device.h"

namespace icon {
namespace {

constexpr int kSgBlock = 256;
constexpr int kSgScanThreads = 1024, kSgScanWaves = kSgScanThreads / 64, kSgItems = 8;    // a round of the balancing scan: 8,192 slots
constexpr int kSgFeistelRounds = 4;
enum : uint32_t { kSgVertex = 0, kSgOffset = 1, kSgSpace = 2, kSgZNoise = 3, kSgPerm = 4 };   // the streams
constexpr double kSgZScale = 0.40, kSgZThickness = 0.5;                                     // PIFuDataset.py:529-538

struct SgParams {
    const float *verts, *normals;      // [V,3]
    int64_t V, N, nS, nU, n;
    int R, half_bits;                  // z-ray samples per surface sample; half the Feistel width
    double sigma;
    double calib[12], calib_inv[12];   // rows of [3][4]
    uint64_t seed;
};

struct U64x2 { uint64_t x0, x1; };

// Philox4x32-10 (Salmon et al., SC'11): key = the seed, counter = (index low, index high, stream, 0)
__device__ __forceinline__ U64x2 philox(uint64_t seed, uint64_t index, uint32_t stream)
{
    uint32_t c0 = (uint32_t)index, c1 = (uint32_t)(index >> 32), c2 = stream, c3 = 0;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return {(uint64_t)c0 | ((uint64_t)c1 << 32), (uint64_t)c2 | ((uint64_t)c3 << 32)};
}

__device__ __forceinline__ double sg_uniform(uint64_t x) { return ((double)(x >> 11) + 0.5) * 0x1p-53; }

// Box-Muller, the cosine branch
__device__ __forceinline__ double sg_normal(U64x2 x)
{
    return sqrt(-2.0 * log(sg_uniform(x.x0))) * cos(6.283185307179586 * sg_uniform(x.x1));
}

// slot -> source: kSgFeistelRounds rounds (L, R) -> (R, L ^ F_r(R)) over 2 * half_bits bits; a value >= n walks on
__device__ __forceinline__ int64_t sg_perm(const SgParams &p, int64_t slot)
{
    const uint64_t mask = (1ull << p.half_bits) - 1ull;
    uint64_t x = (uint64_t)slot;
    do {
        uint64_t l = x >> p.half_bits, r = x & mask;
        for (int q = 0; q < kSgFeistelRounds; ++q) {
            const uint64_t f = philox(p.seed, ((uint64_t)q << 32) | r, kSgPerm).x0 & mask;
            const uint64_t t = l ^ f;
            l = r; r = t;
        }
        x = (l << p.half_bits) | r;
    } while (x >= (uint64_t)p.n);
    return (int64_t)x;
}

struct d3 { double x, y, z; };

__device__ __forceinline__ d3 sg_project(const double *m, d3 p)
{
    return {((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3], ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7],
            ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11]};
}

__device__ __forceinline__ d3 sg_surface(const SgParams &p, int64_t j, int64_t &id)
{
    id = (int64_t)__umul64hi(philox(p.seed, (uint64_t)j, kSgVertex).x0, (uint64_t)p.V);
    const double off = p.sigma * sg_normal(philox(p.seed, (uint64_t)j, kSgOffset));
    const float *v = p.verts + 3 * id, *nv = p.normals + 3 * id;
    return {(double)v[0] + (double)nv[0] * off, (double)v[1] + (double)nv[1] * off, (double)v[2] + (double)nv[2] * off};
}

__global__ __launch_bounds__(kSgBlock) void k_sg_draw(SgParams p, float *__restrict__ all, int32_t *__restrict__ out_source,
                                                      int32_t *__restrict__ out_vertex)
{
    const int64_t i = (int64_t)blockIdx.x * kSgBlock + threadIdx.x;
    if (i >= p.n) return;
    const int64_t s = sg_perm(p, i);
    int64_t id = -1;
    d3 x;
    if (s >= p.nS && s < p.nS + p.nU) {
        const uint64_t j = (uint64_t)(s - p.nS);
        const d3 u = {sg_uniform(philox(p.seed, 3 * j, kSgSpace).x0), sg_uniform(philox(p.seed, 3 * j + 1, kSgSpace).x0),
                      sg_uniform(philox(p.seed, 3 * j + 2, kSgSpace).x0)};
        x = sg_project(p.calib_inv, {2.0 * u.x - 1.0, 2.0 * u.y - 1.0, 2.0 * u.z - 1.0});
    } else {
        const bool zray = s >= p.nS;
        const int64_t k = zray ? s - p.nS - p.nU : 0;
        x = sg_surface(p, zray ? k / p.R : s, id);
        if (zray) {
            d3 c = sg_project(p.calib, x);
            c.z = c.z + kSgZThickness * (kSgZScale * sg_normal(philox(p.seed, (uint64_t)k, kSgZNoise)));
            x = sg_project(p.calib_inv, c);
        }
    }
    all[3 * i] = (float)x.x; all[3 * i + 1] = (float)x.y; all[3 * i + 2] = (float)x.z;
    if (out_source) out_source[i] = (int32_t)s;
    if (out_vertex) out_vertex[i] = (int32_t)id;
}

// the labels: check_sign's rule on the float32 samples, the test k_sdf_query runs per point
__global__ __launch_bounds__(kSgBlock) void k_sg_inside(MeshDev m, const float *__restrict__ all, int64_t n, uint8_t *__restrict__ inside)
{
    const int64_t i = (int64_t)blockIdx.x * kSgBlock + threadIdx.x;
    if (i >= n) return;
    inside[i] = inside_bins(m, clamp_raw(mk3(all[3 * i], all[3 * i + 1], all[3 * i + 2]))) ? 1 : 0;
}

// PIFuDataset.py:562-599 in one workgroup: count the inside flags, then one stable scan of them - slot i is the rank-th inside
// (or i - rank-th outside) sample of the shuffled list, which is its output row when it is kept.  Rounds of 8,192 slots carry the
// running count; the loop ends as soon as both halves are full.
__global__ __launch_bounds__(kSgScanThreads) void k_sg_balance(const float *__restrict__ all, const uint8_t *__restrict__ inside, int64_t n,
                                                               int64_t N, float *__restrict__ samples, float *__restrict__ labels,
                                                               int32_t *__restrict__ counts)
{
    __shared__ int s_w[kSgScanWaves];
    int mine = 0, n_in;
    for (int64_t i = threadIdx.x; i < n; i += kSgScanThreads) mine += inside[i];
    (void)block_excl_scan<kSgScanWaves>(mine, s_w, n_in);
    const int64_t half = N / 2, n_out = n - n_in;
    const int64_t kin = n_in > half ? half : n_in;
    const int64_t want_out = n_in > half ? half : N - n_in;
    const int64_t kout = want_out < n_out ? want_out : n_out;
    int carry = 0;                                               // inside flags before this round
    for (int64_t base = 0; base < n && (carry < kin || base - carry < kout); base += kSgScanThreads * kSgItems) {
        const int64_t i0 = base + (int64_t)threadIdx.x * kSgItems;
        int flag[kSgItems], sum = 0, total;
#pragma unroll
        for (int k = 0; k < kSgItems; ++k) { flag[k] = i0 + k < n ? inside[i0 + k] : 0; sum += flag[k]; }
        __syncthreads();                                         // (the previous scan's s_w has been read)
        int run = carry + block_excl_scan<kSgScanWaves>(sum, s_w, total);
#pragma unroll
        for (int k = 0; k < kSgItems; ++k) {
            const int64_t i = i0 + k;
            if (i < n) {
                const int64_t rank = flag[k] ? run : i - run;
                if (rank < (flag[k] ? kin : kout)) {
                    const int64_t row = flag[k] ? rank : kin + rank;
                    samples[3 * row] = all[3 * i]; samples[3 * row + 1] = all[3 * i + 1]; samples[3 * row + 2] = all[3 * i + 2];
                    labels[row] = flag[k] ? 1.0f : 0.0f;
                }
            }
            run += flag[k];
        }
        carry += total;
    }
    for (int64_t row = kin + kout + threadIdx.x; row < N; row += kSgScanThreads) {   // the outside samples ran short
        samples[3 * row] = 0.0f; samples[3 * row + 1] = 0.0f; samples[3 * row + 2] = 0.0f;
        labels[row] = 0.0f;
    }
    if (threadIdx.x == 0) { counts[0] = (int32_t)kin; counts[1] = (int32_t)kout; }
}

struct SgLayout { size_t all, inside, total; };

SgLayout sg_layout(int64_t n)
{
    SgLayout L{};
    ScratchTake take;
    L.all = take((size_t)n * 12); L.inside = take((size_t)n);
    L.total = take.o;
    return L;
}

}  // namespace
}  // namespace icon

using namespace icon;

extern "C" int icon_sample_geo_bytes(int64_t n, int64_t *bytes)
{
    ICON_ARG(bytes != nullptr, "icon_sample_geo_bytes: null argument");
    ICON_ARG(n > 0 && n < (1ll << 31), "icon_sample_geo_bytes: 0 < n < 2^31");
    *bytes = (int64_t)sg_layout(n).total;
    return ICON_OK;
}

extern "C" int icon_sample_geo(const icon_mesh_t *scan, const float *d_verts, const float *d_vert_normals,
                               const double *calib, const double *calib_inv, int64_t N, double sigma_geo, int zray, int R,
                               uint64_t seed, float *d_samples, float *d_labels, int32_t *d_counts,
                               float *d_all_samples, uint8_t *d_all_inside, int32_t *d_all_source, int32_t *d_all_vertex,
                               void *d_scratch, int64_t scratch_bytes, void *stream)
{
    ICON_ARG(scan && d_verts && calib && calib_inv && d_samples && d_labels && d_counts && d_scratch, "icon_sample_geo: null argument");
    ICON_ARG(N >= 1 && N < (1ll << 24), "icon_sample_geo: 1 <= num_sample_geo < 2^24");
    ICON_ARG(R >= 1 && R <= 64, "icon_sample_geo: 1 <= ray_sample_num <= 64");
    ICON_ARG(sigma_geo == sigma_geo && sigma_geo - sigma_geo == 0.0, "icon_sample_geo: sigma_geo is not finite");
    ICON_ARG(scan->V > 0 && scan->V < (1ll << 31), "icon_sample_geo: the scan has no vertices");
    for (int k = 0; k < 12; ++k)
        ICON_ARG(calib[k] - calib[k] == 0.0 && calib_inv[k] - calib_inv[k] == 0.0, "icon_sample_geo: calib / calib_inv is not finite");
    SgParams p{};
    p.verts = d_verts; p.normals = d_vert_normals ? d_vert_normals : scan->d_vnormals;
    p.V = scan->V; p.N = N; p.nS = 4 * N; p.nU = N / 4; p.R = R;
    p.n = p.nS + p.nU + (zray ? p.nS * R : 0);
    ICON_ARG(p.n < (1ll << 31), "icon_sample_geo: 4 N + N / 4 + 4 N R must stay below 2^31");
    p.half_bits = 1;
    while ((1ll << (2 * p.half_bits)) < p.n) ++p.half_bits;
    p.sigma = sigma_geo; p.seed = seed;
    for (int k = 0; k < 12; ++k) { p.calib[k] = calib[k]; p.calib_inv[k] = calib_inv[k]; }
    const SgLayout L = sg_layout(p.n);
    if (const int e = scratch_check("icon_sample_geo", "icon_sample_geo_bytes", d_scratch, scratch_bytes, L.total)) return e;
    char *s = static_cast<char *>(d_scratch);
    float *all = d_all_samples ? d_all_samples : reinterpret_cast<float *>(s + L.all);
    uint8_t *inside = d_all_inside ? d_all_inside : reinterpret_cast<uint8_t *>(s + L.inside);
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)((p.n + kSgBlock - 1) / kSgBlock);
    hipLaunchKernelGGL(k_sg_draw, dim3(grid), dim3(kSgBlock), 0, st, p, all, d_all_source, d_all_vertex);
    hipLaunchKernelGGL(k_sg_inside, dim3(grid), dim3(kSgBlock), 0, st, scan->dev, (const float *)all, p.n, inside);
    hipLaunchKernelGGL(k_sg_balance, dim3(1), dim3(kSgScanThreads), 0, st, (const float *)all, (const uint8_t *)inside, p.n, N,
                       d_samples, d_labels, d_counts);
    ICON_HIP(hipGetLastError());
    return ICON_OK;
}

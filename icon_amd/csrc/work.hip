// work.hip - the workspace of the query calls (icon_work_*): its scratch (ensure_work), its profiling and set_* entries, the
// shared walks' error record, and the table of the process-wide test / A-B switches (option(), icon_debug_set_*).
#include "geom_device.h"

#include <algorithm>

namespace icon {
// ---- the process-wide switches (test / A-B; production leaves all of them alone) ------------------------------------------------
// id: the row's place, checked below against enum Opt (common.h); key: the name icon_debug_set_option knows it by (null: an ABI
// function of its own sets it); env: the variable read ONCE, at the first use, unless a set came first; ok: the values a set
// accepts (null: a flag - anything non-zero is 1, from the variable too)
struct Option { Opt id; const char *key, *env; int def; bool (*ok)(int); const char *accepts; };
static constexpr Option kOptions[kOptCount] = {
    {kOptPairBox, "pair_box", "ICON_AMD_PAIR_BOX", 1},              // the packet walk culls leaf pairs by their oriented boxes    } meshes and mesh
    {kOptNodeBox, "node_box", "ICON_AMD_NODE_BOX", 1},              // ... tests the children of the bottom inner nodes by them    } batches created
    {kOptBoxClamp, "box_clamp", "ICON_AMD_BOX_CLAMP", 1},           // the lattice launches evaluate them in half units, clamped   } AFTERWARDS
    {kOptLatticeFast, "lattice_fast", "ICON_AMD_LATTICE_FAST", 1},  // 0: every packet derives its own set-up (A/B runs)
    {kOptUnfused, nullptr, "ICON_AMD_UNFUSED", 0},                  // icon_debug_set_unfused: 1 forces the materialising path
    {kOptShellSkip, nullptr, "ICON_AMD_SHELL_SKIP", 1},             // icon_debug_set_shell_skip: 0 evaluates and masks the in_cube shell
    {kOptMcClassify1, "mc_classify1", "ICON_AMD_MC_CLASSIFY1", 0},  // 1: marching cubes classifies one cell per thread at every size (A/B)
    {kOptShareWaves, "share_waves", "ICON_AMD_SHARE", -1,          // wavefronts per shared walk (4: the adaptive schedule's searches only)
     [](int v) { return v == -1 || v == 1 || v == 4 || v == 8 || v == 16; }, "-1 (by launch size), 1, 4, 8 or 16"},
    {kOptShareRing, "share_ring", nullptr, 0,                       // forced ring size of the shared walks (0 = 64)
     [](int v) { return v == 0 || (v >= 2 && v <= 64 && (v & (v - 1)) == 0); }, "0 or a power of two in 2..64"},
    {kOptShareLose, "share_lose_push", nullptr, 0,                  // the ticket of the push that is announced but never stored (0 = none)
     [](int v) { return v >= 0; }, "a ticket >= 1, or 0"},
    {kOptShareSpinLog2, "share_spin_log2", nullptr, 0,              // wait bound 2^n polls (0 = 2^18)
     [](int v) { return v >= 0 && v < 30; }, "0..29"},
};
constexpr bool options_in_enum_order(int o = 0) { return o == kOptCount || (kOptions[o].id == o && options_in_enum_order(o + 1)); }
static_assert(options_in_enum_order(), "kOptions[] must list the switches in the order of enum Opt");
static int g_opt_value[kOptCount];
static bool g_opt_known[kOptCount];          // the value was set, or read from the environment
int option(Opt o)
{
    if (!g_opt_known[o]) {
        const Option &e = kOptions[o];
        const char *v = e.env ? getenv(e.env) : nullptr;
        g_opt_value[o] = !v ? e.def : (e.ok ? atoi(v) : atoi(v) != 0);
        g_opt_known[o] = true;
    }
    return g_opt_value[o];
}
static void set_option(Opt o, int value) { g_opt_value[o] = kOptions[o].ok ? value : (value != 0); g_opt_known[o] = true; }

int work_share_dbg(icon_work *w, ShareDbg *out)
{
    if (!w->h_err) {
        ICON_HIP(hipHostMalloc((void **)&w->h_err, 8 * sizeof(int), hipHostMallocMapped | hipHostMallocPortable));   // (portable: a process may drive several devices)
        memset(w->h_err, 0, 8 * sizeof(int));
    }
    void *dev = nullptr;
    ICON_HIP(hipHostGetDevicePointer(&dev, w->h_err, 0));
    out->err = (int *)dev;
    out->ring = option(kOptShareRing); out->lose = option(kOptShareLose); out->spin_log2 = option(kOptShareSpinLog2);
    return ICON_OK;
}

int work_check_err(icon_work *w)
{
    if (!w || !w->h_err) return ICON_OK;
    volatile int *e = w->h_err;
    const int code = e[0];
    if (code == 0 || code == kShareErrClaimed) return ICON_OK;     // (claimed: a wave is still writing the details - the next look reports it)
    char buf[320];
    static const char *what[] = {"", "a wave waited in vain for the node of its queue ticket (lost or abandoned push)",
                                 "a wave waited in vain for its ring slot to be cleared (ring a full turn behind)",
                                 "an idle wave outlasted its bound while the workgroup was still active"};
    snprintf(buf, sizeof(buf), "shared-walk search: %s [code %d, workgroup %d, wave %d, ticket %d, head %d, tail %d, avail %d, active %d]; the results of "
             "that launch are not to be trusted", what[code >= 1 && code <= 3 ? code : 0], code, e[1], e[7], e[2], e[3], e[4], e[5], e[6]);
    for (int k = 0; k < 8; ++k) e[k] = 0;
    return fail(ICON_ERR_STATE, buf);
}


void mark(icon_work *w, int k, hipStream_t st)
{
    if (w->prof) { (void)hipEventRecord(w->ev[k], st); if (k == 3) w->ev_valid = true; }
}

// scratch for n_points: (slot, d^2) + 1-byte codes + scan arrays + sign list; the 64-byte input rows only
// for the paths that still materialise them (need_x: precision f32 and the brute-force search)
int ensure_work(icon_work *w, int64_t n_points, bool need_x)
{
    { const int rc = work_check_err(w); if (rc) return rc; }      // an earlier launch on this workspace reported: no new work on its results
    if (n_points > w->cap_points) {
        (void)hipFree(w->d_near16); (void)hipFree(w->d_near_d2); w->d_near16 = nullptr; w->d_near_d2 = nullptr; w->cap_points = 0;
        ICON_HIP(hipMalloc((void **)&w->d_near16, (size_t)n_points * sizeof(uint16_t)));
        ICON_HIP(hipMalloc((void **)&w->d_near_d2, (size_t)n_points * sizeof(float)));
        (void)hipFree(w->d_code8); w->d_code8 = nullptr;
        ICON_HIP(hipMalloc((void **)&w->d_code8, (size_t)n_points));
        w->cap_points = n_points;
    }
    if (need_x && n_points > w->cap_x) {
        (void)hipFree(w->d_x); w->d_x = nullptr; w->cap_x = 0;
        ICON_HIP(hipMalloc((void **)&w->d_x, (size_t)n_points * kXRow * sizeof(float)));
        w->cap_x = n_points;
    }
    const int64_t nblk = (n_points + kScanBlock - 1) / kScanBlock;
    if (nblk > w->cap_blocks) {
        (void)hipFree(w->d_block_counts); (void)hipFree(w->d_block_offsets); (void)hipFree(w->d_scan_local); (void)hipFree(w->d_scan_part);
        w->d_block_counts = nullptr; w->d_block_offsets = nullptr; w->d_scan_local = nullptr; w->d_scan_part = nullptr; w->cap_blocks = 0;
        (void)hipFree(w->d_grp_mask); w->d_grp_mask = nullptr;
        ICON_HIP(hipMalloc((void **)&w->d_grp_mask, (size_t)nblk * 4 * sizeof(uint64_t)));
        ICON_HIP(hipMalloc((void **)&w->d_block_counts, (size_t)nblk * sizeof(int32_t)));
        ICON_HIP(hipMalloc((void **)&w->d_block_offsets, (size_t)nblk * sizeof(int64_t)));
        ICON_HIP(hipMalloc((void **)&w->d_scan_local, (size_t)nblk * sizeof(int32_t)));
        ICON_HIP(hipMalloc((void **)&w->d_scan_part, (size_t)((nblk + 1023) / 1024) * sizeof(int64_t)));
        w->cap_blocks = nblk;
    }
    if (n_points > w->cap_signs) {
        (void)hipFree(w->d_signs); w->d_signs = nullptr; w->cap_signs = 0;
        ICON_HIP(hipMalloc((void **)&w->d_signs, (size_t)n_points));
        w->cap_signs = n_points;
    }
    if (!w->d_total) ICON_HIP(hipMalloc((void **)&w->d_total, sizeof(int64_t)));
    if (!w->d_flag) ICON_HIP(hipMalloc((void **)&w->d_flag, sizeof(int)));
    if (!w->d_steal) {
        ICON_HIP(hipMalloc((void **)&w->d_steal, 9 * sizeof(unsigned int)));
        ICON_HIP(hipMemset(w->d_steal, 0, 9 * sizeof(unsigned int)));     // (synchronous with respect to the host: ordered before any launch)
    }
    if (!w->d_seg) ICON_HIP(hipMalloc((void **)&w->d_seg, (kMaxWorld + 1) * sizeof(int64_t)));
    return ICON_OK;
}

int begin_call(icon_work *w, const QueryCall &c, bool need_x)
{
    const int rc = ensure_work(w, c.N, need_x);
    if (rc) return rc;
    if (c.prior == ICON_PRIOR_ICON && c.mesh->F > kNearLoSlots && w->cap_points_hi < w->cap_points) {      // big meshes: the byte of higher slot bits
        (void)hipFree(w->d_near_hi); w->d_near_hi = nullptr; w->cap_points_hi = 0;
        ICON_HIP(hipMalloc((void **)&w->d_near_hi, (size_t)w->cap_points));
        w->cap_points_hi = w->cap_points;
    }
    w->slab_ready = false;
    return ICON_OK;
}

// the stride-(sx, sy, sz) sub-lattice of a [res]^3 volume: one thread per point, one store per wavefront that finds a value above
// the level into a HOST-MAPPED word (visible to the host once the stream has drained: no copy, no second launch)
__global__ __launch_bounds__(256) void k_any_above(const float *__restrict__ occ, int res, int sx, int sy, int sz, int nx, int ny, int nz, float level, int *flag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool pos = false;
    if (i < (int64_t)nx * ny * nz) {
        const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / ((int64_t)nx * ny));
        pos = occ[((int64_t)z * sz * res + (int64_t)y * sy) * res + (int64_t)x * sx] > level;
    }
    if (__any(pos) && (threadIdx.x & 63) == 0) *flag = 1;
}

}  // namespace icon

using namespace icon;

extern "C" int icon_work_create(icon_work_t **out)
{
    ICON_ARG(out != nullptr, "icon_work_create: out is null");
    *out = new icon_work();
    return ICON_OK;
}

extern "C" int icon_work_destroy(icon_work_t *w)
{
    if (!w) return ICON_OK;
    (void)hipFree(w->d_x); (void)hipFree(w->d_grp_mask); (void)hipFree(w->d_block_counts); (void)hipFree(w->d_block_offsets); (void)hipFree(w->d_scan_local); (void)hipFree(w->d_scan_part);
    (void)hipFree(w->d_signs); (void)hipFree(w->d_total); (void)hipFree(w->d_flag); (void)hipFree(w->d_seg); (void)hipFree(w->d_row_count); (void)hipFree(w->d_row_slots); (void)hipFree(w->d_lfast); if (w->h_err) (void)hipHostFree(w->h_err); if (w->h_any) (void)hipHostFree(w->h_any); (void)hipFree(w->d_near16); (void)hipFree(w->d_near_hi); (void)hipFree(w->d_near_d2); (void)hipFree(w->d_code8);
    (void)hipFree(w->d_sort_keys); (void)hipFree(w->d_sort_idx); (void)hipFree(w->d_sort_tmp);
    for (int k = 0; k < 6; ++k) if (w->ev[k]) (void)hipEventDestroy(w->ev[k]);
    (void)hipFree(w->d_clock); (void)hipFree(w->d_steal);
    icon::mc_destroy(w->mc);
    icon::clean_destroy(w->clean);
    icon::adaptive_destroy(w->ad);
    delete w;
    return ICON_OK;
}

// out[0] = the nearest-triangle search kernel alone (ms; 0 when the call had none), out[1] = shader cycles and out[2] = wall
// time (ms) of the fused kernel's workgroup 0 (s_memtime / s_memrealtime stamps), out[3] = out[1] / out[2] as MHz - the
// EFFECTIVE clock under that launch's load.  Synchronises (on the call's last event).
extern "C" int icon_work_profile_detail(icon_work_t *w, double out[4])
{
    ICON_ARG(w != nullptr && out != nullptr, "icon_work_profile_detail: null argument");
    if (!w->prof || !w->ev_valid) return fail(ICON_ERR_STATE, "icon_work_profile_detail: no profiled call on this workspace");
    ICON_HIP(hipEventSynchronize(w->ev[3]));
    out[0] = out[1] = out[2] = out[3] = 0.0;
    if (w->ev_search) {
        float ms = 0.0f;
        ICON_HIP(hipEventElapsedTime(&ms, w->ev[4], w->ev[5]));
        out[0] = ms;
    }
    unsigned long long c[4] = {0, 0, 0, 0};
    ICON_HIP(hipMemcpy(c, w->d_clock, sizeof(c), hipMemcpyDeviceToHost));
    int dev = 0, khz = 0;
    ICON_HIP(hipGetDevice(&dev));
    ICON_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
    if (c[2] > c[0] && c[3] > c[1] && khz > 0) {
        out[1] = (double)(c[2] - c[0]);
        out[2] = (double)(c[3] - c[1]) / (double)khz;
        out[3] = out[1] / out[2] * 1e-3;
    }
    return ICON_OK;
}

// The workgroup records of the most recent profiled launch of the fused kernel.  rec[5 * b + ...] for workgroup b:
// [0] XCC id, [1] start (ms after the earliest workgroup's start), [2] span (ms, constant-rate counter), [3] shader cycles,
// [4] tiles evaluated.  *n = workgroups of that launch (at most cap are written).  Synchronises like icon_work_stage_ms.
extern "C" int icon_work_profile_workgroups(icon_work_t *w, double *rec, int cap, int *n)
{
    ICON_ARG(w != nullptr && rec != nullptr && n != nullptr && cap >= 0, "icon_work_profile_workgroups: bad argument");
    if (!w->prof || !w->ev_valid) return fail(ICON_ERR_STATE, "icon_work_profile_workgroups: no profiled call on this workspace");
    ICON_HIP(hipEventSynchronize(w->ev[3]));
    const int g = std::min(w->clock_grid, kMaxProfGrid);
    *n = g;
    if (g <= 0) return ICON_OK;
    std::vector<unsigned long long> c((size_t)kWgRec * g);
    ICON_HIP(hipMemcpy(c.data(), w->d_clock + 4, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    int dev = 0, khz = 0;
    ICON_HIP(hipGetDevice(&dev));
    ICON_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
    ICON_ARG(khz > 0, "icon_work_profile_workgroups: the device reports no wall clock rate");
    unsigned long long t0 = ~0ull;
    for (int b = 0; b < g; ++b) t0 = std::min(t0, c[(size_t)kWgRec * b + 1]);
    for (int b = 0; b < g && b < cap; ++b) {
        const unsigned long long *r = &c[(size_t)kWgRec * b];
        rec[5 * b + 0] = (double)(r[4] >> 32);
        rec[5 * b + 1] = (double)(r[1] - t0) / (double)khz;
        rec[5 * b + 2] = (double)(r[3] - r[1]) / (double)khz;
        rec[5 * b + 3] = (double)(r[2] - r[0]);
        rec[5 * b + 4] = (double)r[5];
    }
    return ICON_OK;
}

// permille of every workgroup's span of tiles that is drawn dynamically (0 = the static partition of rounds 1-5), in contiguous
// groups of `group` tiles (<= 127), own XCD's spans first.  Any setting gives the same volume bit for bit (a tile's result does not depend on who evaluates it).
extern "C" int icon_work_set_steal(icon_work_t *w, int permille, int group)
{
    ICON_ARG(w != nullptr && permille >= 0 && permille <= 1000 && group >= 1 && group <= 127, "icon_work_set_steal: bad argument");
    w->steal_permille = permille; w->steal_grp = group;
    return ICON_OK;
}

// Seg3dLossless._forward_faster's None test (lib/common/seg3d_lossless.py:173-177: nothing above 0.5 on the COARSEST lattice) on a
// dense device volume: *h_any = 1 when some point of the stride-(sx, sy, sz) sub-lattice exceeds `level`.  One kernel, then the
// call waits for the stream (as the reference's `.sum() == 0` does) - four torch operators, a device-to-host copy and ~35 us of
// GPU time before.
extern "C" int icon_volume_any_above(const float *d_occ, int res, int sx, int sy, int sz, float level, icon_work_t *w, void *stream, int *h_any)
{
    ICON_ARG(d_occ && w && h_any && res >= 1 && sx >= 1 && sy >= 1 && sz >= 1, "icon_volume_any_above: bad argument");
    if (!w->h_any) {
        ICON_HIP(hipHostMalloc((void **)&w->h_any, sizeof(int), hipHostMallocMapped | hipHostMallocPortable));
    }
    void *dev = nullptr;
    ICON_HIP(hipHostGetDevicePointer(&dev, w->h_any, 0));
    *(volatile int *)w->h_any = 0;
    const int nx = (res - 1) / sx + 1, ny = (res - 1) / sy + 1, nz = (res - 1) / sz + 1;
    const int64_t n = (int64_t)nx * ny * nz;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(icon::k_any_above, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_occ, res, sx, sy, sz, nx, ny, nz, level, (int *)dev);
    ICON_HIP(hipGetLastError());
    ICON_HIP(hipStreamSynchronize(st));
    *h_any = *(volatile int *)w->h_any;
    return ICON_OK;
}

extern "C" int icon_work_set_reserve_cus(icon_work_t *w, int n)
{
    ICON_ARG(w != nullptr && n >= 0, "icon_work_set_reserve_cus: bad argument");
    w->reserve_cus = n;
    return ICON_OK;
}

extern "C" int icon_work_profile(icon_work_t *w, int enable)
{
    ICON_ARG(w != nullptr, "icon_work_profile: work is null");
    if (enable && !w->ev[0])
        for (int k = 0; k < 6; ++k) ICON_HIP(hipEventCreate(&w->ev[k]));
    if (enable && !w->d_clock) {
        const size_t bytes = (size_t)(4 + kWgRec * kMaxProfGrid) * sizeof(unsigned long long);
        ICON_HIP(hipMalloc((void **)&w->d_clock, bytes));
        ICON_HIP(hipMemset(w->d_clock, 0, bytes));
    }
    w->clock_grid = 0;
    w->ev_search = false;
    w->prof = enable != 0;
    w->ev_valid = false;
    return ICON_OK;
}

extern "C" int icon_work_stage_ms(icon_work_t *w, float out_ms[3])
{
    ICON_ARG(w && out_ms, "icon_work_stage_ms: null argument");
    if (!w->prof || !w->ev_valid) return fail(ICON_ERR_STATE, "icon_work_stage_ms: no profiled call on this workspace");
    ICON_HIP(hipEventSynchronize(w->ev[3]));
    for (int k = 0; k < 3; ++k) ICON_HIP(hipEventElapsedTime(&out_ms[k], w->ev[k], w->ev[k + 1]));
    return ICON_OK;
}

// the shared walks' error record (see work_check_err): ICON_ERR_STATE once per reported error, then clear again.  Does not
// synchronise - a caller that wants the verdict on a particular launch synchronises its stream first.
extern "C" int icon_work_status(icon_work_t *work)
{
    ICON_ARG(work != nullptr, "icon_work_status: work is null");
    return work_check_err(work);
}

// the switches of the table above by name, and the two that live with their own code
extern "C" int icon_debug_set_option(const char *key, int value)
{
    ICON_ARG(key != nullptr, "icon_debug_set_option: key is null");
    const std::string k(key);
    for (int o = 0; o < kOptCount; ++o) {
        const Option &e = kOptions[o];
        if (!e.key || k != e.key) continue;
        ICON_ARG(!e.ok || e.ok(value), k + ": " + e.accepts);
        set_option((Opt)o, value);
        return ICON_OK;
    }
    if (k == "qc_lanes") { ICON_ARG(value == 0 || value == 64, "qc_lanes: 0 (default) or 64"); g_qc_lanes = value; }
    else if (k == "rn_lanes") { ICON_ARG(value == 0 || value == 1 || value == 8, "rn_lanes: 0 (default), 1 or 8"); g_rn_lanes = value; }
    else if (k == "tt_chunk") { ICON_ARG(value >= 0 && value <= 32, "tt_chunk: 0 (default) or 1..32"); g_tt_chunk = value; }
    else if (k == "ev_lanes") { ICON_ARG(value == 0 || value == 1 || value == 8, "ev_lanes: 0 (default), 1 or 8"); g_ev_lanes = value; }
    else return fail(ICON_ERR_ARG, "icon_debug_set_option: unknown key " + k);
    return ICON_OK;
}

extern "C" int icon_debug_set_unfused(int on)
{
    set_option(kOptUnfused, on);
    return ICON_OK;
}

extern "C" int icon_debug_set_shell_skip(int on)
{
    set_option(kOptShellSkip, on);
    return ICON_OK;
}

extern "C" int icon_work_set_tie_rule(icon_work_t *work, int rule, int ulps)
{
    ICON_ARG(work != nullptr, "icon_work_set_tie_rule: work is null");
    ICON_ARG(rule == 0 || rule == 1, "icon_work_set_tie_rule: rule must be 0 (definition) or 1 (highest index within ulps)");
    ICON_ARG(ulps >= 0 && ulps <= 255, "icon_work_set_tie_rule: ulps must be 0..255");
    work->tie_rule = rule; work->tie_ulps = ulps;
    return ICON_OK;
}

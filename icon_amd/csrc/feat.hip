// feat.hip - the feature handles (icon_feat_*): the image feature planes, and the pamir prior's volume, of one subject or
// of the B subjects of a batched call, repacked channel-last for the gathers of geom_device.h.
#include "common.h"

#include <algorithm>

namespace icon {

// repack B feature stacks [B][C][H][W] -> B plane sets [n_select][H][W][cpad] (channel-last, zero padded), `stride` floats
// apart; grid z = subject
__global__ void k_pack_planes(const float *__restrict__ src, int C, int H, int W, int n_select, int csel, int cpad, int64_t stride,
                              float *__restrict__ dst)
{
    const int64_t n = (int64_t)n_select * H * W * cpad;
    const float *s = src + (int64_t)blockIdx.z * C * H * W;
    float *d = dst + (int64_t)blockIdx.z * stride;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % cpad);
        const int64_t pix = (i / cpad) % ((int64_t)H * W);
        const int sel = (int)(i / ((int64_t)cpad * H * W));
        d[i] = (c < csel) ? s[((int64_t)(sel * csel + c)) * H * W + pix] : 0.0f;
    }
}

}  // namespace icon

using namespace icon;

// ---- feature handles: B plane sets (and, pamir prior, B volumes) at a fixed stride; icon_feat_create is B = 1 ----------------
namespace {

// allocates *dst and packs B stacks into it in one launch (B = 1: the grid of 1024 workgroups a single stack always had)
int pack_planes(const float *d_src, int B, int C, int H, int W, int n_select, int cpad, hipStream_t st, const char *what, float **dst, int64_t *stride)
{
    *stride = (int64_t)n_select * H * W * cpad;
    hipError_t e = hipMalloc((void **)dst, (size_t)*stride * B * sizeof(float));
    if (e != hipSuccess) return fail(ICON_ERR_HIP, std::string("hipMalloc ") + what + ": " + hipGetErrorString(e));
    hipLaunchKernelGGL(k_pack_planes, dim3((unsigned)std::max(1, 1024 / B), 1, (unsigned)B), dim3(256), 0, st, d_src, C, H, W, n_select,
                       C / n_select, cpad, *stride, *dst);
    e = hipGetLastError();
    if (e != hipSuccess) { (void)hipFree(*dst); *dst = nullptr; return fail(ICON_ERR_HIP, std::string("pack ") + what + ": " + hipGetErrorString(e)); }
    return ICON_OK;
}

// (the exported entry points have checked the arguments, each under its own name)
int feat_create(const float *d_planes, int B, int C, int H, int W, int n_select, hipStream_t st, icon_feat_t **out)
{
    icon_feat *f = new icon_feat();
    FeatDev &d = f->dev;
    d.C = C; d.H = H; d.W = W; d.n_select = n_select; d.csel = C / n_select; d.cpad = (d.csel + 3) & ~3;
    d.smpl_mask = kSmplCmap | kSmplNorm;
    d.vol = nullptr; d.Cv = 0; d.Dv = d.Hv = d.Wv = 0; d.vpad = 0;
    f->batch = B;
    const int rc = pack_planes(d_planes, B, C, H, W, n_select, d.cpad, st, "planes", &f->d_planes, &f->plane_stride);
    if (rc) { delete f; return rc; }
    d.planes = f->d_planes;
    *out = f;
    return ICON_OK;
}

// a volume is a "plane" of H' = D*H rows: same channel-last repack, zero padded to vpad
int feat_set_volume(icon_feat *f, const float *d_vol, int Cv, int Dv, int Hv, int Wv, hipStream_t st)
{
    const int vpad = (Cv + 3) & ~3;
    const int rc = pack_planes(d_vol, f->batch, Cv, Dv * Hv, Wv, 1, vpad, st, "volume", &f->d_vol, &f->vol_stride);
    if (rc) return rc;
    FeatDev &d = f->dev;
    d.vol = f->d_vol; d.Cv = Cv; d.Dv = Dv; d.Hv = Hv; d.Wv = Wv; d.vpad = vpad;
    return ICON_OK;
}

}  // namespace

extern "C" int icon_feat_create(const float *d_planes, int C, int H, int W, int n_select,
                                const float *d_vol, int Cv, int Dv, int Hv, int Wv,
                                void *stream, icon_feat_t **out)
{
    ICON_ARG(out != nullptr, "icon_feat_create: out is null");
    *out = nullptr;
    ICON_ARG(d_planes && C > 0 && H > 1 && W > 1, "icon_feat_create: bad planes");
    ICON_ARG(n_select == 1 || n_select == 2, "icon_feat_create: n_select must be 1 or 2");
    ICON_ARG(C % n_select == 0, "icon_feat_create: C not divisible by n_select");
    if (C / n_select > 16) return fail(ICON_ERR_UNSUPPORTED, "icon_feat_create: more than 16 channels per tap");
    if (d_vol) {
        ICON_ARG(Cv > 0 && Dv > 1 && Hv > 1 && Wv > 1, "icon_feat_create: bad volume");
        if (Cv > 8) return fail(ICON_ERR_UNSUPPORTED, "icon_feat_create: more than 8 volume channels");
    }
    icon_feat *f = nullptr;
    int rc = feat_create(d_planes, 1, C, H, W, n_select, (hipStream_t)stream, &f);
    if (!rc && d_vol && (rc = feat_set_volume(f, d_vol, Cv, Dv, Hv, Wv, (hipStream_t)stream))) icon_feat_destroy(f);
    if (!rc) *out = f;
    return rc;
}

extern "C" int icon_feat_create_batch(const float *d_planes, int B, int C, int H, int W, int n_select, void *stream, icon_feat_t **out)
{
    ICON_ARG(out != nullptr, "icon_feat_create_batch: out is null");
    *out = nullptr;
    ICON_ARG(d_planes && B >= 1 && C > 0 && H > 1 && W > 1, "icon_feat_create_batch: bad planes");
    ICON_ARG(n_select == 1 || n_select == 2, "icon_feat_create_batch: n_select must be 1 or 2");
    ICON_ARG(C % n_select == 0, "icon_feat_create_batch: C not divisible by n_select");
    ICON_ARG(B <= 65535, "icon_feat_create_batch: more than 65,535 subjects");
    if (C / n_select > 16) return fail(ICON_ERR_UNSUPPORTED, "icon_feat_create_batch: more than 16 channels per tap");
    return feat_create(d_planes, B, C, H, W, n_select, (hipStream_t)stream, out);
}

extern "C" int icon_feat_batch_set_volume(icon_feat_t *feat, const float *d_vol, int B, int Cv, int Dv, int Hv, int Wv, void *stream)
{
    ICON_ARG(feat != nullptr && d_vol != nullptr, "icon_feat_batch_set_volume: null argument");
    ICON_ARG(B == feat->batch, "icon_feat_batch_set_volume: the volume holds another number of subjects than the feature handle");
    ICON_ARG(feat->dev.vol == nullptr, "icon_feat_batch_set_volume: the handle already holds a volume");
    ICON_ARG(Cv > 0 && Dv > 1 && Hv > 1 && Wv > 1, "icon_feat_batch_set_volume: bad volume");
    if (Cv > 8) return fail(ICON_ERR_UNSUPPORTED, "icon_feat_batch_set_volume: more than 8 volume channels");
    return feat_set_volume(feat, d_vol, Cv, Dv, Hv, Wv, (hipStream_t)stream);
}

extern "C" int icon_feat_set_smpl_feats(icon_feat_t *f, int has_cmap, int has_norm)
{
    ICON_ARG(f != nullptr, "icon_feat_set_smpl_feats: feat is null");
    f->dev.smpl_mask = (has_cmap ? kSmplCmap : 0) | (has_norm ? kSmplNorm : 0);
    return ICON_OK;
}

extern "C" int icon_feat_destroy(icon_feat_t *f)
{
    if (!f) return ICON_OK;
    (void)hipFree(f->d_planes); (void)hipFree(f->d_vol);
    delete f;
    return ICON_OK;
}

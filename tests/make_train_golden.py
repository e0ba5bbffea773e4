#!/usr/bin/env python3
"""Reference fixture of the training step (tests/golden/train_step_ref.npz): the reference's own HGPIFuNet.query and get_error
(lib/net/HGPIFuNet.py:268-387), verbatim, with the regressor in TRAINING mode, on the CPU through oracle/ref_loader (the kaolin
leaves rebound to per-subject loops as tools/make_golden_batch.py rebinds them).

B = 2 subjects (tests/batch_subjects.py), N = 512 points, S = 2 feature stacks [2,12,32,32] that are leaves with requires_grad,
the synthetic checkpoint (norm 'batch', last_op Sigmoid as training builds it), labels = the inside test of the projected points
(oracle.check_sign).  Per variant - icon with all four smpl_feats ("full"), icon with ['sdf'] ("sdf", icon-mvp), pifu - the
file records the per-stack preds, the error, the feature gradients, filters.0.weight.grad, every bias gradient and the BatchNorm
running statistics after the step, once in float32 and once with the module, the features and the labels in float64 (the
geometry stays the float32 the reference computes; grid_sample then forms its weights from the float32 coordinates in float64).
A float64 record x64 is stored next to the float32 run's x32 as q = round((x64 - x32) / scale) in int8 with scale = max |x64 - x32| / 127
per array: x64 = x32 + q * scale to within scale / 2, i.e. to 0.4 % of the largest distance between the two runs (some 1e-8 of
the largest value) - what six float32 gradient arrays [2,12,32,32] leave room for in a committed fixture.

usage: python tests/make_train_golden.py [--check]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import batch_subjects as bs  # noqa: E402
import make_golden_batch as mgb  # noqa: E402
from icon_amd import synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "train_step_ref.npz")
B, N, S, C, SIZE, SDF_CLIP = 2, 512, 2, 12, 32, 0.05
VARIANTS = {"full": (("sdf", "norm", "vis", "cmap"), "icon"), "sdf": (("sdf",), "icon"), "pifu": ((), "pifu")}


def state_dict(variant: str) -> dict:
    feats, prior = VARIANTS[variant]
    if variant == "full":
        return synth.make_assets("body").state_dict
    return synth.make_mlp_state_dict(synth.SEED + 41 + len(variant), dims=(C + 1, 512, 256, 128, 1), sdf_channel=None if prior == "pifu" else C)


def planes(stack: int) -> np.ndarray:
    return bs.planes(B, C, SIZE, stack)


def build(ref, Sj, variant: str, dtype):
    feats, prior = VARIANTS[variant]
    netG, _ = ref_loader.build_netG(synth.make_assets("body"))
    sd = state_dict(variant)
    c0 = sd["filters.0.weight"].shape[1]
    netG.if_regressor = ref.MLP(filter_channels=[c0, 512, 256, 128, 1], name="if", res_layers=[2, 3, 4], norm="batch", last_op=torch.nn.Sigmoid())
    missing, unexpected = netG.if_regressor.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all("num_batches_tracked" in m for m in missing), (missing, unexpected)
    netG.if_regressor.to(dtype)
    netG.prior_type, netG.smpl_feats, netG.sdf_clip = prior, list(feats), SDF_CLIP
    netG.smpl_feat_dict = {k: torch.from_numpy(np.ascontiguousarray(Sj[k])) for k in ("smpl_verts", "smpl_faces", "smpl_cmap", "smpl_vis")}
    if dtype == torch.float64:          # grid_sample wants one dtype: the float32 coordinates of the reference's projection, widened
        netG.index = lambda feat, uv: ref.index(feat, uv.to(feat.dtype))
    netG.train()
    return netG


def run(ref, Sj, points, labels, variant: str, dtype):
    netG = build(ref, Sj, variant, dtype)
    feats = [torch.from_numpy(planes(s)).to(dtype).requires_grad_(True) for s in range(S)]
    preds = netG.query(features=feats, points=torch.from_numpy(points), calibs=torch.from_numpy(Sj["calibs"]), regressor=netG.if_regressor)
    assert len(preds) == S
    error = netG.get_error(preds, torch.from_numpy(labels).to(dtype))
    error.backward()
    reg = netG.if_regressor
    out = {"error": error.detach().numpy().reshape(1), "w0_grad": reg.filters[0].weight.grad.numpy()}
    for s in range(S):
        out[f"preds_{s}"] = preds[s].detach().numpy()
        out[f"feat_grad_{s}"] = feats[s].grad.numpy()
    for l, f in enumerate(reg.filters):
        out[f"bias_grad_{l}"] = f.bias.grad.numpy()
    for l, nrm in enumerate(reg.norms):
        out[f"running_mean_{l}"] = nrm.running_mean.detach().numpy()
        out[f"running_var_{l}"] = nrm.running_var.detach().numpy()
    return out


def generate():
    Sj = bs.subjects(B)
    with mgb.reference() as ref:
        points, redrawn = mgb.draw_points(Sj, N, seed=77)
        xyz = mgb.projected(points, Sj["calibs"])
        labels = np.stack([orc.check_sign(Sj["smpl_verts"][b], Sj["smpl_faces"][0], np.ascontiguousarray(xyz[b].T)) for b in range(B)])
        labels = labels.astype(np.float32)[:, None, :]
        fix = dict(points=points, labels=labels, calibs=Sj["calibs"], sdf_clip=np.float32(SDF_CLIP),
                   sha1_subjects=np.array(bs.sha1(Sj["smpl_verts"], Sj["smpl_vis"], Sj["smpl_cmap"], Sj["calibs"])),
                   sha1_planes=np.array(bs.sha1(*[planes(s) for s in range(S)])))
        for variant in VARIANTS:
            r32 = run(ref, Sj, points, labels, variant, torch.float32)
            r64 = run(ref, Sj, points, labels, variant, torch.float64)
            for k, v in r32.items():
                assert v.dtype == np.float32 and r64[k].dtype == np.float64, (k, v.dtype, r64[k].dtype)
                fix[f"{variant}/{k}"] = v
                d = r64[k] - v.astype(np.float64)
                scale = max(float(np.abs(d).max()), 1e-300) / 127.0
                fix[f"{variant}/{k}/q64"] = np.rint(d / scale).astype(np.int8)
                fix[f"{variant}/{k}/s64"] = np.float64(scale)
            print(f"{variant}: error {r32['error'][0]:.6f} (float64 {r64['error'][0]:.6f}), inside {labels.mean():.3f}, "
                  f"max |feat_grad - feat_grad64| {127 * max(float(fix[f'{variant}/feat_grad_{s}/s64']) for s in range(S)):.3e}")
    return fix


def load(path: str = OUT) -> dict:
    """the fixture with the float64 records reassembled: key 'variant/name' (float32 run) and 'variant/name64'"""
    g = np.load(path)
    out = {}
    for k in g.files:
        if k.endswith("/q64"):
            out[k[:-4] + "64"] = g[k[:-4]].astype(np.float64) + g[k].astype(np.float64) * float(g[k[:-4] + "/s64"])
        elif not k.endswith("/s64"):
            out[k] = g[k]
    return out


def main():
    fix = generate()
    if "--check" in sys.argv:
        g = np.load(OUT)
        for k, v in fix.items():
            assert np.array_equal(g[k], v), k
        print("fixture reproduced")
        return
    np.savez_compressed(OUT, **fix)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

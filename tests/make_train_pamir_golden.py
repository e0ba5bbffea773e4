#!/usr/bin/env python3
"""Reference fixture of the pamir training step (tests/golden/train_step_pamir_ref.npz): the reference's own HGPIFuNet with
prior_type='pamir' in TRAIN mode on the CPU - query + get_error + backward (lib/net/HGPIFuNet.py:268-387) - built by
tools/make_golden.py:pamir_reference_net(ve_gain=1) with the batch leaf of tools/make_golden_batch_pamir.py: its Voxelization
wrapper and its VolumeEncoder (train-mode BatchNorm3d, one [B,7,32,32,32] volume per stack) as they are.

B = 2 subjects of tests/batch_pamir.py with unequal pad counts, N = 512 points, S = 2 feature stacks [2,6,32,32] that are leaves
with requires_grad, the regressor (13,512,256,128,1) of tests/batch_pamir.py with norm 'batch' and last_op Sigmoid, labels = the
projected point lies in an ellipsoid about the origin (deterministic, 20 - 80 % inside).  Recorded, once in float32 and once with
the modules, the features and the labels in float64 (the geometry and the semantic volume stay the float32 the reference
computes): the per-stack preds, the error, the feature gradients, filters.0.weight.grad, every bias gradient and the regressor's
running statistics, the gradient of every parameter of ``ve`` that has one, its BatchNorm3d running statistics after the step, and
the gradient of each stack's ``vol_feat`` at a seeded sample of 4,096 voxels.  Those are captured by wrapping THIS instance's
``ve.forward``: it calls ``retain_grad()`` on the outputs (and hands the float32 semantic volume to the float64 modules as float64 -
Conv3d wants one dtype); nothing else.  The float64 records are stored as int8 steps from the float32 ones exactly as
tests/make_train_golden.py stores them.

usage: python tests/make_train_pamir_golden.py [--check]   (--check: a fresh float64 run against the committed file, see agrees)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import batch_pamir as bp  # noqa: E402
import batch_subjects as bs  # noqa: E402
from make_train_golden import load as _load_records  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "train_step_pamir_ref.npz")
B, N, S, C, CV, SIZE, VOL = 2, 512, 2, 6, 7, 32, 32
N_VOX = 4096                                    # voxels of each stack's vol_feat whose gradient is recorded
ELLIPSOID = (0.6, 0.9, 0.6)


def planes(stack: int) -> np.ndarray:
    return bs.planes(B, C, SIZE, stack)


def voxel_sample() -> np.ndarray:
    """flat indices into [B,CV,VOL,VOL,VOL], ascending"""
    return np.sort(np.random.RandomState(1234).choice(B * CV * VOL ** 3, N_VOX, replace=False)).astype(np.int64)


def labels_of(xyz: np.ndarray) -> np.ndarray:
    """xyz [B,3,N] projected -> [B,1,N] float32"""
    r = sum((xyz[:, k] / ELLIPSOID[k]) ** 2 for k in range(3))
    return (r < 1.0).astype(np.float32)[:, None, :]


def regressor_state_dict() -> dict:
    return bp.state_dict()


def set_regressor(netG, ref, dtype):
    sd = regressor_state_dict()
    netG.if_regressor = ref.MLP(filter_channels=[C + CV, 512, 256, 128, 1], name="if", res_layers=[2, 3, 4], norm="batch", last_op=torch.nn.Sigmoid())
    missing, unexpected = netG.if_regressor.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all("num_batches_tracked" in m for m in missing), (missing, unexpected)
    netG.if_regressor.to(dtype)


def run(Sj, points, labels, dtype, info=None):
    """one training step of a fresh reference network -> the records (numpy, ``dtype``); ``info``: a dict that receives the hash of
    the encoder's state before the step"""
    import make_golden_batch_pamir as mgbp
    with mgbp.reference_net() as (netG, ref):
        if info is not None:
            info["sha1_ve"] = ve_sha1(netG.ve)
        set_regressor(netG, ref, dtype)
        netG.ve.to(dtype)
        if dtype == torch.float64:          # grid_sample wants one dtype: the float32 coordinates of the reference's projection, widened
            netG.index = lambda feat, uv: ref.index(feat, uv.to(feat.dtype))
        held = []
        inner = netG.ve.forward

        def forward(x, intermediate_output=True):
            outs = inner(x.to(dtype), intermediate_output=intermediate_output)
            for o in outs:
                o.retain_grad()
            held.extend(outs)
            return outs
        netG.ve.forward = forward
        netG.train()
        netG.smpl_feat_dict = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in bp.padded(Sj).items()}
        feats = [torch.from_numpy(planes(s)).to(dtype).requires_grad_(True) for s in range(S)]
        preds = netG.query(features=feats, points=torch.from_numpy(points), calibs=torch.from_numpy(Sj["calibs"]), regressor=netG.if_regressor)
        assert len(preds) == S and len(held) == S
        error = netG.get_error(preds, torch.from_numpy(labels).to(dtype))
        error.backward()
        reg = netG.if_regressor
        out = {"error": error.detach().numpy().reshape(1), "w0_grad": reg.filters[0].weight.grad.numpy()}
        idx = voxel_sample()
        for s in range(S):
            out[f"preds_{s}"] = preds[s].detach().numpy()
            out[f"feat_grad_{s}"] = feats[s].grad.numpy()
            out[f"vol_grad_{s}"] = held[s].grad.numpy().reshape(-1)[idx]
        for l, f in enumerate(reg.filters):
            out[f"bias_grad_{l}"] = f.bias.grad.numpy()
        for l, nrm in enumerate(reg.norms):
            out[f"running_mean_{l}"] = nrm.running_mean.detach().numpy()
            out[f"running_var_{l}"] = nrm.running_var.detach().numpy()
        for k, p in netG.ve.named_parameters():
            if p.grad is not None:                   # conv3, bn, conv_out1 / conv_out2 are constructed and never applied (VE.py)
                out[f"ve_grad.{k}"] = p.grad.numpy()
        for k, m in netG.ve.named_modules():
            if isinstance(m, torch.nn.BatchNorm3d) and int(m.num_batches_tracked) > 0:
                out[f"ve_stat.{k}.running_mean"] = m.running_mean.detach().numpy()
                out[f"ve_stat.{k}.running_var"] = m.running_var.detach().numpy()
        return {k: np.ascontiguousarray(v) for k, v in out.items()}


def encoder(dtype=torch.float32):
    """the fixture's volume encoder without the reference's tree: tests/common.py's replica of VolumeEncoder's layer list carrying
    the weights pamir_reference_net gives it - the ``ve.*`` arrays of tests/golden/query_batch_pamir.npz, which the same function
    wrote (``sha1_ve`` of the fixture pins that) - in training mode"""
    from common import volume_encoder_replica
    g = np.load(os.path.join(ROOT, "tests", "golden", "query_batch_pamir.npz"))
    ve = volume_encoder_replica()
    ve.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("ve.")}, strict=False)
    return ve.to(dtype).train()


def ve_sha1(ve) -> str:
    return bs.sha1(*[v.detach().cpu().numpy().astype(np.float32) for k, v in sorted(ve.state_dict().items()) if "num_batches_tracked" not in k])


_VOLUME = {}


def oracle_volume() -> np.ndarray:
    """[B,3,128,128,128] f32: the semantic volume of the fixture's subjects from the oracle's voxeliser (the leaf the reference ran
    on here), every subject stripped and voxelised as the reference does it - computed once per process"""
    if "v" not in _VOLUME:
        from oracle import oracle as orc
        Sj = bp.subjects(B)
        vols = [orc.semantic_voxelize(Sj["verts"][b], len(Sj["code"]), Sj["code"], Sj["tets"], res=bp.VOL_RES, sigma=bp.SIGMA) for b in range(B)]
        _VOLUME["v"] = np.ascontiguousarray(np.stack(vols).transpose(0, 4, 1, 2, 3))
        _VOLUME["v"].setflags(write=False)
    return _VOLUME["v"]


def inputs():
    import make_golden_batch_pamir as mgbp
    Sj = bp.subjects(B)
    points, _ = mgbp.draw_points(Sj, N, seed=77)
    labels = labels_of(mgbp.projected(points, Sj["calibs"]))
    return Sj, points, labels


def generate():
    Sj, points, labels = inputs()
    assert 0.2 < labels.mean() < 0.8, labels.mean()
    pad = bp.padded(Sj)
    assert pad["pad_v_num"][0] != pad["pad_v_num"][1] and pad["pad_f_num"][0] != pad["pad_f_num"][1]
    fix = dict(points=points, labels=labels, calibs=Sj["calibs"], pad_v_num=pad["pad_v_num"], pad_f_num=pad["pad_f_num"],
               voxel_sample=voxel_sample(), sha1_subjects=np.array(bs.sha1(Sj["verts"], Sj["tets"], Sj["code"], Sj["calibs"])),
               sha1_planes=np.array(bs.sha1(*[planes(s) for s in range(S)])),
               sha1_regressor=np.array(bs.sha1(*[v for _, v in sorted(regressor_state_dict().items())])))
    info = {}
    r32 = run(Sj, points, labels, torch.float32, info)
    fix["sha1_ve"] = np.array(info["sha1_ve"])
    r64 = run(Sj, points, labels, torch.float64)
    assert sorted(r32) == sorted(r64)
    for k, v in r32.items():
        assert v.dtype == np.float32 and r64[k].dtype == np.float64, (k, v.dtype, r64[k].dtype)
        fix[f"step/{k}"] = v
        d = r64[k] - v.astype(np.float64)
        scale = max(float(np.abs(d).max()), 1e-300) / 127.0
        fix[f"step/{k}/q64"] = np.rint(d / scale).astype(np.int8)
        fix[f"step/{k}/s64"] = np.float64(scale)
    print(f"error {r32['error'][0]:.6f} (float64 {r64['error'][0]:.6f}), inside {labels.mean():.3f}, "
          f"max |vol_grad| {max(float(np.abs(r64[f'vol_grad_{s}']).max()) for s in range(S)):.3e}, "
          f"{sum(k.startswith('ve_grad.') for k in r32)} ve parameters with a gradient")
    return fix


def load(path: str = OUT) -> dict:
    """the fixture with the float64 records reassembled: key 'step/name' (float32 run) and 'step/name64'"""
    return _load_records(path)


def agrees(r64: dict, path: str = OUT) -> float:
    """a fresh FLOAT64 run against the fixture's float64 records -> the worst distance / allowed.  The float32 run is no yardstick
    for a regeneration: the CPU's float32 convolutions and BatchNorm reductions order their sums by the thread count of the process,
    and two float32 runs of this step differ by up to 2e-3 in a running variance.  The float64 run repeats to some 1e-12 of a
    quantity's size whatever the thread count, and the fixture holds it to half a quantisation step: allowed = step / 2 +
    1e-7 * max |x64| + 1e-12 (the last term for the bias gradients whose true value is 0)."""
    g, raw = load(path), np.load(path)
    assert sorted(f"step/{k}64" for k in r64) == sorted(k for k in g if k.startswith("step/") and k.endswith("64"))
    worst = 0.0
    for k, v in r64.items():
        ref = g[f"step/{k}64"]
        assert v.shape == ref.shape and v.dtype == np.float64, k
        allowed = 0.5 * float(raw[f"step/{k}/s64"]) + 1e-7 * float(np.abs(ref).max()) + 1e-12
        worst = max(worst, float(np.abs(v - ref).max()) / allowed)
    return worst


def main():
    if "--check" in sys.argv:           # inputs and hashes exactly, the float64 run within the fixture's quantisation (see agrees)
        Sj, points, labels = inputs()
        g = np.load(OUT)
        assert np.array_equal(g["points"], points) and np.array_equal(g["labels"], labels) and np.array_equal(g["calibs"], Sj["calibs"])
        info = {}
        worst = agrees(run(Sj, points, labels, torch.float64, info))
        assert str(g["sha1_ve"]) == info["sha1_ve"] and worst <= 1.0, worst
        print(f"fixture reproduced (float64 run: worst distance / allowed = {worst:.3f})")
        return
    fix = generate()
    np.savez_compressed(OUT, **fix)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

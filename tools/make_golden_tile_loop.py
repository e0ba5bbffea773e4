#!/usr/bin/env python3
"""The outputs tests/test_gpu_tile_loop.py pins, computed by the library of the tree this file lies in.

    python tools/make_golden_tile_loop.py [out.npz]      (on the GPU; default tests/golden/tile_loop_parent.npz)

Run at the commit BEFORE a change to the tile loop of the f16x3 MLP kernels (mlp_f16x3_device.h): such a change moves
instructions and addresses, never a bit of a result, and the file is what "never a bit" is checked against.  Arrays only.
Every launch runs twice into a NaN-filled buffer (the second launch starts from the counters and the buffer state the first
one left) and the two must agree.  cases() is also what the test calls, so the two cannot drift apart."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from icon_amd import _lib, synth  # noqa: E402
from icon_amd.engine import IconQueryEngine, MlpHandle  # noqa: E402

ROWS = (1, 31, 32, 33, 255, 256, 257, 600)       # a single wave, a block boundary (32), a tile boundary (256), two tiles
SLAB = (5, 22)                                   # of the res-33 lattice: 17 planes, starts and ends inside a tile
BIG = (97, 20, 52)                               # res, z0, z1: 288,800 work items - the kernel of calls beyond 262,144 points
SCHEDULE = (9, 17, 33)


def dev():
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def set_unfused(on):
    _lib.check(_lib.lib().icon_debug_set_unfused(C.c_int(int(on))), "icon_debug_set_unfused")


def digest(a):
    """sha256 of the array's bytes, as 32 uint8: pins a result too large to commit (with a strided sample beside it)"""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def mlp_state_dict(c0):
    return synth.make_assets("body").state_dict if c0 == 13 else synth.make_mlp_state_dict(synth.SEED + 5, dims=(c0, 512, 256, 128, 1))


def mlp_rows(c0, n):
    x = np.zeros((n, 16), np.float32)
    x[:, :c0] = np.random.RandomState(1000 * c0 + n).normal(0.0, 1.0, (n, c0)).astype(np.float32)
    return x


def icon_engine(cmap_mode="reference"):
    a = synth.make_assets("body")
    eng = IconQueryEngine(prior_type="icon", sdf_clip=a.sdf_clip, cmap_mode=cmap_mode)
    eng.set_mesh(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in a.state_dict.items()})
    return eng, T(a.features)


def vol_engine(prior):
    feat = synth.make_feature_planes(6 if prior == "pamir" else 12, 128, synth.SEED)
    sd = synth.make_mlp_state_dict(synth.SEED + (1 if prior == "pamir" else 2), sdf_channel=None)
    eng = IconQueryEngine(prior_type=prior)
    if prior == "pamir":
        eng.set_volume_features(T(synth.make_feature_volume(7, 32, synth.SEED)))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in sd.items()})
    return eng, T(feat)


def slab_twice(eng, feat, res, z0, z1):
    """eval_slab twice into NaN-filled buffers -> the volume (asserts the two launches agree bit for bit)"""
    outs = []
    for _ in range(2):
        out = torch.full((z1 - z0, res, res), float("nan"), dtype=torch.float32, device=dev())
        eng.eval_slab(feat, res, z0, z1, out=out)
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), (res, z0, z1)
    return outs[0]


def partitions(n_cu):
    """(steal permille, group, reserved CUs) for the 117 tiles of a res-33 volume: the full grid (one tile per workgroup), 39
    workgroups (3 tiles each: odd) and 58 (2 each, one with 3: even and odd) - each all static, with the default pool (empty
    for spans this short) and with half of every span pooled (one tile of a span of two or three)"""
    return [(p, g, r) for r in (0, n_cu - 39, n_cu - 58) for p, g in ((0, 1), (150, 2), (500, 1))]


def cases(only=None):
    """name -> array.  `only`: a prefix to restrict the work to (the test calls it group by group)."""
    out = {}
    want = lambda name: only is None or name.startswith(only)
    if want("mlp"):
        for c0 in (13, 7):
            h = MlpHandle({k: torch.from_numpy(v) for k, v in mlp_state_dict(c0).items()})
            for n in ROWS:
                out[f"mlp_c{c0}_n{n}"] = h.forward(T(mlp_rows(c0, n)), precision="f16x3").cpu().numpy()
    if want("icon"):
        for mode in ("reference", "local"):
            eng, feat = icon_engine(mode)
            for res in (9, 17, 33):
                out[f"icon_{mode}_{res}"] = slab_twice(eng, feat, res, 0, res)
            if mode == "reference":
                out["icon_reference_33_slab"] = slab_twice(eng, feat, 33, *SLAB)
                big = slab_twice(eng, feat, *BIG)
                out["icon_reference_big_sha256"] = digest(big)
                out["icon_reference_big_sample"] = big.ravel()[::97].copy()
    if want("pamir") or want("pifu"):
        for prior in ("pamir", "pifu"):
            if want(prior):
                eng, feat = vol_engine(prior)
                out[f"{prior}_17"] = slab_twice(eng, feat, 17, 0, 17)
                if prior == "pamir":
                    out["pamir_33"] = slab_twice(eng, feat, 33, 0, 33)
    if want("schedule"):
        eng, feat = icon_engine("reference")
        vol, counts, _ = eng.adaptive_eval(feat, list(SCHEDULE))
        out["schedule_33"] = vol.cpu().numpy()
        out["schedule_counts"] = np.asarray(counts, np.int64)
    return out


if __name__ == "__main__":
    _lib.require_device()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "tile_loop_parent.npz")
    arrays = cases()
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")

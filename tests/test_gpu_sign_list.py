"""The outlier sign list of reference cmap mode (csrc/sign_list_device.h, csrc/outlier_list.hip) on every path that reads it:
the fused kernel (default f16x3) and the patch kernel of the materialising paths (f16x3 under icon_debug_set_unfused(1),
precision f32), with the list in each of its three places - the call's own (eval_slab), a global list with a rank offset
(slab_finish), the gathered messages (slab_finish_gathered).

Mesh: the icosphere scaled by 1.3, so that the lattice has outliers of both signs in numbers (the stock body and icosphere
leave the list almost all -1, where a wrong rank or a wrong index would mostly go unseen).  The cuts make every non-empty
slab cross the mesh and leave one rank empty.  The guards on that are computed from the oracle and asserted before any
device comparison."""
from contextlib import contextmanager
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from common import assets, oracle_query, orc
from icon_amd import synth

pytestmark = pytest.mark.gpu

OCC_TOL = 1e-4                                   # the bar of every lattice comparison in test_gpu_parity.py
CUTS = {9: [0, 4, 4, 5, 9],                      # 729 points; every slab is at most two 256-point blocks
        33: [0, 14, 14, 18, 33]}                 # 35,937 points = 140 blocks + 97
PATHS = ["fused", "unfused", "f32"]


def dev():
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


@lru_cache(maxsize=None)
def mesh():
    a = SimpleNamespace(**vars(assets("ico")))
    a.smpl_verts = (a.smpl_verts * np.float32(1.3)).astype(np.float32)
    return a


def slabs(res):
    c = CUTS[res]
    return list(zip(c[:-1], c[1:]))


@lru_cache(maxsize=None)
def oracle(res):
    """the oracle's outlier sign list (lattice order) and occupancy of the res^3 lattice; asserts the guards"""
    a = mesh()
    o = orc.cal_sdf(a.smpl_verts[0], a.smpl_faces[0], a.smpl_cmap[0], a.smpl_vis[0], synth.lattice_points(res))
    sdf = o["sdf"].reshape(res, res * res)
    out = np.abs(sdf) >= np.float32(a.sdf_clip)
    for z0, z1 in slabs(res):
        if z1 > z0:      # every non-empty slab crosses the mesh: points in the band, outliers of both signs
            s, m = sdf[z0:z1], out[z0:z1]
            assert (~m).sum() >= 1 and (m & (s > 0)).sum() >= 1 and (m & (s < 0)).sum() >= 1, (res, z0, z1)
    signs = np.sign(sdf[out]).astype(np.int8)
    K = len(signs)
    j = np.arange(K)[:, None]
    triple = signs[(3 * j + np.arange(3)) % K]                 # HGPIFuNet.py:303-305
    differ = (triple != signs[:, None]).any(1).mean()
    assert differ >= 1 / 20, differ                            # the patched cmap is not what local mode would write
    occ, _ = oracle_query(a, synth.lattice_points(res))
    return SimpleNamespace(signs=signs, occ=occ.reshape(res, res, res))


def _set_unfused(on):
    import ctypes as C
    from icon_amd import _lib
    _lib.check(_lib.lib().icon_debug_set_unfused(C.c_int(int(on))), "icon_debug_set_unfused")


@contextmanager
def on_path(path):
    if path == "unfused":
        _set_unfused(1)
    try:
        yield
    finally:
        if path == "unfused":
            _set_unfused(0)


@lru_cache(maxsize=None)
def engines(precision):
    """[0]: the single call's engine; [1:]: one per rank (a workspace holds one prepared slab)"""
    from icon_amd.engine import IconQueryEngine
    a = mesh()
    out = []
    for _ in range(1 + len(CUTS[9]) - 1):
        e = IconQueryEngine(prior_type="icon", sdf_clip=a.sdf_clip, cmap_mode="reference", precision=precision)
        e.set_mesh(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
        e.set_regressor({k: torch.from_numpy(v) for k, v in a.state_dict.items()})
        out.append(e)
    return out


def engines_of(path):
    return engines("f32" if path == "f32" else "f16x3")


@lru_cache(maxsize=None)
def single_call(path, res):
    """the same path's eval_slab over the whole lattice (computed once, left unchanged)"""
    oracle(res)
    with on_path(path):
        return engines_of(path)[0].eval_slab(T(mesh().features), res, 0, res)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("res", sorted(CUTS))
def test_global_list(res, path):
    """slab_features per rank, the lists concatenated on the host, slab_finish with the total and the rank offsets"""
    exp = oracle(res)
    full = single_call(path, res)
    feat = T(mesh().features)
    ranks = [(r, z0, z1) for r, (z0, z1) in enumerate(slabs(res)) if z1 > z0]
    with on_path(path):
        eng = engines_of(path)
        lists, counts = [], []
        for r, z0, z1 in ranks:
            s, c = eng[1 + r].slab_features(feat, res, z0, z1)
            counts.append(int(c.item())); lists.append(s[: counts[-1]])
        signs = torch.cat(lists).contiguous()
        parts = [eng[1 + r].slab_finish(res, z0, z1, signs, sum(counts), sum(counts[:k]), device=dev()) for k, (r, z0, z1) in enumerate(ranks)]
    assert np.array_equal(signs.cpu().numpy(), exp.signs)
    assert torch.equal(torch.cat(parts), full)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("res", sorted(CUTS))
def test_gathered_messages(res, path):
    """slab_features(msg=), the buffer of a world of 4 with the empty rank's zero header in it, slab_finish_gathered - every slab
    of two or more planes finished in two pieces"""
    exp = oracle(res)
    full = single_call(path, res)
    feat = T(mesh().features)
    world = len(slabs(res))
    per = max(z1 - z0 for z0, z1 in slabs(res))
    stride = 8 + ((per * res * res + 3) // 4 + 7) // 8 * 8
    with on_path(path):
        eng = engines_of(path)
        msgs = []
        for r, (z0, z1) in enumerate(slabs(res)):
            msg = torch.full((stride,), 0x55, dtype=torch.int8, device=dev())     # what lies behind a message must not matter
            msg[:8] = 0
            if z1 > z0:
                eng[1 + r].slab_features(feat, res, z0, z1, msg=msg)
            msgs.append(msg)
        gathered = torch.cat(msgs).contiguous()
        parts = []
        for r, (z0, z1) in enumerate(slabs(res)):
            if z1 == z0:
                continue
            out = torch.full((z1 - z0, res, res), float("nan"), device=dev())
            zm = z0 + (z1 - z0 + 1) // 2
            for za, zb in ((z0, zm), (zm, z1)):
                if zb > za:
                    eng[1 + r].slab_finish_gathered(res, z0, z1, gathered, stride, world, r, out=out, za=za, zb=zb)
            parts.append(out)
    g = gathered.cpu().numpy().view(np.uint8).reshape(world, stride)
    counts = g[:, :8].copy().view(np.int64).ravel()
    assert counts[[z1 == z0 for z0, z1 in slabs(res)].index(True)] == 0 and counts.sum() == len(exp.signs)
    assert torch.equal(torch.cat(parts), full)


@pytest.mark.parametrize("res", sorted(CUTS))
def test_across_paths(res):
    """the materialising f16x3 path equals the fused one bit for bit; f16x3 and f32 are the oracle's volume within the bar"""
    exp = oracle(res)
    fused, unfused, f32 = (single_call(p, res) for p in PATHS)
    assert torch.equal(unfused, fused)
    for name, v in (("f16x3", fused), ("f32", f32)):
        err = np.abs(v.cpu().numpy() - exp.occ).max()
        print(f"res {res} {name}: max |occ - oracle| = {err:.3g}")
        assert err <= OCC_TOL, (name, err)

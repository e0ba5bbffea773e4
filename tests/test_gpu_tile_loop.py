"""The tile loop of the f16x3 MLP kernels (csrc/mlp_f16x3_device.h: layer 1 two chunks per iteration with swapped B-operand
registers, LDS addresses as immediates on per-lane bases, straight-line weight DMA; csrc/fused_f16x3.hip: the lattice index by
exact multiply-high reciprocals) holds nothing but products and activations - and computes, bit for bit, what the kernels
computed before the loop was taken apart: tests/golden/tile_loop_parent.npz holds the parent commit's outputs
(tools/make_golden_tile_loop.py, whose cases() this file runs).  Shapes: the smallest at which each changed path can go wrong -
rows around a wave / block / tile boundary, lattices whose row length is no power of two, a slab that starts and ends inside a
tile, workgroups that run an odd and an even number of tiles (both buffer parities at the hand-over to the next tile),
128-point tiles with waves that only issue DMA, and one call beyond 262,144 points (the kernel of the 257^3 step)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from common import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_golden_tile_loop", os.path.join(ROOT, "tools", "make_golden_tile_loop.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def parent():
    return dict(np.load(os.path.join(GOLDEN, "tile_loop_parent.npz")))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_group(parent, prefix):
    got = gen.cases(prefix)
    names = sorted(k for k in parent if k.startswith(prefix))
    assert names and sorted(got) == names, (sorted(got), names)
    bad = [k for k in names if not same_bits(got[k], parent[k])]
    assert not bad, bad
    return got


def test_mlp_forward_rows(parent):
    """MlpHandle.forward(precision="f16x3"): 1 .. 600 rows, c0 = 13 and c0 = 7"""
    got = check_group(parent, "mlp")
    assert len(got) == 2 * len(gen.ROWS) and all(np.isfinite(v).all() for v in got.values())


def test_icon_volumes(parent):
    """res 9, 17, 33 in both cmap modes, a slab inside the res-33 lattice, 32 planes of res 97 (every launch twice, NaN-prefilled)"""
    got = check_group(parent, "icon")
    assert all(np.isfinite(v).all() for v in got.values())
    v = got["icon_reference_33"]
    assert (v > 0.5).any() and (v < 0.5).any()
    # (the slab is a call of its own: in reference cmap mode its outliers read the slab's sign list, not the volume's)
    assert got["icon_reference_33_slab"].shape == (gen.SLAB[1] - gen.SLAB[0], 33, 33)


@pytest.mark.parametrize("prior", ["pamir", "pifu"])
def test_volume_priors(parent, prior):
    check_group(parent, prior)


def test_schedule_small_tiles(parent):
    """[9, 17, 33] through icon_adaptive_eval: 128-point tiles, waves without points"""
    got = check_group(parent, "schedule")
    assert int(got["schedule_counts"][0]) == 9 ** 3


@pytest.mark.parametrize("prior", ["icon", "pamir"])
def test_workgroup_tile_runs(parent, prior):
    """the res-33 volume (117 tiles of 256 work items) under static and pooled partitions on grids that give a workgroup one,
    two and three tiles: the chunk pairs meet the tile boundary with either buffer parity, the result does not move.  icon:
    the variant that may halve its tiles (it does on the full grid: 233 tiles of 128); pamir: the 257^3 variant and its pools."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_cu > 58
    eng, feat = gen.icon_engine("reference") if prior == "icon" else gen.vol_engine("pamir")
    want = parent["icon_reference_33" if prior == "icon" else "pamir_33"]
    work = eng._work()
    try:
        for permille, group, reserve in gen.partitions(n_cu):
            work.set_steal(permille, group)
            work.set_reserve_cus(reserve)
            assert same_bits(gen.slab_twice(eng, feat, 33, 0, 33), want), (permille, group, reserve)
    finally:
        work.set_steal(150, 2)
        work.set_reserve_cus(0)


def test_fused_equals_materialising(parent):
    """res 17: the fused kernel and the materialising path (k_mlp_f16x3 on rows in HBM) share the chunk bodies and agree bit for bit"""
    eng, feat = gen.icon_engine("reference")
    fused = gen.slab_twice(eng, feat, 17, 0, 17)
    gen.set_unfused(1)
    try:
        rows = gen.slab_twice(eng, feat, 17, 0, 17)
    finally:
        gen.set_unfused(0)
    assert same_bits(fused, rows) and same_bits(fused, parent["icon_reference_17"])

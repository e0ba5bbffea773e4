"""The checker's voxeliser (oracle orc_semantic_voxelize, the float32 restatement the HIP kernel is bit-compared with) against the
independent float64 reference (tests/vox_reference.py) on every case of tests/vox_cases.py: a mistake in the DEFINITION - face
order, orientation, box end points, the on-the-boundary rule - that kernel and checker share shows here, without a GPU.

Occupancy must be equal wherever the reference is decided (everywhere for `lattice`); values must agree to 1e-6: both sides are
float64 sums, the checker's over float32 squared distances."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vox_cases as vc  # noqa: E402
import vox_reference as vr  # noqa: E402
from common import orc  # noqa: E402

TOL = 1e-6


def run_orc(name, res, sigma=0.05):
    c = vc.get(name)
    return orc.semantic_voxelize(c["verts"], c["n_surface"], c["table"][:c["n_surface"]], c["tets"], res=res, sigma=sigma, return_occ=True)


def check(name, res, sigma=0.05):
    vc.check_cap(name, res, sigma)                          # the condition on the inputs first
    out, occ = run_orc(name, res, sigma)
    vc.compare(name, res, sigma, out, occ, TOL)
    return out, occ


def test_reference_candidate_boxes_equal_all_pairs():
    """the reference's own shortcut (candidates from the widened float64 box) against every voxel x every tetrahedron"""
    for name, res in (("lattice", vc.LATTICE_RES), ("mixed", 20), ("clamps_big", 20), ("skipped", 20)):
        c = vc.get(name)
        s, ok = vr.dense_signed(c["verts"], c["tets"], res)
        _, sure_in, und = vc.reference(name, res)
        on_or_in = ((s >= 0).all(-1) & ok[:, None]).any(0).reshape(res, res, res)
        strictly_out = ((s < 0).any(-1) | ~ok[:, None]).all(0).reshape(res, res, res)
        assert not (sure_in & ~on_or_in).any() and not (~sure_in & ~und & ~strictly_out).any()
        if c["exact"]:
            assert np.array_equal(sure_in, on_or_in) and not und.any()


@pytest.mark.parametrize("res", [32, 33])
def test_mirrored(res):
    """two index columns swapped: every volume negative - the other arm of the orientation switch, which no tetrahedron of the
    body takes; the same solid, so the same volume bit for bit"""
    assert (vc.orientation(vc.body()) > 0).all() and (vc.orientation(vc.mirrored()) < 0).all()
    out, occ = check("mirrored", res)
    out0, occ0 = check("body", res)
    assert np.array_equal(occ, occ0) and np.array_equal(out, out0)
    assert np.array_equal(vc.reference("mirrored", res)[1], vc.reference("body", res)[1])


@pytest.mark.parametrize("res", [20, 33, 2, 3, 5, 48])
def test_mixed_and_sizes(res):
    o = vc.orientation(vc.mixed())
    assert (o > 0).mean() >= 0.25 and (o < 0).mean() >= 0.25
    _, occ = check("mixed", res)
    if res in (20, 33):
        assert 0.05 <= occ.mean() <= 0.60


def test_lattice_no_voxel_exempt():
    hits = vc.boundary_hits(vc.lattice(), vc.LATTICE_RES)
    print(f"lattice: {hits} (tetrahedron, voxel) pairs with the centre on a face, edge or vertex")
    assert hits >= 50
    _, _, und = vc.check_cap("lattice", vc.LATTICE_RES)
    assert not und.any()
    check("lattice", vc.LATTICE_RES)


@pytest.mark.parametrize("name,res", [("clamps", 20), ("clamps", 33), ("clamps_big", 20)])
def test_clamps(name, res):
    _, occ = check(name, res)
    assert occ.all() if name == "clamps_big" else (occ.any() and not occ.all())
    if name == "clamps":                                    # every face of the cube has occupied voxels in its outermost layer
        assert all(np.moveaxis(occ, k, 0)[i].any() for k in range(3) for i in (0, -1))


@pytest.mark.parametrize("res", [20, 33])
def test_skipped_rows(res):
    out, occ = check("skipped", res)
    out0, occ0 = check("skipped_valid", res)
    assert np.array_equal(occ, occ0) and np.array_equal(out, out0)
    c = vc.get("skipped")
    none, occ_none = orc.semantic_voxelize(c["verts"], c["n_surface"], c["table"][:c["n_surface"]], np.zeros((0, 4), np.int64), res=res, return_occ=True)
    assert not occ_none.any() and (none == 0).all()


@pytest.mark.parametrize("n_surface", vc.TILE_SURFACES)
def test_surface_vertex_counts(n_surface):
    out, _ = check(f"tiles{n_surface}", 20)
    assert np.abs(out).max() <= 1.0                         # the huge rows past n_surface never contribute


SIGMAS = [0.002, 0.005, 0.05, 0.5]


def tiny_values(sigma):
    """the condition on the inputs that makes "value != 0" useless as the occupancy: occupied voxels of the body at res 32 whose
    value float32 cannot hold as a normal number.  At sigma 0.005 the smallest value of an occupied voxel is 1.9e-19 - small, but
    a normal float32 - so the condition is asserted at 0.002, where the values go down to 1e-137."""
    values, sure_in, _ = vc.check_cap("body", 32, sigma)
    top = np.abs(values).max(-1)
    tiny = sure_in & (top < np.finfo(np.float32).tiny)
    print(f"sigma {sigma}: {int(tiny.sum())} of {int(sure_in.sum())} occupied voxels below float32's smallest normal, smallest {top[sure_in].min():.3e}")
    return int(tiny.sum())


@pytest.mark.parametrize("sigma", SIGMAS)
def test_sigma(sigma):
    n_tiny = tiny_values(sigma)
    if sigma == 0.002:
        assert n_tiny > 0
    check("body", 32, sigma)


def test_batch_subjects():
    for b in range(3):
        check(f"subject{b}of3", 33)

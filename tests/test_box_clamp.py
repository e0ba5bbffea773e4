"""The half-unit, clamped evaluation of the oriented boxes (mesh_rules.h: pair_box_bound_half; "box_clamp") on the host, through
icon_debug_box_bound_half, against pair_box_bound itself (icon_debug_box_bound) on the records the walk reads - the node boxes and
the leaf pairs' boxes of the host builder's arenas:
  4 * bound' == bound bit for bit wherever every axis excess is <= 2 (halving commutes with every rounding),
  4 * bound' <= bound everywhere (beyond 2 the excess stops at 1 in half units: the vote culls less, never more),
  never NaN; a NaN point and a non-finite record give 0 ("not culled").
Which points have every excess <= 2 is decided in float64 from the record, with a margin of 1e-3 either side of 2 in which only
the inequality is asked (the float32 excess may fall on either side there)."""
import ctypes as C

import numpy as np
import pytest

from node_box_cases import K_MAX_TRIS, STRIPS, box_bound, mesh, model, range_box

MESHES = ["body", "ico", "tiny", "dup", "line"] + list(STRIPS)


def box_bound_half(recs, pts, shared):
    """node_box_cases.box_bound's layout: recs [R,16,2], pts [N,3] (shared) or [R,N,3] -> [R,2,N] f32: pair_box_bound_half"""
    from icon_amd import _lib
    recs = np.ascontiguousarray(recs, np.float32); pts = np.ascontiguousarray(pts, np.float32)
    R = len(recs)
    N = pts.shape[0] if shared else pts.shape[1]
    assert recs.shape == (R, 16, 2) and pts.shape == ((N, 3) if shared else (R, N, 3))
    bound = np.full((R, 2, N), np.nan, np.float32)
    _lib.check(_lib.lib().icon_debug_box_bound_half(_lib.ptr(recs), C.c_int64(R), _lib.ptr(pts), C.c_int64(N), C.c_int(1 if shared else 0),
                                                    _lib.ptr(bound)), "icon_debug_box_bound_half")
    return bound


_trees = {}


def records_of(name):
    """every record the walk of this mesh reads: the node boxes of the oriented parents, then the pair boxes of the leaves"""
    if name not in _trees:
        v, f, _, _ = mesh(name)
        tree = model.NodeTree(v, f)
        _trees[name] = np.concatenate([tree.nbox[tree.oriented(K_MAX_TRIS)], tree.pbox[tree.leaf_cnt > 0]]).astype(np.float32)
    return _trees[name]


def max_excess64(recs, pts):
    """float64: the largest axis excess |t_k| - h_k of both components; recs [R,16,2], pts [R,N,3] -> [R,2,N]"""
    r = recs.astype(np.float64); p = pts.astype(np.float64)
    d = p[:, None, :, :] - np.moveaxis(r[:, 0:3, :], 1, 2)[:, :, None, :]              # [R, 2, N, 3]
    ax = np.moveaxis(r[:, 3:12, :], 1, 2).reshape(len(r), 2, 3, 3)                     # [R, 2, axis, xyz]
    t = np.einsum("rcak,rcnk->rcna", ax, d)
    h = np.moveaxis(r[:, 12:15, :], 1, 2)[:, :, None, :]
    return (np.abs(t) - h).max(-1)


def point_sets(recs, seed):
    """per record: lattice 33^3 points (every one used across the records), random points, points on and near the box, the cube's
    corners, and points 5 and 50 units away (the upper clamp) -> [R, N, 3] f32, and the slice of the far points"""
    R = len(recs)
    rs = np.random.RandomState(seed)
    g = np.linspace(-1.0, 1.0, 33)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    nl = max(48, -(-len(lattice) // R))
    il = (np.arange(R)[:, None] * nl + np.arange(nl)[None]) % len(lattice)
    cube = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
    rnd = rs.uniform(-1, 1, (R, 32, 3)).astype(np.float32)
    c = np.nan_to_num(recs[:, 0:3, :].mean(-1).astype(np.float64))                     # between the two boxes' centres
    near = (c[:, None, :] + np.concatenate([np.zeros((R, 1, 3)), rs.uniform(-1, 1, (R, 15, 3)) * 1e-3, rs.uniform(-1, 1, (R, 16, 3)) * 0.05], 1))
    dirs = rs.normal(size=(R, 16, 3)); dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    far = c[:, None, :] + dirs * np.where(np.arange(16) % 2 == 0, 5.0, 50.0)[None, :, None]
    pts = np.concatenate([lattice[il], np.broadcast_to(cube[None], (R, 8, 3)), rnd, near.astype(np.float32), far.astype(np.float32)], 1)
    return np.ascontiguousarray(pts, np.float32), slice(pts.shape[1] - 16, pts.shape[1])


@pytest.mark.parametrize("name", MESHES)
def test_quarter_of_the_bound_bit_for_bit_or_less(name):
    recs = records_of(name)
    if len(recs) == 0:
        pytest.fail(f"{name}: no record")
    pts, far = point_sets(recs, 5)
    full, half = box_bound(recs, pts, False), box_bound_half(recs, pts, False)
    assert not np.isnan(half).any() and not np.isnan(full).any()
    assert (half >= 0).all() and (half <= 3.0).all()                                   # three excesses of at most 1 each
    four = np.float32(4.0) * half                                                      # (exact: a power of two, no overflow)
    assert (four <= full).all()
    ex = max_excess64(recs, pts)
    inside, beyond = ex <= 2.0 - 1e-3, ex >= 2.0 + 1e-3
    assert np.array_equal(four[inside].view(np.uint32), full[inside].view(np.uint32))
    assert (four[beyond] < full[beyond]).all()
    if name in ("body", "ico"):
        assert inside.mean() > 0.5 and beyond[:, :, far].all()                         # both regimes are exercised: 5 and 50 units away clamp
    # a point ON the box (the mean of the two centres need not be; each centre is)
    for comp in (0, 1):
        cpts = np.ascontiguousarray(recs[:, None, 0:3, comp])
        assert (box_bound_half(recs, cpts, False)[:, comp, 0] == 0).all()


def test_nan_points_and_non_finite_records_never_cull():
    recs = records_of("body")[::37]
    nanp = np.float32([[np.nan, 0, 0], [0, np.nan, 0], [0.3, -0.2, np.nan], [np.nan] * 3])
    assert (box_bound_half(recs, nanp, True) == 0).all() and (box_bound(recs, nanp, True) == 0).all()
    pts = np.float32([[0.9, 0.9, 0.9], [-1, 1, -1], [np.nan, 0, 0], [5, -5, 5], [50, 50, -50], [np.inf, 0, 0], [-np.inf, np.inf, 0]])
    a, b, c = np.array([0.1, -0.2, 0.3]), np.array([0.4, 0.1, -0.2]), np.array([-0.3, 0.5, 0.1])
    tri = np.stack([a, b, c]).astype(np.float32)
    for val in (np.nan, np.inf, -np.inf):
        for pos in ((0, 0, 0), (6, 2, 1), (15, 1, 2)):
            t = np.stack([tri + 0.01 * k for k in range(16)]).astype(np.float32)
            t[pos] = val
            rec, kind = range_box(t)                                                   # the rule's own "never culled" record
            assert kind == 2 and np.isinf(rec[12:15]).all()
            r = np.zeros((1, 16, 2), np.float32); r[0, :15, 0] = rec; r[0, :15, 1] = rec
            assert (box_bound_half(r, pts, True) == 0).all()
    # records no builder writes - infinite extents on a real frame, a non-finite centre or axis with infinite extents: still 0, never NaN
    base = recs[:8].copy()
    for fld, val in ((slice(12, 15), np.inf), (0, np.nan), (1, np.inf), (4, np.nan), (7, -np.inf)):
        r = base.copy()
        r[:, 12:15, :] = np.inf
        r[:, fld, :] = val
        out = box_bound_half(r, pts, True)
        assert not np.isnan(out).any() and (out == 0).all(), (fld, val)
    # a finite record at an infinite point: the clamp's upper end, not NaN
    out = box_bound_half(base, pts[5:], True)
    assert not np.isnan(out).any() and (out <= 3.0).all()

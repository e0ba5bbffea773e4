"""The cloth refinement step (icon_amd/cloth.py) - CPU side: ClothTopology against a brute-force construction,
closed-form checks and a gradcheck of the oracle (tests/cloth_oracle.py), the gaps the GPU bars are taken from, and the host
contract of the module and of the native entries."""
import ctypes as C

import numpy as np
import pytest
import torch

import cloth_oracle as co
from icon_amd import _lib


@pytest.mark.parametrize("name", list(co.CASES))
def test_topology_equals_the_brute_force_construction(name):
    from icon_amd.cloth import ClothTopology
    v, f, want = co.mesh(name)
    V = len(v)
    t = ClothTopology(torch.from_numpy(f), num_verts=V)
    assert t.has_faces and t.num_verts == V and t.device.type == "cpu"
    for a in (t.edges, t.nbr_off, t.nbr, t.pairs, t.inc_off, t.inc):
        assert a.dtype == torch.int64 and a.is_contiguous()
    assert np.array_equal(t.edges.numpy(), want["edges"]) and t.num_edges == len(want["edges"])
    key = t.edges[:, 0] * V + t.edges[:, 1]
    assert (t.edges[:, 0] <= t.edges[:, 1]).all() and (key[1:] > key[:-1]).all()
    off, nbr = t.nbr_off.numpy(), t.nbr.numpy()
    assert off.shape == (V + 1,) and off[0] == 0 and off[-1] == 2 * t.num_edges == len(nbr)
    for i in range(V):
        assert nbr[off[i]:off[i + 1]].tolist() == want["rows"][i], i
    assert np.array_equal(t.pairs.numpy(), want["pairs"]) and t.num_pairs == len(want["pairs"])
    P = t.num_pairs
    ioff, inc = t.inc_off.numpy(), t.inc.numpy()
    assert ioff.shape == (V + 1,) and ioff[0] == 0 and ioff[-1] == 4 * P == len(inc)
    assert sorted(inc.tolist()) == list(range(4 * P))                      # every slot of every pair, once
    flat = want["pairs"].reshape(-1)
    for i in range(V):
        row = inc[ioff[i]:ioff[i + 1]]
        assert (np.diff(row) > 0).all() and (flat[row] == i).all(), i
    # int32 copies hold the same numbers; a [1,F,3] batch axis is dropped
    t32 = t.to(index_dtype=torch.int32)
    assert all(getattr(t32, n).dtype == torch.int32 and torch.equal(getattr(t32, n).long(), getattr(t, n)) for n in ClothTopology._FIELDS)
    assert torch.equal(ClothTopology(torch.from_numpy(f)[None].int(), num_verts=V).pairs, t.pairs)


def test_topology_counts_of_the_cases():
    from icon_amd.cloth import ClothTopology
    P = {n: len(co.mesh(n)[2]["pairs"]) for n in co.CASES}
    E = {n: len(co.mesh(n)[2]["edges"]) for n in co.CASES}
    assert (E["ico"], P["ico"]) == (480, 480) and (E["body"], P["body"]) == (20664, 20664)     # closed manifolds: one pair per edge
    assert P["grid"] == P["flat"] == E["grid"] - 2 * (8 + 6) == 130                              # boundary edges give none
    v, f, topo = co.mesh("fan")
    assert [p[:2] for p in topo["pairs"].tolist()].count([41, 42]) == 3 and len(topo["rows"][0]) == 40 and topo["rows"][46] == []
    assert len(co.mesh("v257")[0]) == 257
    for n in co.CASES:                                                     # no degenerate face anywhere: every nc gradient is compared
        v, f, _ = co.mesh(n)
        assert np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).min() > 1e-5
    # from an edge list alone: kept as listed, duplicates and all; no face parts
    e = torch.tensor([[0, 1], [2, 1], [0, 1]])
    t = ClothTopology(num_verts=4, edges=e)
    assert not t.has_faces and t.pairs is None and t.num_pairs == 0 and torch.equal(t.edges, e)
    assert t.nbr_off.tolist() == [0, 2, 5, 6, 6] and t.nbr.tolist() == [1, 1, 0, 0, 2, 1]


def test_topology_refuses_bad_input():
    from icon_amd.cloth import ClothTopology, IconAmdError
    f = torch.tensor([[0, 1, 2], [1, 2, 3]])
    with pytest.raises(IconAmdError, match="outside"):
        ClothTopology(f, num_verts=3)
    with pytest.raises(IconAmdError, match="outside"):
        ClothTopology(torch.tensor([[0, 1, -1]]), num_verts=3)
    with pytest.raises(IconAmdError, match="outside"):
        ClothTopology(num_verts=2, edges=torch.tensor([[0, 2]]))
    with pytest.raises(IconAmdError, match="integer"):
        ClothTopology(f.float(), num_verts=4)
    with pytest.raises(IconAmdError, match=r"\[N,3\]"):
        ClothTopology(f[:, :2], num_verts=4)
    with pytest.raises(IconAmdError, match="either"):
        ClothTopology(num_verts=4)
    with pytest.raises(IconAmdError, match="either"):
        ClothTopology(f, num_verts=4, edges=f[:, :2])
    with pytest.raises(IconAmdError, match="num_verts"):
        ClothTopology(f)


def test_oracle_closed_forms():
    # A = I, b = 0: nothing moves, nothing is stiff, nothing shears
    v, f, topo = co.mesh("ico")
    x = torch.from_numpy(v).double()[None]
    A = torch.eye(3, dtype=torch.float64).repeat(1, len(v), 1, 1)
    y, stiff, rigid = co.local_affine(x, A, torch.zeros(1, len(v), 3, 1, dtype=torch.float64), torch.from_numpy(topo["edges"]))
    assert torch.equal(y, x) and float(stiff) == 0.0 and float(rigid) == 0.0
    # flat: interior residuals vanish; 24 boundary vertices with residual (1, 2) / 4 or (2, 1) / 4, corners (0,0) and (8,6) with
    # (2, 2) / 3, corners (8,0) and (0,6) with (-1, 1) / 2 - the cells are split along (i, j) - (i + 1, j + 1)
    v, f, topo = co.mesh("flat")
    e, n, l = co.priors(torch.from_numpy(v).double(), torch.from_numpy(topo["edges"]), torch.from_numpy(topo["pairs"]))
    want = (24 * np.sqrt(5.0) / 4 + 2 * 2 * np.sqrt(2.0) / 3 + 2 * np.sqrt(2.0) / 2) / 63
    assert abs(float(l) - want) < 1e-14 and float(n) == 0.0
    assert abs(float(e) - (110 * 1.0 + 48 * 2.0) / 158) < 1e-14               # 8*7 + 9*6 = 110 unit sides, 48 diagonals of squared length 2
    # a regular tetrahedron, wound outwards: the normals of two faces enclose arccos(-1/3) - nc = 1 - (-1/3) for all six pairs
    tv = torch.tensor([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=torch.float64)
    tf = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    tt = co.topology_np(tf, 4)
    assert len(tt["pairs"]) == 6
    assert abs(float(co.normal_consistency(tv, torch.from_numpy(tt["pairs"]))) - 4.0 / 3.0) < 1e-14
    assert abs(float(co.normal_consistency(tv, torch.from_numpy(tt["pairs"][:1]))) - 4.0 / 3.0) < 1e-14


def test_oracle_gradcheck_on_the_fan():
    v, f, topo = co.mesh("fan")
    edges, pairs = torch.from_numpy(topo["edges"]), torch.from_numpy(topo["pairs"])
    x, A, b, G = (torch.from_numpy(t).double() for t in co.inputs("fan"))

    def chain(A_, b_):
        y, s, r = co.local_affine(x, A_, b_, edges)
        e, n, l = co.priors(y[0], edges, pairs, 0.1)
        return (y * G).sum() + 10.0 * s + 10.0 * r + l + e + n

    assert torch.autograd.gradcheck(chain, (A.requires_grad_(True), b.requires_grad_(True)), eps=1e-6, atol=1e-7, rtol=1e-5)
    verts = torch.from_numpy(v).double().requires_grad_(True)
    for k in range(3):
        assert torch.autograd.gradcheck(lambda y_: co.priors(y_, edges, pairs, 0.1)[k], (verts,), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_flat_pins_the_zero_subgradient():
    """interior residuals are exactly 0 in float64 AND float32: the Laplacian's gradient is finite, and only the boundary
    vertices' residuals drive it (an interior vertex is moved by its boundary neighbours' terms alone)"""
    for dtype in (torch.float64, torch.float32):
        r = co.run("flat", dtype=dtype)
        assert all(np.isfinite(r[k]).all() for k in r)
        assert float(r["nc"]) == 0.0 and (r["grad_verts_nc"] == 0).all()
        g = r["grad_verts_laplacian"].reshape(7, 9, 3)
        assert (g[2:-2, 2:-2] == 0).all() and np.abs(g[0]).max() > 0


def test_gaps_are_the_recorded_ones():
    """the GAP constants of tests/test_gpu_cloth.py are what the float32 run of the oracle on the CPU differs from its float64
    run by - largest over every run of cloth_oracle.RUNS and seeds 0..4 - measured here again (on one thread: one summation
    order on every host).  A constant may lie at most 3 % above what is measured here, so that the device bars stay at
    4 x gap; a constant BELOW the measurement only tightens the bars, so there is no lower bound - both are printed."""
    import test_gpu_cloth as tg
    worst = co.measure_gaps()
    assert set(worst) == set(tg.GAP)
    for kind, (g, where) in sorted(worst.items()):
        print(f"{kind:16s} float32 oracle against float64: {g:.3e} at {where}; recorded {tg.GAP[kind]:.3e}")
    for kind, (g, where) in worst.items():
        assert tg.GAP[kind] <= 1.03 * g, (kind, g, where)
    # the derived floor: a float32 scalar cannot be held to less than a few ulps of its own final rounding
    assert tg.FLOOR == 2.0 ** -22
    for s in co.SCALARS:
        assert tg.BAR[s] == (4 * tg.GAP[s] if tg.GAP[s] >= tg.FLOOR else tg.FLOOR)
    for kind in set(tg.GAP) - set(co.SCALARS):
        assert tg.BAR[kind] == 4 * tg.GAP[kind]


def test_cloth_entries_exist_and_raise():
    """fails on the parent: there is no icon_amd.cloth"""
    from icon_amd.cloth import (ClothTopology, IconAmdError, LocalAffine, local_affine_device, mesh_shape_prior_losses_device,
                                update_mesh_shape_prior_losses)
    v, f, _ = co.mesh("ico")
    V = len(v)
    topo = ClothTopology(torch.from_numpy(f), num_verts=V)
    x, A, b, _ = (torch.from_numpy(t) for t in co.inputs("ico"))
    verts = torch.from_numpy(v)
    with pytest.raises(IconAmdError, match="constant"):
        local_affine_device(x.clone().requires_grad_(True), A, b, topo)
    with pytest.raises(IconAmdError, match="must agree"):
        local_affine_device(x, A.repeat(2, 1, 1, 1), b, topo)
    with pytest.raises(IconAmdError, match="must agree"):
        local_affine_device(x, A, b[:, :-1], topo)
    with pytest.raises(IconAmdError, match="x must be"):
        local_affine_device(x[0], A, b, topo)
    with pytest.raises(IconAmdError, match="ClothTopology"):
        local_affine_device(x, A, b, torch.from_numpy(f))
    with pytest.raises(IconAmdError, match="cot"):
        mesh_shape_prior_losses_device(verts, topo, method="cot")
    with pytest.raises(IconAmdError, match="cot"):
        mesh_shape_prior_losses_device(verts, topo, method="cotcurv")
    with pytest.raises(IconAmdError, match="one mesh"):
        mesh_shape_prior_losses_device(verts[None].repeat(2, 1, 1), topo)
    with pytest.raises(IconAmdError, match="terms"):
        mesh_shape_prior_losses_device(verts, topo, terms=("edge", "cot"))
    with pytest.raises(IconAmdError, match="terms"):
        mesh_shape_prior_losses_device(verts, topo, terms=())
    with pytest.raises(IconAmdError, match="from faces"):
        mesh_shape_prior_losses_device(verts, ClothTopology(num_verts=V, edges=topo.edges))
    with pytest.raises(IconAmdError, match="verts must be"):
        mesh_shape_prior_losses_device(verts[:-1], topo)
    model = LocalAffine(V, 2, topo.edges)
    assert {k: tuple(t.shape) for k, t in model.state_dict().items()} == {"A": (2, V, 3, 3), "b": (2, V, 3, 1)}
    assert torch.equal(model.A[1, 5], torch.eye(3)) and float(model.b.detach().abs().max()) == 0.0 and model.num_points == V
    with pytest.raises(IconAmdError, match="needs the edges"):
        LocalAffine(V)(x, return_stiff=True)
    losses = {k: {"weight": 1.0, "value": 0.0} for k in ("edge", "nc", "laplacian")}
    host = "no CPU fallback" if not torch.cuda.is_available() else "one HIP device"
    with pytest.raises(IconAmdError, match=host):
        local_affine_device(x, A, b, topo)
    with pytest.raises(IconAmdError, match=host):
        mesh_shape_prior_losses_device(verts, topo)
    with pytest.raises(IconAmdError, match=host):
        update_mesh_shape_prior_losses(verts[None], torch.from_numpy(f)[None], losses)
    with pytest.raises(IconAmdError, match=host):
        LocalAffine(V, 1, topo.edges)(x)


def test_native_cloth_entries_refuse_bad_arguments_with_messages():
    names = ("icon_local_affine_bytes", "icon_local_affine_forward", "icon_local_affine_backward",
             "icon_mesh_priors_bytes", "icon_mesh_priors_forward", "icon_mesh_priors_backward")
    for s in names:
        assert s in _lib.SYMBOLS
    lib = _lib.lib()
    i64, n = C.c_int64, C.c_int64(0)
    assert lib.icon_local_affine_bytes(i64(1), i64(6890), i64(20664), C.byref(n)) == 0 and n.value >= 81 * 16 and n.value % 256 == 0
    assert lib.icon_local_affine_bytes(i64(0), i64(10), i64(10), C.byref(n)) == 1 and b"positive" in lib.icon_last_error()
    assert lib.icon_local_affine_bytes(i64(1), i64(10), i64(-1), C.byref(n)) == 1 and b"negative" in lib.icon_last_error()
    assert lib.icon_local_affine_bytes(i64(1), i64(10), i64(10), None) == 1 and b"null" in lib.icon_last_error()
    assert lib.icon_mesh_priors_bytes(i64(6890), i64(20664), i64(20664), C.byref(n)) == 0
    assert n.value >= 81 * 24 + 6890 * 24 + 20664 * 48 and n.value % 256 == 0
    assert lib.icon_mesh_priors_bytes(i64(0), i64(1), i64(1), C.byref(n)) == 1 and b"positive" in lib.icon_last_error()
    assert lib.icon_mesh_priors_bytes(i64(10), i64(1), i64(1), None) == 1 and b"null" in lib.icon_last_error()
    # host buffers are enough to reach the checks: nothing is launched before they pass
    buf = np.zeros(4096, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 256
    p, odd, f0 = C.c_void_p(base), C.c_void_p(base + 4), C.c_float(0.0)
    la_f = lambda scratch, nbytes, y=p: lib.icon_local_affine_forward(p, p, p, i64(1), i64(3), p, i64(3), C.c_int(1), y, p, p, scratch, i64(nbytes), None)
    la_b = lambda g=p: lib.icon_local_affine_backward(p, p, p, i64(1), i64(3), p, p, i64(3), C.c_int(1), g, p, p, p, p, None)   # a single gather: no scratch
    mp_f = lambda scratch, nbytes, o=p, terms=7: lib.icon_mesh_priors_forward(p, i64(3), p, p, p, i64(3), p, i64(1), C.c_int(1), f0, C.c_int(terms), o, p, p,
                                                                              scratch, i64(nbytes), None)
    mp_b = lambda scratch, nbytes, g=p, terms=7: lib.icon_mesh_priors_backward(p, i64(3), p, p, p, i64(3), p, p, p, i64(1), C.c_int(1), f0, C.c_int(terms),
                                                                               g, p, p, p, scratch, i64(nbytes), None)
    for call in (la_f, mp_f, mp_b):
        assert call(odd, 1 << 30) == 1 and b"aligned" in lib.icon_last_error()
        assert call(p, 16) == 1 and b"scratch" in lib.icon_last_error()
        assert call(p, 1 << 30, None) == 1 and b"null" in lib.icon_last_error()
    assert la_b(None) == 1 and b"null" in lib.icon_last_error()
    assert lib.icon_local_affine_backward(p, p, p, i64(0), i64(3), p, p, i64(3), C.c_int(1), p, p, p, p, p, None) == 1 and b"positive" in lib.icon_last_error()
    for call in (mp_f, mp_b):
        assert call(p, 1 << 30, p, 0) == 1 and b"terms" in lib.icon_last_error()
        assert call(p, 1 << 30, p, 8) == 1 and b"terms" in lib.icon_last_error()

"""Device marching cubes (csrc/mc_device.hip) at every size class, level and slab cut - the cases of tests/mc_cases.py.

What the rest of the suite leaves out: it runs the device kernels at res 33 / 49 / 65 / 129 / 257 / 513 and level 0.5 only, so
k_mc_classify (one cell per thread: every res with (res - 1) % 4 != 0) never ran, nor a volume smaller than one workgroup, nor a
level other than 0.5, nor the block counts around the switch between the two scans of the block totals (8,192 blocks: res 204 |
205), nor a Z-slab range (icon_mc_count_range / icon_mc_emit_keyed) outside the multi-process worker's balanced cuts.

The reference of a mesh is oracle/mc_classic.py (the published classic algorithm in float64, numpy); tests/test_mc_cases.py runs
the same comparison on the host implementation without a GPU and asserts what each case contains."""
import ctypes as C
from contextlib import contextmanager
from functools import lru_cache

import numpy as np
import pytest
import torch

import mc_cases as mc
from common import set_option

pytestmark = pytest.mark.gpu

ICON_ERR_ARG = 1


def _dev():
    return torch.device("cuda", 0)


def T(vol):
    return torch.from_numpy(np.array(vol, np.float32)).to(_dev())          # (a copy: the shared cases are read-only)


@contextmanager
def classify1(on):
    """the "mc_classify1" switch for the block; off (the default) afterwards"""
    set_option("mc_classify1", on)
    try:
        yield
    finally:
        set_option("mc_classify1", 0)


@lru_cache(maxsize=None)
def _case(kind, res, level_id):
    """(volume, level, classic vertices, classic faces): computed once, shared, never written to"""
    if kind in ("ellipsoid", "slab_sparse"):
        vol, level = getattr(mc, kind)(res), 0.5
        cv, cf = mc.classic_mesh(vol, level, blocks=True)
    else:
        vol, level = mc.case(kind, res, level_id)
        cv, cf = mc.classic_mesh(vol, level)
    for a in (vol, cv, cf):
        a.setflags(write=False)
    return vol, level, cv, cf


def _check_against_classic(v, f, kind, res, level_id, what):
    _, _, cv, cf = _case(kind, res, level_id)
    c = mc.compare_with_classic(v.cpu().numpy(), f.cpu().numpy(), cv, cf, mc.vertex_bound(res))
    print(f"{what} res {res} {kind} level {level_id}: {c['verts'][0]} vertices, {c['faces'][0]} faces, "
          f"max_vertex_diff {c['max_vertex_diff']:.3e} (bound {c['bound']:.3e})")
    mc.assert_same_as_classic(c)
    return c


def _mc_on(work, occ, level):
    """icon_mc_count + icon_mc_emit on a given workspace (export_mesh_device's calls)"""
    from icon_amd import _lib
    from icon_amd._native import stream
    L = _lib.lib()
    nv, nf = C.c_int64(0), C.c_int64(0)
    _lib.check(L.icon_mc_count(_lib.ptr(occ), C.c_int(occ.shape[0]), C.c_float(level), work.h, stream(), C.byref(nv), C.byref(nf)), "icon_mc_count")
    verts = torch.empty((max(nv.value, 1), 3), dtype=torch.float32, device=occ.device)
    faces = torch.empty((max(nf.value, 1), 3), dtype=torch.int64, device=occ.device)
    if nv.value and nf.value:
        _lib.check(L.icon_mc_emit(_lib.ptr(verts), _lib.ptr(faces), work.h, stream()), "icon_mc_emit")
    return verts[: nv.value], faces[: nf.value]


# ---------------------------------------------------------------------------------------------
# a. both classify kernels against the independent reference
# ---------------------------------------------------------------------------------------------
def _vs_classic_and_host(res, kind, level_id):
    from icon_amd.recon import export_mesh_device, export_mesh_numpy
    from test_gpu_parity import _canonical_mesh
    vol, level, cv, cf = _case(kind, res, level_id)
    v, f = export_mesh_device(T(vol), level)
    assert v.dtype == torch.float32 and f.dtype == torch.int64
    _check_against_classic(v, f, kind, res, level_id, "device")
    assert len(cf) > 0 or (kind == "border" and res == 3)         # (res 3's cropped grid is all shell: the empty mesh)
    vh, fh = export_mesh_numpy(vol, level)
    assert v.shape == vh.shape and f.shape == fh.shape
    if len(fh):
        a, b = _canonical_mesh(v.cpu().numpy(), f.cpu().numpy()), _canonical_mesh(vh.numpy(), fh.numpy())
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])          # vertices bit for bit, same triangles


@pytest.mark.parametrize("level_id", mc.LEVELS)
@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("res", mc.SIZES_SMALL)
def test_small_sizes_vs_classic_marching_cubes(res, kind, level_id):
    """one cube ... 17^3 cells, all four residues of (res - 1) % 4: fewer cells than a workgroup, a last workgroup that is partly
    empty and holds crossings, a multiple of 1,024 cells (res 17) and one row past it (res 18); three levels, 0.37 not a float32"""
    _vs_classic_and_host(res, kind, level_id)


@pytest.mark.parametrize("level_id", mc.LEVELS)
@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("res", mc.SIZES_MID)
def test_mid_sizes_vs_classic_marching_cubes(res, kind, level_id):
    """res 34 / 35 / 36 / 50 (k_mc_classify) and 37 (k_mc_classify4): dozens of workgroups, every cube configuration"""
    _vs_classic_and_host(res, kind, level_id)


# ---------------------------------------------------------------------------------------------
# b. the two classify kernels on one volume
# ---------------------------------------------------------------------------------------------
def _both_ways(vol, level):
    from icon_amd.recon import export_mesh_device
    occ = T(vol)
    with classify1(0):
        v4, f4 = export_mesh_device(occ, level)
    with classify1(1):
        v1, f1 = export_mesh_device(occ, level)
    assert torch.equal(v4, v1) and torch.equal(f4, f1)           # same order, not only the same sets
    return len(f4)


def _switch_cases(res):
    if res == 205:
        return [("ellipsoid", "0.5"), ("slab_sparse", "0.5")]
    return [(kind, level_id) for kind in mc.KINDS for level_id in mc.LEVELS]


@pytest.mark.parametrize("res", [5, 9, 13, 17, 33, 37, 205])
def test_one_cell_and_four_cell_classification_give_the_same_mesh(res):
    """(res - 1) % 4 == 0: k_mc_classify4 serves the size, "mc_classify1" forces k_mc_classify - "bit-for-bit the same flags /
    counts" (mc_device.hip), so the same vertices and faces in the same order"""
    faces = 0
    for kind, level_id in _switch_cases(res):
        vol, level = _case(kind, res, level_id)[:2] if res != 33 else mc.case(kind, res, level_id)
        faces += _both_ways(vol, level)
    assert faces > 0
    print(f"res {res}: {len(_switch_cases(res))} cases, {faces} faces")


@pytest.mark.parametrize("res", [4, 6, 7, 34, 35, 36])
def test_the_switch_changes_nothing_where_only_one_kernel_serves(res):
    for kind, level_id in _switch_cases(res):
        vol, level = _case(kind, res, level_id)[:2]
        assert _both_ways(vol, level) > 0


# ---------------------------------------------------------------------------------------------
# c. the scan switch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ellipsoid", "slab_sparse"])
@pytest.mark.parametrize("res,one_cell", [(204, 0), (205, 0), (205, 1), (206, 0)])
def test_scan_switch_vs_classic_marching_cubes(res, one_cell, kind):
    """204: 8,170 block totals, one-workgroup scan (k_mc_scanblocks), one-cell classification; 205: 8,291, the two-pass scan
    (k_mc_scan_local / _apply), four-cell classification - and one-cell by the switch; 206: two-pass, one-cell"""
    from icon_amd.recon import export_mesh_device
    vol, level, _, cf = _case(kind, res, "0.5")
    with classify1(one_cell):
        v, f = export_mesh_device(T(vol), level)
    assert len(cf) > 40000
    _check_against_classic(v, f, kind, res, "0.5", f"device (mc_classify1 = {one_cell})")


# ---------------------------------------------------------------------------------------------
# d. slab ranges in one process
# ---------------------------------------------------------------------------------------------
def _slab_merge(occ, cuts, level):
    """the parts [c_i, c_i+1) of the planes through DenseReconEngine._hip_slab_mesh with the arguments _gather_mesh forms, one
    after the other on the one marching-cubes workspace, merged by key -> (verts, faces, vertices per part)"""
    from icon_amd.recon import DenseReconEngine, merge_keyed_meshes
    res = occ.shape[0]
    assert cuts[0] == 0 and cuts[-1] == res and all(a < b for a, b in zip(cuts[:-1], cuts[1:]))
    keys, verts, faces, per = [], [], [], []
    for z0, z1 in zip(cuts[:-1], cuts[1:]):
        nz, halo = z1 - z0, z1 < res                              # every part is non-empty: the next part's first plane is plane z1
        buf = torch.zeros((nz + 1, res, res), dtype=torch.float32, device=occ.device)
        buf[:nz] = occ[z0:z1]
        if halo:
            buf[nz] = occ[z1]
        zc0, zc1 = max(z0 - 1, 0), (z1 - 1 if halo else res - 1)
        if zc1 <= zc0:
            per.append(None)
            continue
        k, v, f = DenseReconEngine._hip_slab_mesh(buf, z0, res, zc0, zc1, halo, level)
        keys.append(k); verts.append(v); faces.append(f); per.append(int(k.shape[0]))
    mv, mf = merge_keyed_meshes(keys, verts, faces)
    return mv, mf, per


def _all_cuts_restore_the_whole_mesh(vol, level, cuts_list, one_cell):
    from icon_amd.recon import export_mesh_device
    occ = T(vol)
    with classify1(one_cell):
        wv, wf = export_mesh_device(occ, level)
        assert len(wf) > 0
        for cuts in cuts_list:
            mv, mf, _ = _slab_merge(occ, cuts, level)
            assert torch.equal(mv, wv) and torch.equal(mf, wf), cuts


@pytest.mark.parametrize("res,one_cell", [(6, 0), (9, 0), (9, 1), (34, 0), (37, 0), (37, 1)])
def test_every_single_cut_restores_the_whole_mesh(res, one_cell):
    """two parts, the cut at every plane 1 .. res - 1 (a one-plane first part triangulates nothing, a one-plane last part the top
    layer alone): merged, the same vertices and faces in the same order as marching cubes on the whole volume"""
    for kind, level_id in (("noise", "0.5"), ("at_level", "0.37")):
        vol, level = _case(kind, res, level_id)[:2]
        _all_cuts_restore_the_whole_mesh(vol, level, mc.plane_cuts(res, 1), one_cell)


@pytest.mark.parametrize("res,one_cell", [(9, 0), (9, 1), (10, 0)])
def test_every_pair_of_cuts_restores_the_whole_mesh(res, one_cell):
    """three parts, one-plane parts in the middle included"""
    vol, level = _case("noise", res, "0.37")[:2]
    cuts = mc.plane_cuts(res, 2)
    assert any(b - a == 1 for c in cuts for a, b in zip(c[:-1], c[1:]))
    _all_cuts_restore_the_whole_mesh(vol, level, cuts, one_cell)


@pytest.mark.parametrize("res,one_cell", [(37, 0), (37, 1), (50, 0)])
def test_slabs_without_any_crossing(res, one_cell):
    """the ellipsoid in the middle third of z, cut into three and four parts: parts whose layers hold no crossing return nothing
    and the rest still merges into the whole mesh - and a small range after a large one on the one workspace"""
    from icon_amd.recon import export_mesh_device
    vol = _case("slab_sparse", res, "0.5")[0]
    occ = T(vol)
    q = res // 4
    with classify1(one_cell):
        wv, wf = export_mesh_device(occ, 0.5)
        for cuts in ((0, res // 3, 2 * res // 3, res), (0, q, 2 * q, 3 * q, res), (0, res - 6, res - 3, res), (0, 2, res // 2, res - 1, res)):
            mv, mf, per = _slab_merge(occ, cuts, 0.5)
            assert torch.equal(mv, wv) and torch.equal(mf, wf), cuts
            assert 0 in per and max(p or 0 for p in per) > 100, (cuts, per)


@pytest.mark.parametrize("res,one_cell", [(9, 0), (9, 1), (10, 0)])
def test_one_layer_range_with_a_halo(res, one_cell):
    """icon_mc_count_range with zc0 == zc1 and halo = 1: no layer of its own, the halo layer alone - the crossings of that
    layer's x and y edges, no face; the keyed vertices are the rows of the whole-volume call with those keys"""
    from icon_amd.recon import DenseReconEngine
    vol, level = _case("noise", res, "0.5")[:2]
    occ = T(vol)
    n = res - 1
    crossed = mc.crossed_edges(vol, level)
    with classify1(one_cell):
        wk, wv, _ = DenseReconEngine._hip_slab_mesh(occ, 0, res, 0, res - 1, False, level)
        assert torch.equal(wk, torch.sort(wk)[0]) and len(torch.unique(wk)) == len(wk)
        for zc in range(0, res - 1):
            k, v, f = DenseReconEngine._hip_slab_mesh(occ, 0, res, zc, zc, True, level)
            want = int(crossed[2][zc].sum() + crossed[1][zc].sum())
            assert f.shape[0] == 0 and k.shape[0] == want and want > 0, (zc, k.shape, f.shape, want)
            rows = (torch.div(wk, 3 * n * n, rounding_mode="floor") == zc) & (wk % 3 < 2)
            assert torch.equal(k, wk[rows]) and torch.equal(v, wv[rows]), zc


def test_range_arguments_are_refused_before_any_launch():
    from icon_amd import _lib
    from icon_amd.engine import Workspace
    from icon_amd._native import stream
    L = _lib.lib()
    occ = T(mc.noise(9, 1))
    work = Workspace()
    nv, nf = C.c_int64(-1), C.c_int64(-1)

    def count(res, zc0, zc1, halo):
        return L.icon_mc_count_range(_lib.ptr(occ), C.c_int(res), C.c_float(0.5), C.c_int(zc0), C.c_int(zc1), C.c_int(halo), work.h, stream(),
                                     C.byref(nv), C.byref(nf))
    for args in ((9, 3, 2, 0), (9, 0, 9, 0), (9, 0, 8, 1), (9, -1, 4, 0), (2, 0, 1, 0), (1292, 0, 1291, 0)):
        assert count(*args) == ICON_ERR_ARG and b"icon_mc_count" in L.icon_last_error(), args
        assert nv.value == -1 and nf.value == -1
    # nothing was counted: the workspace still refuses an emit
    v, f = torch.empty((8, 3), device=occ.device), torch.empty((8, 3), dtype=torch.int64, device=occ.device)
    assert L.icon_mc_emit(_lib.ptr(v), _lib.ptr(f), work.h, stream()) == ICON_ERR_ARG
    assert count(9, 0, 8, 0) == 0 and nv.value > 0 and nf.value > 0


# ---------------------------------------------------------------------------------------------
# e. one workspace, many sizes
# ---------------------------------------------------------------------------------------------
def test_one_workspace_serves_shrinking_and_growing_volumes():
    """205 -> 5 -> 50 -> 4 -> 205 on the shared workspace: both scans, both classify kernels, the arrays keep their capacity
    (and the larger call's contents) while npts shrinks - every mesh equals the same call on a fresh workspace"""
    from icon_amd.engine import Workspace
    from icon_amd.recon import _mc_workspace
    shared = _mc_workspace(_dev())
    seq = [("ellipsoid", 205, "0.5"), ("noise", 5, "0.37"), ("at_level", 50, "0.5"), ("noise", 4, "0.5"), ("slab_sparse", 205, "0.5")]
    for kind, res, level_id in seq:
        vol, level = _case(kind, res, level_id)[:2]
        occ = T(vol)
        v, f = _mc_on(shared, occ, level)
        fv, ff = _mc_on(Workspace(), occ, level)
        assert len(ff) > 0 and torch.equal(v, fv) and torch.equal(f, ff), (kind, res)


def test_emit_needs_exactly_one_count():
    from icon_amd import _lib
    from icon_amd.engine import Workspace
    from icon_amd._native import stream
    L = _lib.lib()
    occ = T(mc.noise(6, 2))
    work = Workspace()
    v, f = torch.empty((400, 3), device=occ.device), torch.empty((400, 3), dtype=torch.int64, device=occ.device)
    assert L.icon_mc_emit(_lib.ptr(v), _lib.ptr(f), work.h, stream()) == ICON_ERR_ARG            # no count before it
    nv, nf = C.c_int64(0), C.c_int64(0)
    assert L.icon_mc_count(_lib.ptr(occ), C.c_int(6), C.c_float(0.5), work.h, stream(), C.byref(nv), C.byref(nf)) == 0
    assert 0 < nv.value <= 400 and 0 < nf.value <= 400
    assert L.icon_mc_emit(_lib.ptr(v), _lib.ptr(f), work.h, stream()) == 0
    assert L.icon_mc_emit(_lib.ptr(v), _lib.ptr(f), work.h, stream()) == ICON_ERR_ARG            # a second emit after one count
    assert b"icon_mc_count first" in L.icon_last_error()


# ---------------------------------------------------------------------------------------------
# f. through the public entry points
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(7, 12, 9), (36, 20, 33)])
def test_export_mesh_of_a_box_volume_device_vs_host(shape):
    """DenseReconEngine.export_mesh pads a (D, H, W) volume to its longest axis - 12 and 36 here: one-cell sizes - the device path
    against the host path on the same volume"""
    from icon_amd.recon import DenseReconEngine
    from test_gpu_parity import _canonical_mesh
    D, H, W = shape
    vol = mc.noise_box(shape, 40 + D)
    # (the constructor insists on odd W and H, as upstream's does, and on a query function for per-axis resolutions; export_mesh
    # reads the shape of the volume it is handed alone)
    from icon_amd.engine import query_func
    eng = DenseReconEngine(query_func=query_func, resolutions=[(W | 1, H | 1, D)], align_corners=True)
    vd, fd = eng.export_mesh(T(vol))
    vh, fh = eng.export_mesh(torch.from_numpy(vol))
    assert not vd.is_cuda and vd.shape == vh.shape and fd.shape == fh.shape and len(fh) > 100
    a, b = _canonical_mesh(vd.numpy(), fd.numpy()), _canonical_mesh(vh.numpy(), fh.numpy())
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert float(vd[:, 0].max()) <= W - 1 and float(vd[:, 1].max()) <= H - 1 and float(vd[:, 2].max()) <= D - 1      # the padding adds nothing beyond the box


@pytest.mark.parametrize("res", [4] + mc.SIZES_MID)
def test_clean_mesh_of_one_cell_sizes_vs_plain_python_checker(res):
    """clean_mesh(*export_mesh_device(...)) on the noise cases - thousands of components, pinch vertices - and on a mesh of a few
    faces: vertex for vertex and face for face what oracle/mc_check.py: largest_component_by_faces keeps"""
    from icon_amd.recon import clean_mesh, export_mesh_device
    from oracle.mc_check import largest_component_by_faces
    vol, level = _case("noise", res, "0.5")[:2]
    v, f = export_mesh_device(T(vol), level)
    cv, cf = clean_mesh(v, f)
    ev, ef = largest_component_by_faces(v.cpu().numpy(), f.cpu().numpy())
    assert 0 < len(ef) <= len(f)
    assert np.array_equal(cv.cpu().numpy(), ev) and np.array_equal(cf.cpu().numpy(), ef)

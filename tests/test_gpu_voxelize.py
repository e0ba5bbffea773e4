"""GPU: icon_semantic_voxelize and icon_semantic_voxelize_batch (icon_amd/csrc/vox_kernels.hip) against the independent float64
reference (tests/vox_reference.py) on the cases of tests/vox_cases.py - both orientations, sizes that leave a partial last
workgroup, surface-vertex counts around the LDS tile, tetrahedra across and outside the cube, skipped rows, T = 0, three sigmas.

Both entries are called through the C ABI, so the test owns the buffers: the volume is filled with NaN and the occupancy scratch
with 0xAB before every call (every voxel must be written, outside ones as exact 0.0), and the occupancy compared with the
reference is the uint8 array the batch entry leaves in d_occ, not "value != 0".  The single-subject entry has no such output:
its values must equal the batch entry's bit for bit.

Acceptance per case (vox_cases.compare): the reference's undecided voxels <= 0.5 % of its occupied ones (asserted before the
result is read; exactly 0 for `lattice`), occupancy equal on every decided voxel, outside voxels exactly 0, values within 1e-5
(the bound of tests/test_voxelize.py) at every sigma."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_pamir as bp  # noqa: E402
import vox_cases as vc  # noqa: E402
from icon_amd import _lib  # noqa: E402
from icon_amd._lib import check, ptr  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_batch(verts, n_surface, table, tets, res, sigma=0.05, device_inputs=None):
    """verts [B,V,3] -> (out [B,R,R,R,3] f32, occ [B,R,R,R] u8) device tensors, on torch's current stream.  The code table
    buffer has V rows, huge past n_surface; the entry is told n_surface."""
    v, code, t = device_inputs if device_inputs is not None else (T(verts), T(table), T(tets))
    B, V = v.shape[0], v.shape[1]
    out = torch.full((B, res, res, res, 3), float("nan"), dtype=torch.float32, device=DEV)
    occ = torch.full((B, res, res, res), 0xAB, dtype=torch.uint8, device=DEV)
    check(_lib.lib().icon_semantic_voxelize_batch(ptr(v), C.c_int(B), C.c_int64(V), C.c_int64(n_surface), ptr(code), ptr(t),
                                                  C.c_int64(t.shape[0]), C.c_int(res), C.c_float(sigma), ptr(occ), ptr(out), _stream()),
          "icon_semantic_voxelize_batch")
    return out, occ


def run_single(verts, n_surface, table, tets, res, sigma=0.05):
    v, code, t = T(verts), T(table), T(tets)
    out = torch.full((res, res, res, 3), float("nan"), dtype=torch.float32, device=DEV)
    check(_lib.lib().icon_semantic_voxelize(ptr(v), C.c_int64(v.shape[0]), C.c_int64(n_surface), ptr(code), ptr(t),
                                            C.c_int64(t.shape[0]), C.c_int(res), C.c_float(sigma), ptr(out), _stream()),
          "icon_semantic_voxelize")
    return out


def voxelise(name, res, sigma=0.05):
    """one case through both entries: the poison is gone, the two volumes are equal bit for bit, and the batch entry's volume
    and occupancy meet the reference.  Returns (out, occ) as numpy and the largest value difference."""
    vc.check_cap(name, res, sigma)                          # the condition on the inputs, before any result exists
    c = vc.get(name)
    out, occ = run_batch(c["verts"][None], c["n_surface"], c["table"], c["tets"], res, sigma)
    one = run_single(c["verts"], c["n_surface"], c["table"], c["tets"], res, sigma)
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and not torch.isnan(one).any()
    assert bool(((occ == 0) | (occ == 1)).all())
    assert torch.equal(out[0], one)
    out, occ = out[0].cpu().numpy(), occ[0].cpu().numpy()
    err = vc.compare(name, res, sigma, out, occ, TOL)
    return out, occ, err


@pytest.mark.parametrize("res", [32, 33])
def test_mirrored(res):
    """every volume negative: the arm of the orientation switch no tetrahedron of the body takes.  The same solid: bit-equal."""
    assert (vc.orientation(vc.body()) > 0).all() and (vc.orientation(vc.mirrored()) < 0).all()
    out, occ, _ = voxelise("mirrored", res)
    out0, occ0, _ = voxelise("body", res)
    assert np.array_equal(occ, occ0) and np.array_equal(out, out0)


@pytest.mark.parametrize("res", [20, 33, 2, 3, 5, 48])
def test_mixed_and_sizes(res):
    """random tetrahedra of both orientations; res^3 is a multiple of the 256-voxel workgroup only at 48"""
    o = vc.orientation(vc.mixed())
    assert (o > 0).mean() >= 0.25 and (o < 0).mean() >= 0.25
    _, occ, _ = voxelise("mixed", res)
    if res in (20, 33):
        assert 0.05 <= occ.mean() <= 0.60


def test_body_128():
    voxelise("body", 128)


def test_lattice_no_voxel_exempt():
    """exact inputs: centres on faces, edges and vertices must be inside, and no voxel is excused"""
    assert vc.boundary_hits(vc.lattice(), vc.LATTICE_RES) >= 50
    _, _, und = vc.check_cap("lattice", vc.LATTICE_RES)
    assert not und.any()
    voxelise("lattice", vc.LATTICE_RES)


@pytest.mark.parametrize("name,res", [("clamps", 20), ("clamps", 33), ("clamps_big", 20)])
def test_clamps(name, res):
    _, occ, _ = voxelise(name, res)
    assert occ.all() if name == "clamps_big" else (occ.any() and not occ.all())
    if name == "clamps":
        assert all(np.moveaxis(occ, k, 0)[i].any() for k in range(3) for i in (0, -1))


@pytest.mark.parametrize("res", [20, 33])
def test_skipped_rows(res):
    """indices -1, V, 2^40 and zero-volume rows between valid ones change nothing; no tetrahedra at all gives all zeros"""
    out, occ, _ = voxelise("skipped", res)
    out0, occ0, _ = voxelise("skipped_valid", res)
    assert np.array_equal(occ, occ0) and np.array_equal(out, out0)
    c = vc.get("skipped")
    none = torch.zeros((0, 4), dtype=torch.int64, device=DEV)
    outb, occb = run_batch(None, c["n_surface"], None, None, res, device_inputs=(T(c["verts"][None]), T(c["table"]), none))
    out1 = torch.full((res, res, res, 3), float("nan"), dtype=torch.float32, device=DEV)
    v, code = T(c["verts"]), T(c["table"])
    check(_lib.lib().icon_semantic_voxelize(ptr(v), C.c_int64(len(v)), C.c_int64(c["n_surface"]), ptr(code), C.c_void_p(0), C.c_int64(0),
                                            C.c_int(res), C.c_float(0.05), ptr(out1), _stream()), "icon_semantic_voxelize")
    torch.cuda.synchronize()
    assert bool((outb == 0).all()) and bool((occb == 0).all()) and bool((out1 == 0).all())


@pytest.mark.parametrize("n_surface", vc.TILE_SURFACES)
def test_surface_vertex_counts(n_surface):
    """1, 255, 256, 257, 513 surface vertices around the 256-vertex LDS tile; the rows of the table past them are 1e30"""
    out, _, _ = voxelise(f"tiles{n_surface}", 20)
    assert np.abs(out).max() <= 1.0


@pytest.mark.parametrize("sigma", [0.002, 0.005, 0.05, 0.5])
def test_sigma(sigma):
    """measured max |value - reference| on the body at res 32: see DESIGN.md section 4.8.  At 0.002 the reference has occupied
    voxels whose value is below float32's smallest normal (tests/test_vox_reference.py::tiny_values): the kernel's value there
    is 0 or denormal and only the occupancy array can tell them from outside voxels."""
    out, occ, err = voxelise("body", 32, sigma)
    zero_in = int(((np.abs(out).sum(-1) == 0) & (occ == 1)).sum())
    print(f"sigma {sigma}: max |value - reference| {err:.3e}; {zero_in} occupied voxels with an all-zero value")
    if sigma == 0.002:
        values, sure_in, _ = vc.reference("body", 32, sigma)
        assert (sure_in & (np.abs(values).max(-1) < np.finfo(np.float32).tiny)).any()


@pytest.mark.parametrize("B", [1, 3, 5])
def test_batch(B):
    """unlike subjects in one launch; permuted subjects give permuted volumes bit for bit; B = 3 runs on a side stream behind a
    fill of its inputs queued on that stream (an entry that ignored its stream argument would read the unfilled buffers)"""
    S = bp.subjects(B)
    b0 = vc.body()
    res = 33
    for b in range(B):
        vc.check_cap(f"subject{b}of{B}", res)
    args = (b0["n_surface"], b0["table"], b0["tets"], res)
    if B == 3:
        side = torch.cuda.Stream()
        src = (T(S["verts"]), T(b0["table"]), T(b0["tets"]))
        dst = tuple(torch.zeros_like(x) for x in src)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for d, s in zip(dst, src):
                d.copy_(s, non_blocking=True)                 # the inputs exist only once this stream has run
            out, occ = run_batch(None, *args[:1], None, None, res, device_inputs=dst)
        side.synchronize()
    else:
        out, occ = run_batch(S["verts"], *args)
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and bool(((occ == 0) | (occ == 1)).all())
    for b in range(B):
        vc.compare(f"subject{b}of{B}", res, 0.05, out[b].cpu().numpy(), occ[b].cpu().numpy(), TOL)
    perm = np.random.RandomState(B).permutation(B) if B > 1 else np.array([0])
    outp, occp = run_batch(S["verts"][perm], *args)
    torch.cuda.synchronize()
    assert torch.equal(outp, out[T(perm)]) and torch.equal(occp, occ[T(perm)])

"""icon_query_color / icon_amd.recon.query_color on the device against the CPU checker (tests/color_checker.py, pinned against the
reference's own function by tests/test_query_color.py) and against the stored verbatim run (tests/golden/query_color_ref.npz).

Bars.  Visible set: equal to oracle.visibility and to get_visibility on the same arguments.  Normal branch: bit-equal to the
checker (S1 fixes the order of every addition).  Sampled branch: within color_checker.SAMPLED_GPU_BAR = 4 x 6.8e-4 = 2.72e-3
colour units (0..255) of the checker - 6.8e-4 is the largest distance of the checker itself from float64 on these meshes
(test_checker_sampled_branch_vs_float64).  Observed on the MI355X: body, icosphere, offset icosphere and fan 1.53e-5, bumped
level-7 icosphere and the marching-cubes 257^3 mesh 3.05e-5 - one or two ulps of a colour near 255 - and the bytes are NOT equal
to torch's CPU grid_sample on any mesh (it unnormalises as (x + 1) * ((W - 1) / 2) and takes the far weights as 1 - w; the device
uses ATen's CUDA form), so the bar is asserted, not equality; each test prints the distance it saw."""
import ctypes as C

import numpy as np
import pytest
import torch

import color_checker as cc
from common import assets, golden, orc

pytestmark = pytest.mark.gpu


def _dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dtype is None else t.to(dtype)


def _mc_mesh_device():
    """the cleaned marching-cubes mesh of the dense 257^3 synthetic volume, in the [-1,1] cube (apps/ICON.py:755-759), on the device"""
    from icon_amd.recon import clean_mesh, export_mesh_device
    from test_gpu_parity import make_engine, T
    a = assets("body")
    occ = make_engine(a).eval_slab(T(a.features), 257, 0, 257)
    v, f = clean_mesh(*export_mesh_device(occ, 0.5))
    return (v.float() - 128.0) / 128.0, f, occ


def _compare(name, v, f, image, colors, vis):
    """colors / vis: what the device returned for (v, f) numpy"""
    from icon_amd.engine import get_visibility
    want, want_vis = cc.checker_query_color(v, f, image)
    frac = cc.assert_both_branches(want_vis)
    vis = vis.cpu().numpy()
    assert np.array_equal(vis, want_vis), f"{name}: {(vis != want_vis).sum()} vertices differ from oracle.visibility"
    vt = torch.from_numpy(v)
    old = get_visibility(vt[:, :2], vt[:, 2:3], torch.from_numpy(f[:, [0, 2, 1]].copy()))[:, 0].numpy()
    assert np.array_equal(vis, old), f"{name}: differs from get_visibility"
    got, want = colors.cpu().numpy(), want.numpy()
    hidden = want_vis == 0
    assert np.array_equal(got[hidden], want[hidden]), f"{name}: normal branch, max |d| = {np.abs(got[hidden] - want[hidden]).max()}"
    d = float(np.abs(got[~hidden].astype(np.float64) - want[~hidden]).max())
    print(f"{name}: {len(v)} vertices, {len(f)} faces, {100 * frac:.1f} % visible; sampled branch max |device - checker| = {d:.3e}"
          f" (bar {cc.SAMPLED_GPU_BAR:.2e}; bit-equal: {np.array_equal(got[~hidden], want[~hidden])})")
    assert d <= cc.SAMPLED_GPU_BAR
    return got


@pytest.mark.parametrize("mesh", ["body", "ico"])
def test_gpu_query_color_vs_the_stored_reference_run(mesh):
    from icon_amd.recon import query_color
    g = golden("query_color_ref.npz")
    v, f = cc.MESHES[mesh]()
    out = query_color(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(g["image"]))
    assert out.dtype == torch.float32 and out.shape == (len(v), 3) and out.device.type == "cpu"
    got, want, hidden = out.numpy(), g[f"{mesh}_colors"], g[f"{mesh}_vis"] == 0
    cc.assert_both_branches(g[f"{mesh}_vis"])
    assert np.array_equal(got[hidden], want[hidden])
    d = float(np.abs(got[~hidden].astype(np.float64) - want[~hidden]).max())
    print(f"{mesh}: sampled branch max |device - reference| = {d:.3e}")
    assert d <= cc.SAMPLED_GPU_BAR
    assert 0.0 <= got.min() and got.max() <= 255.0


@pytest.mark.parametrize("mesh", ["body", "ico", "ico_offset", "bumpy_ico"])
def test_gpu_query_color_vs_checker(mesh):
    from icon_amd.recon import query_color_device
    v, f = (cc.MESHES.get(mesh) or cc.bumpy_ico)()
    image = cc.make_image()
    colors, vis = query_color_device(_dev(v), _dev(f), image.cuda(), return_vis=True)
    assert colors.is_cuda and colors.shape == (len(v), 3) and vis.shape == (len(v),)
    _compare(mesh, v, f, image, colors, vis)


def test_gpu_query_color_on_the_marching_cubes_mesh_index_types_determinism_and_stream_order():
    """the mesh the call is made on upstream: export_mesh_device -> clean_mesh -> query_color_device enqueued back to back (no
    synchronisation of ours in between) against the checker and against the host-tensor call; int32 faces (clean_mesh's) and int64
    faces give the same bytes; so do two runs"""
    from icon_amd.recon import query_color, query_color_device
    v, f32, _ = _mc_mesh_device()
    image = cc.make_image()
    img_d = image.cuda()
    assert f32.dtype == torch.int32 and f32.is_cuda and v.is_cuda
    colors, vis = query_color_device(v, f32, img_d, return_vis=True)            # straight behind clean_mesh on the stream
    again, vis2 = query_color_device(v, f32, img_d, return_vis=True)
    c64, vis64 = query_color_device(v, f32.long(), img_d, return_vis=True)
    host = query_color(v.cpu(), f32.cpu(), image)
    vn, fn = v.cpu().numpy(), f32.cpu().numpy().astype(np.int64)
    assert len(vn) > 50_000 and len(fn) > 100_000
    got = _compare("marching cubes 257^3", vn, fn, image, colors, vis)
    assert got.tobytes() == again.cpu().numpy().tobytes() and vis.cpu().numpy().tobytes() == vis2.cpu().numpy().tobytes()
    assert got.tobytes() == c64.cpu().numpy().tobytes() and vis.cpu().numpy().tobytes() == vis64.cpu().numpy().tobytes()
    assert got.tobytes() == host.numpy().tobytes()


@pytest.mark.parametrize("mesh", ["body", "bumpy_ico"])
def test_gpu_query_color_index_types_and_determinism(mesh):
    from icon_amd.recon import query_color_device
    v, f = (cc.MESHES.get(mesh) or cc.bumpy_ico)()
    img_d = cc.make_image().cuda()
    a = query_color_device(_dev(v), _dev(f), img_d).cpu().numpy()
    b = query_color_device(_dev(v), _dev(f), img_d).cpu().numpy()
    c = query_color_device(_dev(v), _dev(f, torch.int32), img_d).cpu().numpy()
    assert a.tobytes() == b.tobytes() and a.tobytes() == c.tobytes()


def test_gpu_query_color_high_valence_vertex_is_summed_in_order():
    """a fan of 1,500 triangles around one vertex, hidden behind a cap: the apex normal is the S1 sum, bit for bit.  The cap's
    triangles are large (80 x 80 pixels): they take the deferred-face path of the rasteriser."""
    from icon_amd.recon import query_color_device
    v, f = cc.fan()
    assert (f == 0).sum() >= 1000
    image = cc.make_image()
    colors, vis = query_color_device(_dev(v), _dev(f), image.cuda(), return_vis=True)
    got = _compare("fan", v, f, image, colors, vis)
    assert vis[0].item() == 0
    want = ((torch.from_numpy(orc.vertex_normals(v, f)) + 1.0) * 0.5 * 255.0).numpy()
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1:1501], want[1:1501])


@pytest.mark.parametrize("n", [31, 32, 33, 64, 65])
def test_gpu_query_color_apex_valence_around_the_short_and_long_list_switch(n):
    """the fan with an apex of valence n (hidden behind the cap at each of these sizes, by the checker): 32 entries are the longest
    list one thread sums, 33 the shortest a wavefront rank-sorts; 64 fill the wavefront's one round of adding, 65 start a second.
    Apex and rim equal the S1 normals' colours byte for byte, for int64 and int32 faces; the rest as the checker has it."""
    from icon_amd.recon import query_color_device
    v, f = cc.fan(n)
    assert (f == 0).sum() == n and (f[:n, 0] == 0).all()
    image = cc.make_image()
    want, want_vis = cc.checker_query_color(v, f, image)
    assert not want_vis[:n + 1].any() and want_vis.any()                    # apex and rim hidden, the cap's vertices sampled
    colors, vis = query_color_device(_dev(v), _dev(f), image.cuda(), return_vis=True)
    c32 = query_color_device(_dev(v), _dev(f, torch.int32), image.cuda())
    got = colors.cpu().numpy()
    assert np.array_equal(vis.cpu().numpy(), want_vis)
    normal = ((torch.from_numpy(orc.vertex_normals(v, f)) + 1.0) * 0.5 * 255.0).numpy()
    assert np.array_equal(got[0], normal[0]), (got[0], normal[0])
    assert np.array_equal(got[1:n + 1], normal[1:n + 1])
    assert got.tobytes() == c32.cpu().numpy().tobytes()
    hidden = want_vis == 0
    assert np.array_equal(got[hidden], want.numpy()[hidden])
    d = float(np.abs(got[~hidden].astype(np.float64) - want.numpy()[~hidden]).max())
    print(f"fan({n}): sampled branch max |device - checker| = {d:.3e} (bar {cc.SAMPLED_GPU_BAR:.2e})")
    assert d <= cc.SAMPLED_GPU_BAR


def test_gpu_query_color_raster_mappings_agree():
    """the A/B switch of tools/time_query_color.py: 8 lanes per face (the default) and one wavefront per face give the same bytes (the z-buffer key does not depend
    on who rasterises a face)"""
    from icon_amd import _lib
    from icon_amd.recon import query_color_device
    v, f = cc.body()
    img_d = cc.make_image().cuda()
    outs = []
    try:
        for lanes in (0, 64):
            assert _lib.lib().icon_debug_set_option(b"qc_lanes", C.c_int(lanes)) == 0
            col, vis = query_color_device(_dev(v), _dev(f), img_d, return_vis=True)
            outs.append(col.cpu().numpy().tobytes() + vis.cpu().numpy().tobytes())
    finally:
        _lib.lib().icon_debug_set_option(b"qc_lanes", C.c_int(0))
    assert all(o == outs[0] for o in outs)


def test_gpu_query_color_raw_entry_skips_bad_faces_and_refuses_small_scratch():
    """the C entry itself (no Python check in the way), as test_gpu_visibility_reference_call_pattern_and_errors does for
    icon_visibility: a face that names a vertex that does not exist is skipped - no memory fault, every vertex as without it -
    and counted in the first word of the scratch; a scratch that is too small is an error code, nothing runs"""
    from icon_amd import _lib
    from icon_amd.engine import _stream
    from icon_amd.recon import IconAmdError, query_color
    v, f = cc.body()
    image = cc.make_image()
    fb = np.concatenate([f[:100], np.array([[0, 1, len(v) + 7]], np.int64), f[100:5000], np.array([[-1, 2, 3]], np.int64), f[5000:]])
    vd, fd, img = _dev(v), _dev(fb), image.cuda().contiguous()
    L = _lib.lib()
    n = C.c_int64(0)
    assert L.icon_query_color_bytes(C.c_int64(len(v)), C.c_int64(len(fb)), C.c_int(4096), C.byref(n)) == 0
    scratch = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    colors = torch.empty((len(v), 3), device="cuda")
    vis = torch.empty(len(v), device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    args = lambda nbytes: (p(vd), C.c_int64(len(v)), p(fd), C.c_int64(len(fb)), C.c_int(1), p(img), C.c_int(img.shape[2]), C.c_int(img.shape[3]),
                           C.c_int(4096), p(colors), p(vis), p(scratch), C.c_int64(nbytes), _stream())
    assert L.icon_query_color(*args(n.value - 1)) == 1 and b"scratch" in L.icon_last_error()
    assert L.icon_query_color(*args(n.value)) == 0
    torch.cuda.synchronize()
    assert int(scratch[:4].view(torch.int32).item()) == 2
    _compare("body with two bad faces", v, f, image, colors, vis)
    # the Python entry: device faces are not read back before the launch; the host-returning call reports what the kernels counted
    with pytest.raises(IconAmdError, match="out of range"):
        query_color(vd, fd, img)


def test_example_writes_the_colours_query_color_gives(tmp_path):
    """examples/dense_recon.py --color: the r g b columns of the OBJ are query_color's answer on the example's own mesh (rebuilt
    here with the same deterministic pipeline), to the six decimals the file carries"""
    import os
    import subprocess
    import sys
    from types import SimpleNamespace
    from common import ROOT
    from icon_amd import synth
    from icon_amd.engine import query_func
    from icon_amd.recon import DenseReconEngine, clean_mesh, query_color
    from test_gpu_parity import make_engine, T
    out = tmp_path / "body.obj"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dense_recon.py"), "--res", "65", "--color", "--out", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "query_color" in r.stdout
    rows = [l.split() for l in open(out) if l.startswith("v ")]
    assert rows and all(len(x) == 7 for x in rows)
    file_v = np.array([[float(t) for t in x[1:4]] for x in rows])
    file_c = np.array([[float(t) for t in x[4:]] for x in rows])
    a = assets("body")
    eng = make_engine(a)
    recon = DenseReconEngine(query_func=query_func, b_min=[[-1.0, 1.0, -1.0]], b_max=[[1.0, -1.0, 1.0]], resolutions=[65], align_corners=True,
                             balance_value=0.5, faster=True).cuda()
    occ = recon(opt=SimpleNamespace(num_views=1), netG=eng, features=[T(a.features)], proj_matrix=None)
    v, f = clean_mesh(*recon.export_mesh(occ))
    v = (v.float() - 32.0) / 32.0
    assert len(v) == len(rows) and np.abs(file_v - v.numpy()).max() <= 1e-6
    image = torch.from_numpy(np.tanh(synth.make_feature_planes(3, 512, 531)).astype(np.float32))
    want = query_color(v, f, image).numpy() / 255.0
    assert np.abs(file_c - want).max() <= 1e-6 and file_c.min() >= 0.0 and file_c.max() <= 1.0

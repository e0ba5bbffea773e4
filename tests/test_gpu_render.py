"""icon_render_normal / icon_amd.render on the device against the float32 statement of the rule (tests/render_checker.py
render_f32, itself held against pytorch3d's pipeline in float64 by tests/test_render.py): face ids equal on every pixel, depths
and colours bit-equal, for every mesh, size and camera set of render_checker.CASES; index types, lane mappings, bad faces,
streams, graph replay and the Render class."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_checker as rc

pytestmark = pytest.mark.gpu


def _dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dtype is None else t.to(dtype)


def _render(v, f, cams, S, dtype=torch.int64):
    from icon_amd.render import render_normal_device
    img, dep, pix = render_normal_device(_dev(v), _dev(f, dtype), cams, S, return_depth=True, return_faces=True)
    return pix.cpu().numpy(), dep.cpu().numpy(), img.cpu().numpy()


def _set_lanes(n):
    from icon_amd import _lib
    assert _lib.lib().icon_debug_set_option(b"rn_lanes", C.c_int(n)) == 0


@pytest.mark.parametrize("name", list(rc.CASES))
def test_gpu_render_equals_the_float32_rule(name):
    v, f, S, cams, (pix, depth, image) = rc.case(name)
    got = _render(v, f, cams, S)
    print(f"{name}: {int((got[0] != pix).sum())} pixels with another face, max |depth| diff {np.abs(got[1] - depth).max():.3e}, "
          f"max |colour| diff {np.abs(got[2] - image).max():.3e}, covered {int((pix >= 0).sum())}")
    assert got[0].dtype == np.int32 and got[0].shape == (len(cams), S, S) and got[2].shape == (len(cams), 3, S, S)
    assert np.array_equal(got[0], pix)
    assert got[1].tobytes() == depth.tobytes()
    assert got[2].tobytes() == image.tobytes()
    assert np.abs(got[2]).max() <= 1.0 + 4 * 2.0 ** -23           # b0 + b1 + b2 and |n| are 1 to within their float32 rounding
    # int32 faces and the other lane mappings: the same bytes
    g32 = _render(v, f, cams, S, torch.int32)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, g32))
    try:
        for lanes in (1, 8):
            _set_lanes(lanes)
            alt = _render(v, f, cams, S)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, alt)), lanes
    finally:
        _set_lanes(0)


@pytest.mark.parametrize("n", [31, 32, 33, 64, 65])
def test_gpu_render_apex_valence_around_the_short_and_long_list_switch(n):
    """the fan with an apex of valence n: 32 entries are the longest list one thread sums, 33 the shortest a wavefront rank-sorts;
    64 fill the wavefront's one round of adding, 65 start a second.  Front and back view (the back view looks at the fan: the
    apex normal colours its faces) against the float32 rule, for equality"""
    import color_checker as cc
    v, f = cc.fan(n)
    assert (f == 0).sum() == n
    pix, depth, image = rc.render_f32(v, f, (0, 2), 64)
    got = _render(v, f, (0, 2), 64)
    assert (pix[1] >= 0).any() and (pix[1][pix[1] >= 0] < n).any()          # the back view shows fan faces
    assert np.array_equal(got[0], pix)
    assert got[1].tobytes() == depth.tobytes()
    assert got[2].tobytes() == image.tobytes()


def test_gpu_render_skips_and_counts_bad_faces():
    """the C entry itself: the face naming vertex V is skipped and counted in the first word of the scratch; the result is the
    icosphere's, rendered without the three extra faces"""
    from icon_amd import _lib
    from icon_amd.engine import _stream
    v, f, S, cams, _ = rc.case("bad")
    want = rc.case("ico")
    vd, fd = _dev(v), _dev(f)
    L = _lib.lib()
    n = C.c_int64(0)
    assert L.icon_render_bytes(C.c_int64(len(v)), C.c_int64(len(f)), C.c_int(S), C.c_int(2), C.byref(n)) == 0
    scratch = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    img = torch.empty((2, 3, S, S), device="cuda")
    dep = torch.empty((2, S, S), device="cuda")
    pix = torch.empty((2, S, S), dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    args = lambda nbytes: (p(vd), C.c_int64(len(v)), p(fd), C.c_int64(len(f)), C.c_int(1), (C.c_int * 2)(*cams), C.c_int(2), C.c_int(S),
                           p(img), p(dep), p(pix), p(scratch), C.c_int64(nbytes), _stream())
    assert L.icon_render_normal(*args(n.value - 1)) == 1 and b"scratch" in L.icon_last_error()
    assert L.icon_render_normal(*args(n.value)) == 0
    torch.cuda.synchronize()
    assert int(scratch[:4].view(torch.int32).item()) == 1
    ref = _render(want[0], want[1], cams, S)
    assert np.array_equal(pix.cpu().numpy(), ref[0]) and dep.cpu().numpy().tobytes() == ref[1].tobytes()
    assert img.cpu().numpy().tobytes() == ref[2].tobytes()
    # depth and face planes are optional
    a = list(args(n.value))
    a[9], a[10] = None, None
    img2 = torch.empty_like(img)
    a[8] = p(img2)
    assert L.icon_render_normal(*a) == 0
    assert torch.equal(img, img2)


def test_gpu_render_two_streams_do_not_disturb_each_other():
    from icon_amd.render import render_normal_device
    va, fa, Sa, ca, wa = rc.case("body")
    vb, fb, Sb, cb, wb = rc.case("fan")
    a_in, b_in = (_dev(va), _dev(fa)), (_dev(vb), _dev(fb))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs_a, outs_b = [], []
    for _ in range(3):
        with torch.cuda.stream(s1):
            outs_a.append(render_normal_device(*a_in, ca, Sa, return_depth=True, return_faces=True))
        with torch.cuda.stream(s2):
            outs_b.append(render_normal_device(*b_in, cb, Sb, return_depth=True, return_faces=True))
    torch.cuda.synchronize()
    for outs, want in ((outs_a, wa), (outs_b, wb)):
        for img, dep, pix in outs:
            assert np.array_equal(pix.cpu().numpy(), want[0]) and dep.cpu().numpy().tobytes() == want[1].tobytes()
            assert img.cpu().numpy().tobytes() == want[2].tobytes()


def test_gpu_render_replays_from_a_captured_graph():
    """single stream, no parallel branches: the call allocates nothing and waits for nothing, so it can be captured"""
    from icon_amd.render import render_normal_device
    v, f, S, cams, want = rc.case("ico")
    vd, fd = _dev(v), _dev(f)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        render_normal_device(vd, fd, cams, S, return_depth=True, return_faces=True)          # warm-up: scratch of this stream
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        img, dep, pix = render_normal_device(vd, fd, cams, S, return_depth=True, return_faces=True)
    for _ in range(2):
        img.zero_(); dep.zero_(); pix.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(pix.cpu().numpy(), want[0]) and dep.cpu().numpy().tobytes() == want[1].tobytes()
        assert img.cpu().numpy().tobytes() == want[2].tobytes()


def test_gpu_render_class_follows_the_reference_signatures():
    from icon_amd.render import Render, render_normal_device
    v, f, S, cams, want = rc.case("body")
    r = Render(size=S, device=torch.device("cuda:0"))
    r.load_meshes(v, f)                                                   # host arrays
    two = r.get_rgb_image()
    assert len(two) == 2 and all(t.shape == (1, 3, S, S) and t.is_cuda and t.dtype == torch.float32 for t in two)
    assert two[0].cpu().numpy().tobytes() == want[2][0:1].tobytes() and two[1].cpu().numpy().tobytes() == want[2][1:2].tobytes()
    # ... which is the plain call of each camera alone, camera 2 mirrored
    vd, fd = _dev(v), _dev(f)
    front, back = render_normal_device(vd, fd, (0,), S), render_normal_device(vd, fd, (2,), S)
    assert torch.equal(two[0], front) and torch.equal(two[1], torch.flip(back, dims=[3]))
    dm = r.get_depth_map(cam_ids=[0, 2])
    assert len(dm) == 2 and dm[0].shape == (S, S)
    assert dm[0].cpu().numpy().tobytes() == want[1][0].tobytes() and dm[1].cpu().numpy().tobytes() == want[1][1].tobytes()
    assert float(dm[0].min()) == -1.0 and 99.0 < float(dm[0][dm[0] > 0].min()) < 101.0
    # four views: returned unmirrored, in camera order; a list of meshes keeps element 0; device tensors are taken as they are
    r.load_meshes([vd, vd[:3]], [fd, fd[:1] * 0 + torch.tensor([0, 1, 2], device="cuda")])
    four = r.get_rgb_image(cam_ids=[0, 1, 2, 3])
    assert len(four) == 4 and torch.equal(four[0], front) and torch.equal(four[2], back)
    assert not torch.equal(four[1], four[3])
    d4 = r.get_depth_map(cam_ids=[0, 1, 2, 3])
    _, dep4 = render_normal_device(vd, fd, (0, 1, 2, 3), S, return_depth=True)
    assert torch.equal(d4[0], dep4[0]) and torch.equal(d4[1], dep4[1]) and torch.equal(d4[2], torch.fliplr(dep4[2]))


def test_gpu_render_of_a_cleaned_marching_cubes_mesh():
    """65^3 synthetic volume -> device marching cubes -> clean_mesh -> render at 128^2, all on the device, int32 faces as
    clean_mesh returns them: coverage (and the rest) equal to the float32 rule"""
    from common import assets
    from icon_amd.recon import clean_mesh, export_mesh_device
    from icon_amd.render import render_normal_device
    from test_gpu_parity import make_engine, T
    a = assets("body")
    occ = make_engine(a).eval_slab(T(a.features), 65, 0, 65)
    v, f = clean_mesh(*export_mesh_device(occ, 0.5))
    v = (v.float() - 32.0) / 32.0
    assert f.dtype == torch.int32 and f.is_cuda and len(f) > 3000
    img, dep, pix = render_normal_device(v, f, (0, 1, 2, 3), 128, return_depth=True, return_faces=True)
    wp, wd, wi = rc.render_f32(v.cpu().numpy(), f.cpu().numpy(), (0, 1, 2, 3), 128)
    got = pix.cpu().numpy()
    print(f"marching cubes 65^3: {len(v)} vertices, {len(f)} faces, covered {int((wp >= 0).sum())}, other face on {int((got != wp).sum())} pixels, "
          f"max |colour| diff {np.abs(img.cpu().numpy() - wi).max():.3e}")
    assert np.array_equal(got >= 0, wp >= 0) and (wp >= 0).sum() > 4000
    assert np.array_equal(got, wp) and dep.cpu().numpy().tobytes() == wd.tobytes() and img.cpu().numpy().tobytes() == wi.tobytes()

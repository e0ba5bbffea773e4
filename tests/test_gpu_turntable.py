"""icon_render_turntable / icon_amd.render on the device against the float32 statement of the rule (tests/turntable_checker.py
render_f32, itself held against pytorch3d's pipeline in float64 by tests/test_turntable.py): face ids, depths, colours and frame
bytes equal for every mesh and size of turntable_checker.CASES at its seven angles; index types, lane mappings, chunk boundaries,
the four fixed cameras, 360 views, the canvas, streams, graph replay and the Render class."""
import ctypes as C
import sys
import types

import numpy as np
import pytest
import torch

import render_checker as rc
import turntable_checker as tc

pytestmark = pytest.mark.gpu


def _dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dtype is None else t.to(dtype)


def _render(v, f, angles, S, dtype=torch.int64):
    """-> pix, depth, image, frames as numpy"""
    from icon_amd.render import render_turntable_device
    frames, img, dep, pix = render_turntable_device(_dev(v), _dev(f, dtype), angles, S, return_images=True, return_depth=True, return_faces=True)
    return pix.cpu().numpy(), dep.cpu().numpy(), img.cpu().numpy(), frames.cpu().numpy()


def _same(got, want):
    return all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, want))


def _option(key, n):
    from icon_amd import _lib
    assert _lib.lib().icon_debug_set_option(key, C.c_int(n)) == 0


@pytest.mark.parametrize("name", list(tc.CASES))
def test_gpu_turntable_equals_the_float32_rule(name):
    v, f, S, want = tc.case(name)
    n = len(tc.ANGLES)
    got = _render(v, f, tc.ANGLES, S)
    print(f"{name}: {int((got[0] != want[0]).sum())} pixels with another face, max |depth| diff {np.abs(got[1] - want[1]).max():.3e}, "
          f"max |colour| diff {np.abs(got[2] - want[2]).max():.3e}, {int((got[3] != want[3]).sum())} other bytes, covered {int((want[0] >= 0).sum())}")
    assert got[0].dtype == np.int32 and got[0].shape == (n, S, S) and got[2].shape == (n, 3, S, S)
    assert got[3].dtype == np.uint8 and got[3].shape == (n, S, S, 3)
    assert np.array_equal(got[0], want[0])
    assert got[1].tobytes() == want[1].tobytes()
    assert got[2].tobytes() == want[2].tobytes()
    assert got[3].tobytes() == want[3].tobytes()
    # int32 faces, the other lane mappings and chunks of 2 and 3 views (the seven views then span several chunks): the same bytes
    assert _same(_render(v, f, tc.ANGLES, S, torch.int32), got)
    try:
        for lanes in (1, 8):
            _option(b"rn_lanes", lanes)
            for chunk in (2, 3):
                _option(b"tt_chunk", chunk)
                assert _same(_render(v, f, tc.ANGLES, S), got), (lanes, chunk)
    finally:
        _option(b"rn_lanes", 0)
        _option(b"tt_chunk", 0)


def test_gpu_turntable_at_quarter_turns_is_the_four_fixed_cameras():
    """an independent statement that needs no numpy rule: the float outputs at 90, 0, 270 and 180 degrees are
    render_normal_device's for cameras 0, 1, 2, 3, byte for byte"""
    from icon_amd.render import render_normal_device
    fn, S = tc.CASES["body"]
    v, f = fn()
    pix, dep, img, _ = _render(v, f, [90, 0, 270, 180], S)
    wi, wd, wp = render_normal_device(_dev(v), _dev(f), (0, 1, 2, 3), S, return_depth=True, return_faces=True)
    assert (wp >= 0).sum() > 4000
    assert _same((pix, dep, img), (wp.cpu().numpy(), wd.cpu().numpy(), wi.cpu().numpy()))


def test_gpu_turntable_360_views_and_every_chunk_size_of_one():
    v, f = tc.CASES["ico"][0]()
    S = 32
    from icon_amd.render import turntable_cos_sin
    want = tc.render_f32(v, f, turntable_cos_sin(range(360)), S)
    got = _render(v, f, range(360), S)
    assert _same(got, want)
    try:
        _option(b"tt_chunk", 1)
        assert _same(_render(v, f, range(360), S), got)
    finally:
        _option(b"tt_chunk", 0)


def test_gpu_turntable_writes_its_panel_of_the_canvas_and_nothing_else():
    """W = 3 S + 5, two meshes at x0 = 5 and 5 + S over sentinel bytes: a row of the canvas is 3 W = 591 bytes, so the panels' rows start
    at every residue of 4 and the lanes that store bytes and those that store dwords both meet every alignment"""
    from icon_amd.render import render_turntable_device, turntable_cos_sin
    S, angles = 64, [10, 200, 10, 123.5, 200]
    W = 3 * S + 5
    meshes = [tc.CASES["ico"][0](), tc.CASES["fan"][0]()]
    alone = [render_turntable_device(_dev(v), _dev(f), angles, S) for v, f in meshes]
    canvas = torch.full((len(angles), S, W, 3), 0xA5, dtype=torch.uint8, device="cuda")
    want = canvas.clone()
    for k, ((v, f), a) in enumerate(zip(meshes, alone)):
        x0 = 5 + k * S
        assert render_turntable_device(_dev(v), _dev(f), angles, S, out=canvas, x0=x0) is canvas
        want[:, :, x0:x0 + S] = a
    assert torch.equal(canvas, want)
    for (v, f), a in zip(meshes, alone):                                   # duplicated angles give duplicated frames
        assert torch.equal(a[0], a[2]) and torch.equal(a[1], a[4]) and not torch.equal(a[0], a[1])
        assert a.cpu().numpy().tobytes() == tc.render_f32(v, f, turntable_cos_sin(angles), S)[3].tobytes()
    # an odd size at the last possible column
    S = 63
    v, f = meshes[0]
    canvas = torch.full((2, S, S + 2, 3), 0xA5, dtype=torch.uint8, device="cuda")
    render_turntable_device(_dev(v), _dev(f), [37, 359], S, out=canvas, x0=2)
    assert (canvas[:, :, :2] == 0xA5).all() and torch.equal(canvas[:, :, 2:], render_turntable_device(_dev(v), _dev(f), [37, 359], S))


def test_gpu_turntable_two_streams_do_not_disturb_each_other():
    from icon_amd.render import render_turntable_device
    va, fa, Sa, wa = tc.case("body")
    vb, fb, Sb, wb = tc.case("fan")
    a_in, b_in = (_dev(va), _dev(fa)), (_dev(vb), _dev(fb))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs_a, outs_b = [], []
    for _ in range(3):
        with torch.cuda.stream(s1):
            outs_a.append(render_turntable_device(*a_in, tc.ANGLES, Sa, return_depth=True))
        with torch.cuda.stream(s2):
            outs_b.append(render_turntable_device(*b_in, tc.ANGLES, Sb, return_depth=True))
    torch.cuda.synchronize()
    for outs, want in ((outs_a, wa), (outs_b, wb)):
        for frames, dep in outs:
            assert frames.cpu().numpy().tobytes() == want[3].tobytes() and dep.cpu().numpy().tobytes() == want[1].tobytes()


def test_gpu_turntable_replays_from_a_captured_graph():
    """single stream, no parallel branches: after a warm-up (this stream's scratch and angle pairs) the call allocates nothing,
    copies nothing and waits for nothing - kernel nodes only.  Chunks of 3: the resolve pass's clears are replayed too"""
    from icon_amd.render import render_turntable_device
    v, f, S, want = tc.case("quads")
    vd, fd = _dev(v), _dev(f)
    try:
        _option(b"tt_chunk", 3)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            render_turntable_device(vd, fd, tc.ANGLES, S, return_faces=True)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            frames, pix = render_turntable_device(vd, fd, tc.ANGLES, S, return_faces=True)
        for _ in range(2):
            frames.zero_(); pix.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(pix.cpu().numpy(), want[0]) and frames.cpu().numpy().tobytes() == want[3].tobytes()
    finally:
        _option(b"tt_chunk", 0)


def test_gpu_turntable_bad_mesh_renders_as_ico():
    """the C entry's count of the faces it skipped, too: the first word of the scratch after the call"""
    from icon_amd._native import scratch
    v, f, S, _ = tc.case("bad")
    got = _render(v, f, tc.ANGLES, S)
    torch.cuda.synchronize()
    assert int(scratch(torch.device("cuda", torch.cuda.current_device()), 4)[:4].view(torch.int32).item()) == 1
    assert _same(got, tc.case("ico")[3])
    vi, fi = tc.CASES["ico"][0]()
    assert _same(got, _render(vi, fi, tc.ANGLES, S))


class _StubWriter:
    def __init__(self, path, fourcc, fps, size):
        self.path, self.fourcc, self.fps, self.size, self.frames, self.released = path, fourcc, fps, size, [], False

    def write(self, frame):
        assert not self.released
        self.frames.append(frame.copy())

    def release(self):
        self.released = True


def test_gpu_turntable_render_class_frames_and_video(monkeypatch):
    from PIL import Image
    from icon_amd.render import IconAmdError, Render, render_turntable_device
    S = 64
    angles = [0, 37, 90, 123.5, 200, 270, 359, 10, 20, 30, 40, 50]
    meshes = [tc.CASES["ico"][0](), tc.CASES["fan"][0]()]
    rng = np.random.RandomState(3)
    images = [rng.randint(0, 256, (100, 150, 3)).astype(np.uint8), rng.randint(0, 256, (80, 80, 3)).astype(np.uint8)]
    new_w = int(np.around(S / 100 * 150))
    r = Render(size=S, device=torch.device("cuda:0"))
    r.load_meshes([m[0] for m in meshes], [m[1] for m in meshes])
    before = [t.clone() for t in r.get_rgb_image(cam_ids=[0, 1, 2, 3])]
    chunks = list(r.get_rendered_frames(images, angles=angles, chunk=5))
    W = 2 * new_w + 2 * S
    assert [tuple(c.shape) for c in chunks] == [(5, S, W, 3), (5, S, W, 3), (2, S, W, 3)]
    assert all(c.is_cuda and c.dtype == torch.uint8 for c in chunks)
    frames = torch.cat(chunks)
    assert torch.equal(frames, next(r.get_rendered_frames(images, angles=angles, chunk=len(angles))))
    x = 0
    for img in images:                                                     # the image panels first, as the reference resizes them
        small = np.array(Image.fromarray(img).resize((new_w, S))).astype(np.uint8)[:, :, [2, 1, 0]]
        assert small.shape == (S, new_w, 3)
        assert (frames[:, :, x:x + new_w].cpu().numpy() == small[None]).all()
        x += new_w
    for v, f in meshes:                                                    # then one panel per mesh, in the order they were loaded
        assert torch.equal(frames[:, :, x:x + S], render_turntable_device(_dev(v), _dev(f), angles, S))
        x += S
    assert x == W
    # no images: the panels alone
    assert next(r.get_rendered_frames([], angles=[5.0])).shape == (1, S, 2 * S, 3)

    # the video: a recording stub in cv2's place (the real writer is not installed here)
    made = []
    stub = types.ModuleType("cv2")
    stub.VideoWriter_fourcc = lambda *c: "".join(c)
    stub.VideoWriter = lambda *a: made.append(_StubWriter(*a)) or made[-1]
    monkeypatch.setitem(sys.modules, "cv2", stub)
    r.get_rendered_video(images, "turntable.mp4")
    w, = made
    assert (w.path, w.fourcc, w.fps, w.size) == ("turntable.mp4", "mp4v", 30, (W, S)) and w.released
    assert len(w.frames) == 360 and all(fr.shape == (S, W, 3) and fr.dtype == np.uint8 for fr in w.frames)
    whole = [0, 37, 90, 200, 270, 359]
    assert all(np.array_equal(w.frames[a], frames[angles.index(a)].cpu().numpy()) for a in whole)
    monkeypatch.setitem(sys.modules, "cv2", None)                          # import cv2 now raises ImportError
    with pytest.raises(IconAmdError, match="get_rendered_frames"):
        r.get_rendered_video(images, "turntable.mp4")
    # the four cameras are left alone
    after = r.get_rgb_image(cam_ids=[0, 1, 2, 3])
    assert len(after) == 4 and all(torch.equal(a, b) for a, b in zip(before, after))

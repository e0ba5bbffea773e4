"""The turntable renderer (icon_amd.render.render_turntable_device / Render.get_rendered_frames) - CPU side.
The angle pairs; the float32 projection against pytorch3d's look-at camera and orthographic matrix in float64, and against the
four fixed cameras of 4.13; the float32 rule the device is compared with (turntable_checker.render_f32) against pytorch3d's
pipeline in float64 (render_checker.render_blend_f64 with the turntable's eyes); and the host contract of the Python and C entries
without a device.

f32 rule against the float64 blend at the seven angles of turntable_checker.ANGLES, measured on this suite's meshes:

    case      covered  only one covers  colour     depth      outliers colour / depth (> 4 x median of the maxima)
    ico         4833        0           2.23e-03   2.13e-05     0 / 0
    ico_odd     4677        0           1.46e-03   1.94e-05     0 / 0
    fan         3676        0           2.99e-01   1.83e-05     3 / 0
    quads       4641        0           2.60e-07   1.87e-05     0 / 0
    bad         4833        0           2.23e-03   2.13e-05     0 / 0
    body       13505        0           1.53e-02   1.97e-05     4 / 0

Every outlier lies within the blur radius of a projected edge (asserted).  The projection itself, on the body at the 360 whole
angles: X within 4.3e-8, Y equal, D within 7.7e-6 (one float32 ulp at 100) of the float64 camera.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import render_checker as rc
import turntable_checker as tc
from icon_amd import _lib
from icon_amd.render import IconAmdError, Render, render_turntable_device, turntable_cos_sin

CAP = 0.005            # the cap of test_render.py::test_f32_rule_against_the_float64_blend on both counts: 0.5 % of the covered pixels


def test_pairs_are_exact_at_quarter_turns_and_rounded_float64_elsewhere():
    exact = {0: (1, 0), 90: (0, 1), 180: (-1, 0), 270: (0, -1), -90: (0, -1), 450: (0, 1), 360: (1, 0), -180: (-1, 0), 720.0: (1, 0)}
    got = turntable_cos_sin(list(exact))
    assert got.dtype == np.float32 and got.shape == (len(exact), 2)
    assert got.tobytes() == np.array(list(exact.values()), np.float32).tobytes()              # no -0.0 either
    other = [37, 123.5, 200, 359, -12.25, 1000.5, 89.999]
    want = np.array([(np.cos(np.pi / 180 * a), np.sin(np.pi / 180 * a)) for a in other]).astype(np.float32)
    assert turntable_cos_sin(other).tobytes() == want.tobytes()
    assert turntable_cos_sin(np.arange(360)).shape == (360, 2) and turntable_cos_sin(range(3)).shape == (3, 2)
    assert turntable_cos_sin([]).shape == (0, 2)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(IconAmdError, match="finite"):
            turntable_cos_sin([0, bad])


def test_projection_equals_the_look_at_camera_and_the_four_fixed_ones():
    v, _ = rc.body()
    v = np.ascontiguousarray(v, np.float32)
    K = rc.ortho_matrix_f64()
    worst = np.zeros(3)
    for a, (c, s) in zip(range(360), turntable_cos_sin(range(360))):
        R, T = rc.look_at_f64(tc.eye_f64(a))
        view = v.astype(np.float64) @ R + T
        ndc = np.concatenate([view, np.ones((len(view), 1))], 1) @ K.T
        X, Y, D = tc.project_f32(v, c, s)
        worst = np.maximum(worst, [np.abs(X - ndc[:, 0]).max(), np.abs(Y - ndc[:, 1]).max(), np.abs(D - view[:, 2]).max()])
    print(f"360 whole angles on the body: max |X| {worst[0]:.2e}, |Y| {worst[1]:.2e}, |D| {worst[2]:.2e} off the float64 camera")
    assert worst[0] <= 1e-6 and worst[1] <= 1e-6
    assert worst[2] <= 1.6e-5                                                # two float32 ulps of a depth at 100
    for a, cam in ((0, 1), (90, 0), (180, 3), (270, 2)):
        (c, s), = turntable_cos_sin([a])
        X, Y, D = tc.project_f32(v, c, s)
        Xc, Yc, Dc = rc._view_f32(v, cam)
        assert X.tobytes() == Xc.tobytes() and D.tobytes() == Dc.tobytes() and Y.tobytes() == Yc.tobytes(), (a, cam)


def test_f32_rule_against_the_float64_blend(monkeypatch):
    """the conditions of test_render.py::test_f32_rule_against_the_float64_blend at the turntable's angles: pixels only one
    statement covers <= 0.5 % of the covered ones; colour / depth outliers (beyond 4 x the median over the meshes of the largest
    difference on the commonly covered pixels) <= 0.5 %, each within the blur radius of a projected edge by the float64 distance.
    The float64 side is render_blend_f64 itself, given the reference's eyes.  The module docstring has the measured table."""
    monkeypatch.setattr(rc, "CAM_EYES", list(rc.CAM_EYES) + [tc.eye_f64(a) for a in tc.ANGLES])
    cams = tuple(range(4, 4 + len(tc.ANGLES)))
    rows = {}
    for name in tc.CASES:
        v, f, S, (pix, depth, image, _) = tc.case(name)
        p64, d64, i64, e2 = rc.render_blend_f64(v, f, cams, S, flip=False)
        c32, c64 = pix >= 0, p64 >= 0
        both = c32 & c64
        dc = np.abs(image.astype(np.float64) - i64).max(1)
        dd = np.abs(depth.astype(np.float64) - d64)
        rows[name] = (int(c32.sum()), int((c32 != c64).sum()), both, dc, dd, e2)
    med_c = float(np.median([r[3][r[2]].max() for r in rows.values()]))
    med_d = float(np.median([r[4][r[2]].max() for r in rows.values()]))
    print(f"median of the per-mesh maxima: colour {med_c:.3e}, depth {med_d:.3e}")
    for name, (covered, mismatch, both, dc, dd, e2) in rows.items():
        out_c, out_d = both & (dc > 4 * med_c), both & (dd > 4 * med_d)
        print(f"{name:9s} covered {covered:5d}  only one covers {mismatch:3d}  colour {dc[both].max():.2e}  depth {dd[both].max():.2e}"
              f"  outliers colour {int(out_c.sum())} depth {int(out_d.sum())}")
        assert mismatch <= CAP * covered, name
        assert out_c.sum() <= CAP * covered and out_d.sum() <= CAP * covered, name
        assert (e2[out_c | out_d] < rc.BLUR).all(), name


def test_quads_fill_the_image_in_views_of_later_chunks():
    """the GPU tests rely on it: at 90, 123.5 and 270 degrees (view indices 2, 3, 5) quad A covers the whole 32 x 32 image - its
    triangles' pixel boxes go to the deferred lists, in chunks after the first when the chunk is 2 or 3 views"""
    _, _, S, (pix, _, _, frames) = tc.case("quads")
    assert S * S > 8 * 64
    for k in (2, 3, 5):
        assert (pix[k] >= 0).all() and set(np.unique(pix[k])) >= {0, 1}, k
    assert (frames[0][pix[0] < 0] == 127).all()


def test_bad_faces_render_as_the_mesh_without_them():
    a, b = tc.case("bad"), tc.case("ico")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[3], b[3]))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device behaviour")
def test_turntable_fails_loudly_without_device():
    v, f = (torch.from_numpy(x) for x in rc.quads())
    with pytest.raises(IconAmdError, match="no CPU fallback"):
        render_turntable_device(v, f, [0, 90], 32)
    r = Render(size=32)
    with pytest.raises(IconAmdError, match="no CPU fallback"):
        next(r.get_rendered_frames([], angles=[0, 1]))


def test_turntable_bad_arguments_raise():
    v, f = (torch.from_numpy(x) for x in rc.quads())
    S = 32
    canvas = lambda n=2, h=S, w=2 * S, c=3, dtype=torch.uint8: torch.zeros((n, h, w, c), dtype=dtype)
    with pytest.raises(IconAmdError, match="uint8"):
        render_turntable_device(v, f, [0, 90], S, out=canvas(dtype=torch.float32))
    for bad in (canvas(n=3), canvas(h=S + 1), canvas(c=4), canvas()[:, :, ::2], canvas()[0]):
        with pytest.raises(IconAmdError, match="canvas"):
            render_turntable_device(v, f, [0, 90], S, out=bad)
    with pytest.raises(IconAmdError, match="canvas"):
        render_turntable_device(v, f, [0, 90], S, out=canvas(w=S - 1))                        # narrower than a panel
    for x0 in (-1, S + 1, 0.5):
        with pytest.raises(IconAmdError, match="x0"):
            render_turntable_device(v, f, [0, 90], S, out=canvas(), x0=x0)
    with pytest.raises(IconAmdError, match="x0"):
        render_turntable_device(v, f, [0, 90], S, x0=1)
    with pytest.raises(IconAmdError, match="angles"):
        render_turntable_device(v, f, [], S)
    with pytest.raises(IconAmdError, match="angles"):
        render_turntable_device(v, f, range(1025), S)
    with pytest.raises(IconAmdError, match="finite"):
        render_turntable_device(v, f, [float("nan")], S)
    with pytest.raises(IconAmdError, match="size"):
        render_turntable_device(v, f, [0], 4)
    with pytest.raises(IconAmdError, match="verts"):
        render_turntable_device(v[:, :2], f, [0], S)
    with pytest.raises(IconAmdError, match="faces"):
        render_turntable_device(v, f.float(), [0], S)


def test_library_binds_the_turntable_symbols():
    assert "icon_render_turntable_bytes" in _lib.SYMBOLS and "icon_render_turntable" in _lib.SYMBOLS
    lib = _lib.lib()
    assert lib.icon_render_turntable_bytes.restype is C.c_int and lib.icon_render_turntable.restype is C.c_int
    assert lib.icon_version() == 100


def test_native_turntable_entries_refuse_bad_arguments_with_messages():
    lib = _lib.lib()
    V, F, S = 6890, 13776, 512
    nbytes = lambda n, S=S, V=V, F=F: (lambda b: (lib.icon_render_turntable_bytes(C.c_int64(V), C.c_int64(F), C.c_int(S), C.c_int(n), C.byref(b)), b.value))(C.c_int64(0))
    try:
        # the scratch holds one chunk's z-buffers: it grows up to the default chunk and not beyond it
        sizes = [nbytes(n) for n in range(1, 34)]
        assert all(rc_ == 0 for rc_, _ in sizes)
        grow = [b for _, b in sizes]
        chunk = next(n for n in range(1, 33) if grow[n] == grow[n - 1])                      # n views need what n + 1 need
        assert 1 <= chunk <= 32 and all(grow[n] > grow[n - 1] for n in range(1, chunk)) and all(b == grow[chunk - 1] for b in grow[chunk:])
        assert nbytes(360) == (0, grow[chunk - 1]) and nbytes(1024) == (0, grow[chunk - 1])
        assert grow[chunk - 1] >= chunk * S * S * 8 + F * 12 + V * 12                          # z-buffers, incidence list, normals at least
        # "tt_chunk" moves the boundary
        assert lib.icon_debug_set_option(b"tt_chunk", C.c_int(3)) == 0
        assert nbytes(2)[1] < nbytes(3)[1] == nbytes(4)[1] == nbytes(360)[1]
        for bad in (-1, 33):
            assert lib.icon_debug_set_option(b"tt_chunk", C.c_int(bad)) == 1 and b"tt_chunk" in lib.icon_last_error()
    finally:
        assert lib.icon_debug_set_option(b"tt_chunk", C.c_int(0)) == 0
    assert nbytes(0)[0] == 1 and b"n_views" in lib.icon_last_error()
    assert nbytes(1025)[0] == 1 and b"n_views" in lib.icon_last_error()
    assert nbytes(4, S=7)[0] == 1 and b"size" in lib.icon_last_error()
    assert nbytes(4, S=2049)[0] == 1 and b"size" in lib.icon_last_error()
    assert nbytes(4, V=0)[0] == 1 and b"V" in lib.icon_last_error()
    assert nbytes(4, F=1 << 29)[0] == 1 and b"F" in lib.icon_last_error()
    assert lib.icon_render_turntable_bytes(C.c_int64(10), C.c_int64(10), C.c_int(64), C.c_int(2), None) == 1 and b"null" in lib.icon_last_error()
    # host buffers are enough to reach the remaining checks: nothing is launched before they pass
    buf = np.zeros(4096, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 256
    p = C.c_void_p(base)

    def call(verts=p, cos_sin=p, n=2, size=64, canvas=p, width=64, x0=0, images=None, scratch=p, scratch_bytes=0):
        return lib.icon_render_turntable(verts, C.c_int64(3), p, C.c_int64(1), C.c_int(1), cos_sin, C.c_int(n), C.c_int(size),
                                         canvas, C.c_int64(width), C.c_int64(x0), images, None, None, scratch, C.c_int64(scratch_bytes), None)
    assert call(verts=None) == 1 and b"null" in lib.icon_last_error()
    assert call(cos_sin=None) == 1 and b"null" in lib.icon_last_error()
    assert call(scratch=None) == 1 and b"null" in lib.icon_last_error()
    assert call(canvas=None) == 1 and b"null" in lib.icon_last_error()                     # neither a canvas nor float planes
    assert call(size=4) == 1 and b"size" in lib.icon_last_error()
    assert call(n=0) == 1 and b"n_views" in lib.icon_last_error()
    assert call(n=1025) == 1 and b"n_views" in lib.icon_last_error()
    assert call(x0=-1) == 1 and b"x0" in lib.icon_last_error()
    assert call(x0=1) == 1 and b"x0" in lib.icon_last_error()                              # 1 + 64 > 64
    assert call(width=63) == 1 and b"x0" in lib.icon_last_error()
    assert call(width=70, x0=6, scratch=C.c_void_p(base + 4), scratch_bytes=1 << 30) == 1 and b"aligned" in lib.icon_last_error()
    assert call(width=70, x0=6, scratch_bytes=16) == 1 and b"scratch" in lib.icon_last_error()
    assert call(canvas=None, images=p, x0=-5, scratch_bytes=16) == 1 and b"scratch" in lib.icon_last_error()   # no canvas: x0 is not looked at

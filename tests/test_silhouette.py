"""The soft silhouette (icon_amd.render.silhouette_device) - CPU side: the constants and views of the oracle
(tests/silhouette_oracle.py) against the look-at camera, its gradient against central differences, the exclusion caps, the gaps
the GPU bars are taken from, the truncation report, the mirroring of Render.get_silhouette_image and the host contract."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_checker as rc
import silhouette_oracle as so
from icon_amd import _lib


def test_constants_and_views_equal_the_look_at_camera():
    assert so.SIGMA == 1e-4 and abs(so.BLUR_SIL - 4.60512e-4) < 1e-9
    assert so.BLUR_SIL == np.log(1.0 / 1e-4 - 1.0) * 5e-5
    # what a pair at the blur radius weighs - the most that one flipped pair moves alpha by: 0.0099 < EXCLUDED_BAR
    assert abs(1.0 / (1.0 + np.exp(so.BLUR_SIL / so.SIGMA)) - 0.0099) < 2e-6 and so.EXCLUDED_BAR == 0.0102
    src = open(_lib.CSRC + "/silhouette.hip").read()
    assert f"kSilBlur = {np.float32(so.BLUR_SIL):.9e}f" in src
    assert f"kSilBlurR = {np.sqrt(np.float32(so.BLUR_SIL)):.9e}f" in src
    # DESIGN.md 4.13's table: NDC X = -x, +z, +x, -z and depth 100 -+ coordinate, from the look-at camera and the projection matrix
    p = torch.tensor([[0.3, -0.2, 0.45]], dtype=torch.float64)
    want = {0: (-0.3, 100 - 0.45), 1: (0.45, 100 - 0.3), 2: (0.3, 100 + 0.45), 3: (-0.45, 100 + 0.3)}
    for cam, (x, d) in want.items():
        X, Y, D = so.project(p, cam, torch.float64)
        assert abs(float(X) - x) < 1e-12 and abs(float(Y) + 0.2) < 1e-12 and abs(float(D) - d) < 1e-12


def test_oracle_gradient_equals_central_differences():
    """ico at 16^2, all four cameras, float64: d sum(alpha grad_alpha) / d verts by autograd against central differences along
    six random directions.  Exclusion pixels are zero-weighted.  Step 1e-6: alpha changes by up to |x| / sigma per unit of
    squared distance, its second derivative is ~1 / sigma^2 = 1e8 of that, so the truncation error of a central difference is
    ~1e8 h^2 = 1e-4 relative at h = 1e-6, and rounding (1e-16 / h = 1e-10) is far below it; a pair changing its candidate status
    between the two evaluations would show as a jump ~1e-4 / h - none does at this size (the check would fail)."""
    v, f = so.CASES["ico"][0]()
    S, cams = 16, (0, 1, 2, 3)
    first = so.silhouette(v, f, cams, S, grad_alpha=so.smooth_field(4, S), zero_excluded=True)
    ga = so.smooth_field(4, S) * ~(first["excl_blur"] | first["excl_area"])
    g = first["grad_verts"]
    assert np.abs(g).max() > 1.0
    rs = np.random.RandomState(5)
    h = 1e-6
    for _ in range(6):
        u = rs.normal(size=v.shape)
        u /= np.linalg.norm(u)
        hi = (so.silhouette(v.astype(np.float64) + h * u, f, cams, S)["alpha"] * ga).sum()
        lo = (so.silhouette(v.astype(np.float64) - h * u, f, cams, S)["alpha"] * ga).sum()
        fd, an = (hi - lo) / (2 * h), float((g * u).sum())
        print(f"central difference {fd:.8e}, autograd {an:.8e}")
        assert abs(fd - an) <= 1e-3 * np.abs(g).max() / np.sqrt(g.size) + 1e-3 * abs(an)


def test_exclusion_caps_hold_and_excluded_pixels_agree():
    for name in so.CASES:
        c = so.case(name)
        ex, a64, a32 = c["excluded"], c["f64"]["alpha"], c["f32"]["alpha"]
        covered = int((a64 > 0).sum())
        print(f"{name:11s} alpha > 0 on {covered:6d}, excluded {int(ex.sum()):4d} ({100.0 * ex.sum() / covered:.3f} %): near the blur radius "
              f"{int(c['f64']['excl_blur'].sum())}, near-zero area {int(c['f64']['excl_area'].sum())}; most candidates on a pixel {int(c['f64']['count'].max())}")
        assert ex.sum() <= so.EXCLUDED_CAP * covered, name
        assert not ex.any() or np.abs(a32 - a64)[ex].max() <= so.EXCLUDED_BAR, name
        assert (c["grad_alpha"][ex] == 0).all()


def test_gaps_are_the_recorded_ones():
    """GAP_FWD / GAP_BWD of tests/test_gpu_silhouette.py are what the float32 run of the oracle differs from its float64 run by,
    measured here again.  The constants are the measured values to three digits: they may lie at most 3 % above what is measured
here, so that the device bars stay at 4 x gap (a constant BELOW the measurement - another CPU's float32 kernels may round
otherwise - only tightens the bars; 20 % below, the record is stale)"""
    import test_gpu_silhouette as tg
    gap_fwd = gap_bwd = 0.0
    for name in so.CASES:
        c = so.case(name)
        d = float(np.abs(c["f32"]["alpha"] - c["f64"]["alpha"])[~c["excluded"]].max())
        e = float(np.abs(c["f32"]["grad_verts"] - c["f64"]["grad_verts"]).max() / np.abs(c["f64"]["grad_verts"]).max())
        print(f"{name:11s} float32 oracle against float64: alpha {d:.3e}, gradient {e:.3e}")
        gap_fwd, gap_bwd = max(gap_fwd, d), max(gap_bwd, e)
    print(f"gap_fwd {gap_fwd:.3e}, gap_bwd {gap_bwd:.3e}")
    assert 0.8 * gap_fwd <= tg.GAP_FWD <= 1.03 * gap_fwd
    assert 0.8 * gap_bwd <= tg.GAP_BWD <= 1.03 * gap_bwd


def test_sliver_case_culls_its_back_face_for_every_camera():
    fn, S, cams = so.CASES["sliver"]
    v, f = fn()
    for cam in cams:
        X, Y, _ = (a.numpy() for a in so.project(torch.tensor(v, dtype=torch.float64), cam, torch.float64))
        area = so._ef(X[f[:, 2]], Y[f[:, 2]], X[f[:, 0]], Y[f[:, 0]], X[f[:, 1]], Y[f[:, 1]])
        assert area[0] > 1e-3 and area[1] > 1e-3 and area[2] < -1e-3
        assert X[f[0]].max() + np.sqrt(so.BLUR_SIL) > 1.0 or Y[f[0]].max() + np.sqrt(so.BLUR_SIL) > 1.0      # the box leaves the image
    with_face, without = so.case("sliver")["f64"], so.silhouette(v, f[:2], cams, S)
    assert np.array_equal(with_face["alpha"], without["alpha"]) and with_face["count"].max() >= 1
    assert (so.case("sliver")["f64"]["grad_verts"][6:9] == 0).all()


def test_truncation_report_covers_the_body():
    over, diff, most = so.truncation_report("body")
    print(f"body at 128^2: {over} pixels with more than 50 candidates (most: {most}), largest |alpha_all - alpha_50| {diff:.3e}")
    assert most > 50 and over > 0 and 0.0 <= diff <= 1.0
    over_f, diff_f, most_f = so.truncation_report("fan")
    print(f"fan at 64^2: {over_f} pixels with more than 50 candidates (most: {most_f}), largest |alpha_all - alpha_50| {diff_f:.3e}")
    assert most_f > 500


def test_get_silhouette_image_mirrors_camera_2_only_for_two_views(monkeypatch):
    """through a stubbed native call that returns the oracle's arrays as the native call would (camera 2 mirrored when IT renders two views)"""
    from icon_amd import render
    fn, S, _ = so.CASES["ico_offset"]
    v, f = fn()
    plain = {cam: so.silhouette(v, f, (cam,), S)["alpha"][0] for cam in (0, 1, 2)}
    assert not np.array_equal(plain[2], plain[2][:, ::-1])

    def stub(verts, faces, cam_ids=(0, 2), size=512):
        out = [plain[c] if not (len(cam_ids) == 2 and c == 2) else plain[c][:, ::-1] for c in cam_ids]
        return torch.from_numpy(np.stack(out).copy())

    monkeypatch.setattr(render, "silhouette_device", stub)
    monkeypatch.setattr(render, "_need_device", lambda what: None)
    r = render.Render(size=S)
    r.meshes = [(torch.from_numpy(v), torch.from_numpy(f))]
    two = r.get_silhouette_image()
    assert len(two) == 2 and two[0].shape == (1, S, S)
    assert np.array_equal(two[0][0].numpy(), plain[0]) and np.array_equal(two[1][0].numpy(), plain[2][:, ::-1])
    swapped = r.get_silhouette_image(cam_ids=[2, 0])                       # ascending camera order
    assert np.array_equal(swapped[0][0].numpy(), plain[0]) and np.array_equal(swapped[1][0].numpy(), plain[2][:, ::-1])
    one = r.get_silhouette_image(cam_ids=[2])
    assert len(one) == 1 and np.array_equal(one[0][0].numpy(), plain[2])
    three = r.get_silhouette_image(cam_ids=[0, 1, 2])
    assert len(three) == 3 and np.array_equal(three[2][0].numpy(), plain[2]) and np.array_equal(three[1][0].numpy(), plain[1])
    dup = r.get_silhouette_image(cam_ids=[2, 2])                           # the reference decides by len(cam_ids)
    assert len(dup) == 1 and np.array_equal(dup[0][0].numpy(), plain[2][:, ::-1])
    assert render._mirror_cam2([0, 2], (0, 2)) is False and render._mirror_cam2([2, 2], (2,)) is True


def test_silhouette_entries_exist_and_raise():
    """fails on the parent: there is no silhouette_device and no Render.get_silhouette_image"""
    from icon_amd.render import IconAmdError, Render, silhouette_device
    v, f = (torch.from_numpy(x) for x in rc.quads())
    with pytest.raises(IconAmdError, match="cam_ids"):
        silhouette_device(v, f, (0, 4), 32)
    with pytest.raises(IconAmdError, match="cam_ids"):
        silhouette_device(v, f, (), 32)
    with pytest.raises(IconAmdError, match="size"):
        silhouette_device(v, f, (0,), 4)
    with pytest.raises(IconAmdError, match="size"):
        silhouette_device(v, f, (0,), 4096)
    with pytest.raises(IconAmdError, match="verts"):
        silhouette_device(v[:, :2], f, (0,), 32)
    with pytest.raises(IconAmdError, match="verts"):
        silhouette_device(v.long(), f, (0,), 32)
    with pytest.raises(IconAmdError, match="faces"):
        silhouette_device(v, f.float(), (0,), 32)
    with pytest.raises(IconAmdError, match="faces"):
        silhouette_device(v, f[:, :2], (0,), 32)
    with pytest.raises(IconAmdError, match="cam_ids"):
        Render(size=32).get_silhouette_image(cam_ids=[5])
    if not torch.cuda.is_available():
        with pytest.raises(IconAmdError, match="no CPU fallback"):
            silhouette_device(v, f, (0, 2), 32)
        with pytest.raises(IconAmdError, match="no CPU fallback"):
            Render(size=32).get_silhouette_image()
    else:
        with pytest.raises(IconAmdError, match="one HIP device"):
            silhouette_device(v, f, (0, 2), 32)
        with pytest.raises(IconAmdError, match="load_meshes"):
            Render(size=32).get_silhouette_image()


def test_native_silhouette_entries_refuse_bad_arguments_with_messages():
    for s in ("icon_silhouette_bytes", "icon_silhouette_forward", "icon_silhouette_backward"):
        assert s in _lib.SYMBOLS
    lib = _lib.lib()
    n, four = C.c_int64(0), C.c_int64(0)
    assert lib.icon_silhouette_bytes(C.c_int64(6890), C.c_int64(13776), C.c_int(512), C.c_int(2), C.byref(n)) == 0
    assert n.value >= 2 * 13776 * (48 + 8 + 24) + 13776 * 24 + 6890 * 16
    assert lib.icon_silhouette_bytes(C.c_int64(6890), C.c_int64(13776), C.c_int(512), C.c_int(4), C.byref(four)) == 0 and four.value > n.value
    assert lib.icon_silhouette_bytes(C.c_int64(0), C.c_int64(10), C.c_int(512), C.c_int(2), C.byref(n)) == 1 and b"V" in lib.icon_last_error()
    assert lib.icon_silhouette_bytes(C.c_int64(10), C.c_int64(10), C.c_int(7), C.c_int(2), C.byref(n)) == 1 and b"size" in lib.icon_last_error()
    assert lib.icon_silhouette_bytes(C.c_int64(10), C.c_int64(10), C.c_int(2049), C.c_int(2), C.byref(n)) == 1 and b"size" in lib.icon_last_error()
    assert lib.icon_silhouette_bytes(C.c_int64(10), C.c_int64(10), C.c_int(64), C.c_int(5), C.byref(n)) == 1 and b"n_views" in lib.icon_last_error()
    assert lib.icon_silhouette_bytes(C.c_int64(10), C.c_int64(10), C.c_int(64), C.c_int(2), None) == 1 and b"null" in lib.icon_last_error()
    # host buffers are enough to reach the checks: nothing is launched before they pass
    buf = np.zeros(4096, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 256
    p = C.c_void_p(base)
    cams, bad = (C.c_int * 2)(0, 2), (C.c_int * 2)(0, 4)
    fwd = lambda cam, size, scratch, nbytes, out=p: lib.icon_silhouette_forward(p, C.c_int64(3), p, C.c_int64(1), C.c_int(1), cam, C.c_int(2), C.c_int(size),
                                                                               out, scratch, C.c_int64(nbytes), None)
    bwd = lambda cam, size, scratch, nbytes, ga=p: lib.icon_silhouette_backward(p, C.c_int64(3), p, C.c_int64(1), C.c_int(1), cam, C.c_int(2), C.c_int(size),
                                                                                p, ga, p, scratch, C.c_int64(nbytes), None)
    for call in (fwd, bwd):
        assert call(bad, 64, p, 0) == 1 and b"cam_ids" in lib.icon_last_error()
        assert call(cams, 4, p, 0) == 1 and b"size" in lib.icon_last_error()
        assert call(cams, 64, C.c_void_p(base + 4), 1 << 30) == 1 and b"aligned" in lib.icon_last_error()
        assert call(cams, 64, p, 16) == 1 and b"scratch" in lib.icon_last_error()
        assert call(cams, 64, p, 1 << 30, None) == 1 and b"null" in lib.icon_last_error()

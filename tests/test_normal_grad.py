"""The gradient of the normal maps (icon_amd.render.render_normal_device(differentiable=True), Render(normal_grad=True);
DESIGN.md 4.15) - CPU side: the oracle (tests/normal_grad_oracle.py) against central differences, the exclusion caps, the gap the
GPU bar is taken from, the normalisation's |N| <= 1e-6 branch, the record of the difference from the full soft blend, and the
host contract of the two new native entries."""
import ctypes as C

import numpy as np
import pytest
import torch

import normal_grad_oracle as no
import render_checker as rc
from icon_amd import _lib


@pytest.mark.parametrize("cams", [(0, 2), (0, 1, 2, 3)])
def test_oracle_gradient_equals_central_differences(cams):
    """ico at 16^2 (faces under a pixel), float64: d sum(images grad_images) / d verts by autograd against central differences
    along six random directions, the winners held fixed.  The function is smooth between clamp flips (excluded pixels are
    zero-weighted); its third derivative is ~ (1 / face size)^3 ~ 1e4 of the first, so a central difference at h = 1e-6 is off by
    ~1e-8 relative, and by rounding ~1e-16 / h = 1e-10."""
    c = no.case("ico16")
    v, f, S = c["verts"], c["faces"], 16
    pix = rc.render_f32(v, f, cams, S)[0]
    gi = no.grad_field(len(cams), S) * ~no.excluded(v, f, pix, cams, S)[:, None]
    g = no.loss_and_grad(v, f, pix, cams, S, gi)[1]
    assert np.abs(g).max() > 1.0
    rs = np.random.RandomState(5)
    h = 1e-6
    for _ in range(6):
        u = rs.normal(size=v.shape)
        u /= np.linalg.norm(u)
        hi = no.loss_and_grad(v.astype(np.float64) + h * u, f, pix, cams, S, gi)[0]
        lo = no.loss_and_grad(v.astype(np.float64) - h * u, f, pix, cams, S, gi)[0]
        fd, an = (hi - lo) / (2 * h), float((g * u).sum())
        print(f"cameras {cams}: central difference {fd:.10e}, autograd {an:.10e}, difference / |g|inf {abs(fd - an) / np.abs(g).max():.2e}")
        assert abs(fd - an) <= 1e-7 * np.abs(g).max()


def test_exclusion_caps_hold():
    for name in no.CASES:
        c = no.case(name)
        ex = c["excluded"]
        print(f"{name:11s} covered {c['covered']:5d}, excluded {int(ex.sum()):3d} ({100.0 * ex.sum() / c['covered']:.2f} %)")
        assert c["covered"] > 0 and ex.sum() <= no.EXCLUDED_CAP * c["covered"], name
        assert not (ex & (c["pix"] < 0)).any()
        assert (c["grad_images"][np.broadcast_to(ex[:, None], c["grad_images"].shape)] == 0).all()
        assert np.isfinite(c["g64"]).all() and np.isfinite(c["g32"]).all()


def test_gaps_are_the_recorded_ones():
    """GAP_BWD of tests/test_gpu_normal_grad.py is what the float32 run of the oracle differs from its float64 run by, measured
    here again: the constant may lie at most 3 % above what is measured here (and not more than 20 % below: the record is stale then)"""
    import test_gpu_normal_grad as tg
    gap = 0.0
    for name in no.CASES:
        c = no.case(name)
        e = float(np.abs(c["g32"] - c["g64"]).max() / np.abs(c["g64"]).max())
        print(f"{name:11s} float32 oracle against float64: gradient {e:.3e}, |g|inf {np.abs(c['g64']).max():.3e}")
        gap = max(gap, e)
    print(f"gap_bwd {gap:.3e}")
    assert 0.8 * gap <= tg.GAP_BWD <= 1.03 * gap


def test_normalisation_branch_of_cancelling_normals_is_finite():
    """n = N / max(|N|, 1e-6) where |N| <= 1e-6: d (n . g) / d N is g 1e6 exactly - at N = 0 too, where a differentiated square
    root would give NaN.  Two faces over the same three vertices, wound in opposite senses, have N_v = 0 at every vertex: the
    colour is sum b - 1 = 0 on every covered pixel and the gradient is finite"""
    g = torch.tensor([[0.3, -0.2, 0.5], [1.0, 0.0, -1.0], [0.25, 0.5, 0.75], [2.0, -3.0, 0.5]], dtype=torch.float64)
    N = torch.tensor([[0.0, 0.0, 0.0], [3e-7, -4e-7, 0.0], [0.0, 0.0, 1e-6], [3.0, 0.0, 4.0]], dtype=torch.float64, requires_grad=True)
    n = no.normalise(N)
    got = torch.autograd.grad((n * g).sum(), N)[0]
    assert torch.isfinite(got).all() and torch.equal(got[:3], g[:3] * 1e6) and torch.equal(n[:3], N[:3].detach() * 1e6)
    unit = torch.tensor([0.6, 0.0, 0.8], dtype=torch.float64)
    assert torch.allclose(got[3], (g[3] - unit * (unit * g[3]).sum()) / 5.0, rtol=1e-14, atol=0)
    v = np.array([[-0.5, -0.4, 0.1], [0.6, -0.3, 0.2], [0.0, 0.7, 0.15]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 1]], np.int64)
    assert (no.normal_sums(torch.tensor(v, dtype=torch.float64), f) == 0).all()
    pix = rc.render_f32(v, f, (0,), 16)[0]
    assert (pix >= 0).sum() > 10
    for dtype in (torch.float64, torch.float32):
        loss, grad = no.loss_and_grad(v, f, pix, (0,), 16, no.grad_field(1, 16), dtype=dtype)
        assert np.isfinite(grad).all() and np.isfinite(loss)
    assert float(no.images(torch.tensor(v, dtype=torch.float64), f, pix, (0,), 16).abs().max()) < 1e-12


def test_blend_difference_record():
    """a RECORD, not a bar: how far the winner's gradient is from the gradient of the full float64 soft blend
    (gamma = 1e-8, 1e-10 background weight) on ico and quads at 32^2.  The pixels responsible are those where another candidate
    than the nearest holds any of the blend's weight: each lies within the blur radius of a projected edge (two faces that share
    the edge are both candidates there, at depths closer than gamma resolves); the difference that remains without them (the
    1e-10 background weight's) is printed next to it."""
    for name in ("ico", "quads"):
        d = no.blend_difference(name)
        tied = d["tied"]
        print(f"{name} at 32^2: ||g_blend - g_winner||inf / ||g_winner||inf = {d['rel']:.3e} from {int(tied.sum())} of {d['covered']} covered pixels "
              f"({d['excluded']} excluded); without them {d['rel_rest']:.3e}")
        assert (d["edge_d2"][tied] < rc.BLUR).all()
        assert np.isfinite(d["rel"]) and np.isfinite(d["rel_rest"]) and d["covered"] > 0


def test_normal_grad_entries_exist_and_raise():
    """fails on the parent: there is no `differentiable` keyword and no `normal_grad`"""
    from icon_amd.render import IconAmdError, Render, render_normal_device
    v, f = (torch.from_numpy(x) for x in rc.quads())
    with pytest.raises(IconAmdError, match="cam_ids"):
        render_normal_device(v, f, (0, 4), 32, differentiable=True)
    with pytest.raises(IconAmdError, match="size"):
        render_normal_device(v, f, (0,), 4, differentiable=True)
    with pytest.raises(IconAmdError, match="verts"):
        render_normal_device(v[:, :2], f, (0,), 32, differentiable=True)
    with pytest.raises(IconAmdError, match="floating-point"):
        render_normal_device(v.long(), f, (0,), 32, differentiable=True)
    with pytest.raises(IconAmdError, match="faces"):
        render_normal_device(v, f.float(), (0,), 32, differentiable=True)
    with pytest.raises(IconAmdError, match="faces"):
        render_normal_device(v, f[:, :2], (0,), 32, differentiable=True)
    with pytest.raises(IconAmdError, match="HIP device"):
        Render(size=32, device="cpu", normal_grad=True)
    r = Render(size=32, normal_grad=True)
    assert r.normal_grad is True and Render(size=32).normal_grad is False
    with pytest.raises(IconAmdError, match="cam_ids"):
        r.get_rgb_image(cam_ids=[5])
    if not torch.cuda.is_available():
        with pytest.raises(IconAmdError, match="no CPU fallback"):
            render_normal_device(v, f, (0, 2), 32, differentiable=True)
        with pytest.raises(IconAmdError, match="no CPU fallback"):
            r.get_rgb_image()
        with pytest.raises(IconAmdError, match="no CPU fallback"):
            r.load_meshes(v.requires_grad_(True), f)
    else:
        with pytest.raises(IconAmdError, match="one HIP device"):
            render_normal_device(v, f, (0, 2), 32, differentiable=True)
        with pytest.raises(IconAmdError, match="load_meshes"):
            r.get_rgb_image()


def test_native_normal_grad_entries_refuse_bad_arguments_with_messages():
    for s in ("icon_render_normal_backward_bytes", "icon_render_normal_backward"):
        assert s in _lib.SYMBOLS
    lib = _lib.lib()
    assert hasattr(lib, "icon_render_normal_backward_bytes") and hasattr(lib, "icon_render_normal_backward")
    n, four = C.c_int64(0), C.c_int64(0)
    size_of = lambda V, F, S, nv, out: lib.icon_render_normal_backward_bytes(C.c_int64(V), C.c_int64(F), C.c_int(S), C.c_int(nv), out)
    assert size_of(6890, 13776, 512, 2, C.byref(n)) == 0
    # per view 36 + 24 bytes per face of corner records and 4 of the deferred list; 36 per face of the face pass; 24 of incidence lists
    assert n.value >= 2 * 13776 * (36 + 24 + 4) + 13776 * (36 + 24) + 6890 * (16 + 24)
    assert size_of(6890, 13776, 512, 4, C.byref(four)) == 0 and four.value > n.value
    assert size_of(0, 10, 512, 2, C.byref(n)) == 1 and b"V" in lib.icon_last_error()
    assert size_of(10, 0, 512, 2, C.byref(n)) == 1 and b"F" in lib.icon_last_error()
    assert size_of(10, 1 << 29, 512, 2, C.byref(n)) == 1 and b"F" in lib.icon_last_error()
    assert size_of(10, 10, 7, 2, C.byref(n)) == 1 and b"size" in lib.icon_last_error()
    assert size_of(10, 10, 2049, 2, C.byref(n)) == 1 and b"size" in lib.icon_last_error()
    assert size_of(10, 10, 64, 0, C.byref(n)) == 1 and b"n_views" in lib.icon_last_error()
    assert size_of(10, 10, 64, 5, C.byref(n)) == 1 and b"n_views" in lib.icon_last_error()
    assert size_of(10, 10, 64, 2, None) == 1 and b"null" in lib.icon_last_error()
    # host buffers are enough to reach the checks: nothing is launched before they pass
    buf = np.zeros(4096, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 256
    p = C.c_void_p(base)
    cams, bad = (C.c_int * 2)(0, 2), (C.c_int * 2)(0, 4)
    call = lambda cam, size, scratch, nbytes, pix=p, gi=p: lib.icon_render_normal_backward(
        p, C.c_int64(3), p, C.c_int64(1), C.c_int(1), cam, C.c_int(2), C.c_int(size), pix, gi, p, scratch, C.c_int64(nbytes), None)
    assert call(bad, 64, p, 0) == 1 and b"cam_ids" in lib.icon_last_error()
    assert call(cams, 4, p, 0) == 1 and b"size" in lib.icon_last_error()
    assert call(cams, 64, C.c_void_p(base + 4), 1 << 30) == 1 and b"aligned" in lib.icon_last_error()
    assert call(cams, 64, p, 16) == 1 and b"scratch" in lib.icon_last_error()
    assert call(cams, 64, p, 1 << 30, None) == 1 and b"null" in lib.icon_last_error()
    assert call(cams, 64, p, 1 << 30, p, None) == 1 and b"null" in lib.icon_last_error()

"""icon_silhouette_forward / icon_silhouette_backward / icon_amd.render.silhouette_device on the device against the float64
statement of the rule (tests/silhouette_oracle.py): forward and backward parity on the eight cases, determinism,
index types, bad faces, the autograd plumbing of the Render class, graph replay and a descent.

The bars are taken from the ORACLE, never from the device: the same torch statement run in float32 on the CPU differs from its
float64 run by GAP_FWD / GAP_BWD (tests/test_silhouette.py::test_gaps_are_the_recorded_ones measures them again: the constants
below may not lie more than 3 % above what it measures); the device may differ by four times that - another exp, another reciprocal, another
product order, another summation order over a face's pixels."""
import ctypes as C

import numpy as np
import pytest
import torch

import silhouette_oracle as so

pytestmark = pytest.mark.gpu

# largest |oracle float32 - oracle float64| of alpha over the compared (non-excluded) pixels of the eight cases, and largest
# ||g32 - g64||inf / ||g64||inf of the float32 oracle's autograd gradient over them: silhouette_oracle.case() on the CPU, the
# measured values as test_gaps_are_the_recorded_ones prints them (ico_odd; body)
GAP_FWD = 3.51e-6
GAP_BWD = 1.40e-5
BAR_FWD = 4 * GAP_FWD
BAR_BWD = 4 * GAP_BWD


def _dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dtype is None else t.to(dtype)


def _forward(v, f, cams, S, dtype=torch.int64):
    from icon_amd.render import silhouette_device
    return silhouette_device(_dev(v), _dev(f, dtype), cams, S)


def _both(v, f, cams, S, grad_alpha, dtype=torch.int64):
    """-> alpha [n,S,S], grad_verts [V,3] as float32 numpy"""
    from icon_amd.render import silhouette_device
    vd = _dev(v).requires_grad_(True)
    alpha = silhouette_device(vd, _dev(f, dtype), cams, S)
    alpha.backward(_dev(grad_alpha, torch.float32))
    return alpha.detach().cpu().numpy(), vd.grad.cpu().numpy()


def _rel(g, ref):
    return float(np.abs(g - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name", list(so.CASES))
def test_gpu_silhouette_forward_and_backward_parity(name):
    c = so.case(name)
    v, f, S, cams, ex = c["verts"], c["faces"], c["S"], c["cams"], c["excluded"]
    a64, g64 = c["f64"]["alpha"], c["f64"]["grad_verts"]
    alpha, grad = _both(v, f, cams, S, c["grad_alpha"])
    assert alpha.shape == (len(cams), S, S) and alpha.dtype == np.float32 and grad.shape == v.shape
    d = np.abs(alpha - a64)
    err = _rel(grad, g64)
    print(f"{name}: max |alpha - f64| compared {d[~ex].max():.3e} (bar {BAR_FWD:.2e}), excluded {d[ex].max() if ex.any() else 0:.3e} on {int(ex.sum())} pixels; "
          f"gradient err {err:.3e} (bar {BAR_BWD:.2e}), |g|inf {np.abs(g64).max():.3e}")
    assert d[~ex].max() <= BAR_FWD
    assert (alpha[~ex & (a64 == 0)] == 0).all()
    assert (alpha[~ex & (a64 == 1)] >= 1 - BAR_FWD).all() and alpha.max() <= 1.0 and alpha.min() >= 0.0
    assert not ex.any() or d[ex].max() <= so.EXCLUDED_BAR
    assert err <= BAR_BWD
    # determinism: the same bytes again, and from int32 faces
    again = _both(v, f, cams, S, c["grad_alpha"])
    i32 = _both(v, f, cams, S, c["grad_alpha"], torch.int32)
    for other in (again, i32):
        assert other[0].tobytes() == alpha.tobytes() and other[1].tobytes() == grad.tobytes()


@pytest.mark.parametrize("name", ["ico", "sliver"])
def test_gpu_silhouette_single_views_leave_the_view_axis_alone(name):
    """each view alone: the coordinate along its axis gets exactly nothing; the views' gradients add up to the joint call's"""
    c = so.case(name)
    v, f, S, cams = c["verts"], c["faces"], c["S"], c["cams"]
    total = np.zeros(v.shape, np.float64)
    for k, cam in enumerate(cams):
        ga = c["grad_alpha"][k:k + 1]
        if len(cams) == 2 and cam == 2:
            ga = ga[:, :, ::-1]                                            # a single view is not mirrored
        _, g = _both(v, f, (cam,), S, ga)
        axis = 0 if cam & 1 else 2
        assert (g[:, axis] == 0).all() and np.abs(g[:, 2 - axis]).max() > 0 and np.abs(g[:, 1]).max() > 0
        total += g
    _, joint = _both(v, f, cams, S, c["grad_alpha"])
    assert np.abs(total - joint).max() <= 4 * 2.0 ** -23 * np.abs(joint).max() * len(cams)


def test_gpu_silhouette_two_view_call_mirrors_camera_2():
    c = so.case("ico_offset")
    v, f, S = c["verts"], c["faces"], c["S"]
    two = _forward(v, f, (0, 2), S)
    front, back = _forward(v, f, (0,), S), _forward(v, f, (2,), S)
    assert torch.equal(two[0:1], front) and torch.equal(two[1:2], torch.flip(back, dims=[2])) and not torch.equal(two[1:2], back)
    four = _forward(v, f, (0, 1, 2, 3), S)
    assert torch.equal(four[2:3], back)


def test_gpu_silhouette_bad_faces_are_skipped_and_counted():
    """the C entries themselves: `bad` renders and differentiates as `ico` does (equal bytes), the face naming vertex V is counted
    in the first word of the scratch by either direction, and a too small scratch is refused"""
    from icon_amd import _lib
    from icon_amd.engine import _stream
    b, i = so.case("bad"), so.case("ico")
    v, f, S, cams = b["verts"], b["faces"], b["S"], b["cams"]
    assert np.array_equal(v, i["verts"]) and len(f) == len(i["faces"]) + 3
    ga = b["grad_alpha"]
    vd, fd = _dev(v), _dev(f)
    L = _lib.lib()
    n = C.c_int64(0)
    assert L.icon_silhouette_bytes(C.c_int64(len(v)), C.c_int64(len(f)), C.c_int(S), C.c_int(2), C.byref(n)) == 0
    scratch = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    alpha = torch.empty((2, S, S), device="cuda")
    gv = torch.empty((len(v), 3), device="cuda")
    gad = _dev(ga, torch.float32)
    p = lambda t: C.c_void_p(t.data_ptr())
    head = (p(vd), C.c_int64(len(v)), p(fd), C.c_int64(len(f)), C.c_int(1), (C.c_int * 2)(*cams), C.c_int(2), C.c_int(S))
    assert L.icon_silhouette_forward(*head, p(alpha), p(scratch), C.c_int64(n.value - 1), _stream()) == 1 and b"scratch" in L.icon_last_error()
    assert L.icon_silhouette_forward(*head, p(alpha), p(scratch), C.c_int64(n.value), _stream()) == 0
    torch.cuda.synchronize()
    assert int(scratch[:4].view(torch.int32).item()) == 1
    scratch.fill_(0xff)                                                    # the backward call does not need what the forward left
    assert L.icon_silhouette_backward(*head, p(alpha), p(gad), p(gv), p(scratch), C.c_int64(n.value), _stream()) == 0
    torch.cuda.synchronize()
    assert int(scratch[:4].view(torch.int32).item()) == 1
    ref_alpha, ref_grad = _both(i["verts"], i["faces"], cams, S, ga)
    assert alpha.cpu().numpy().tobytes() == ref_alpha.tobytes()
    assert gv.cpu().numpy().tobytes() == ref_grad.tobytes()


def test_gpu_silhouette_zero_grad_alpha_gives_zero_gradient():
    c = so.case("fan")
    _, g = _both(c["verts"], c["faces"], c["cams"], c["S"], np.zeros_like(c["grad_alpha"]))
    assert (g == 0).all()


def test_gpu_silhouette_autograd_reaches_the_leaf_through_the_render_class():
    """verts = base + trans, trans a leaf: load_meshes -> get_silhouette_image -> L1 loss -> backward; trans.grad is the column
    sums of the oracle's grad_verts for that loss.  get_rgb_image after the same load_meshes: the bytes of a detached mesh"""
    from icon_amd.render import Render
    c = so.case("ico")
    v, f, S = c["verts"], c["faces"], c["S"]
    target, _, _ = so.descent_f64()
    ref = so.silhouette(v, f, (0, 2), S, grad_alpha=lambda k, r, cc, a: np.sign(a - target[k, r, cc]) / (S * S))
    base, fd = _dev(v), _dev(f)
    trans = torch.zeros(3, device="cuda", requires_grad=True)
    r = Render(size=S, device=torch.device("cuda:0"))
    r.load_meshes(base + trans, fd)
    sil = r.get_silhouette_image()
    assert len(sil) == 2 and all(t.shape == (1, S, S) and t.requires_grad for t in sil)
    loss = (torch.cat(sil) - _dev(target, torch.float32)).abs().sum() / (S * S)
    loss.backward()
    want = ref["grad_verts"].sum(0)
    got = trans.grad.cpu().numpy()
    print(f"trans.grad {got}, oracle {want}")
    assert np.abs(got - want).max() <= BAR_BWD * np.abs(want).max()
    rgb = r.get_rgb_image()
    assert not rgb[0].requires_grad
    r2 = Render(size=S, device=torch.device("cuda:0"))
    r2.load_meshes(base, fd)
    assert all(torch.equal(a, b) for a, b in zip(rgb, r2.get_rgb_image()))
    assert all(torch.equal(a.detach(), b) for a, b in zip(sil, r2.get_silhouette_image()))


def test_gpu_silhouette_forward_replays_from_a_captured_graph():
    """single stream, one linear chain of kernel nodes: the call allocates nothing and waits for nothing"""
    from icon_amd.render import silhouette_device
    c = so.case("ico")
    vd, fd = _dev(c["verts"]), _dev(c["faces"])
    want = silhouette_device(vd, fd, c["cams"], c["S"]).cpu().numpy()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        silhouette_device(vd, fd, c["cams"], c["S"])                       # warm-up: scratch of this stream
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        alpha = silhouette_device(vd, fd, c["cams"], c["S"])
    for _ in range(2):
        alpha.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert alpha.cpu().numpy().tobytes() == want.tobytes()


def test_gpu_silhouette_descent_follows_the_oracle():
    """ten plain gradient steps on the translation towards the shifted sphere's silhouette, smooth loss sum (alpha - target)^2 /
    (2 S^2) (silhouette_oracle has the reason): the device's losses follow the float64 oracle's - each within the forward bar x
    (pixels that differ from the target) / S^2 - and fall at every step"""
    from icon_amd.render import silhouette_device
    c = so.case("ico")
    v, f, S = c["verts"], c["faces"], c["S"]
    target, want, ndiff = so.descent_f64()
    assert (np.diff(want) < 0).all()
    base, fd, tgt = _dev(v), _dev(f), _dev(target, torch.float32)
    trans = torch.zeros(3, device="cuda", requires_grad=True)
    losses = []
    for _ in range(so.DESCENT_STEPS + 1):
        alpha = silhouette_device(base + trans, fd, (0, 2), S)
        losses.append(so.l2_loss(alpha.detach().cpu().numpy().astype(np.float64), target))
        loss = ((alpha - tgt) ** 2).sum() / (2 * S * S)
        trans.grad = None
        loss.backward()
        with torch.no_grad():
            trans -= so.DESCENT_LR * trans.grad
    losses = np.array(losses)
    print("device ", losses, "\noracle ", want, "\nbound  ", BAR_FWD * ndiff / (S * S))
    assert (np.diff(losses) < 0).all()
    assert (np.abs(losses - want) <= BAR_FWD * ndiff / (S * S)).all()

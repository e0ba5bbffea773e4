"""icon_amd._native on the device: ONE scratch pool for every family of native calls, keyed by (thread, device, stream).

What sharing the pool adds as a hazard is that a call now finds what ANY previous call left in the scratch, not only its own
leftovers: every scratch-taking Python entry is run over a scratch full of 0x00 and over one full of 0xff and must give equal
bytes.  Shapes: the icosahedron (V = 12, F = 20; the level-0 mesh of the render tests' icosphere), images of 32 to 128 pixels,
N <= 1,001 points, B <= 2 - the smallest that reach every piece of each call's scratch layout."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import smpl_oracle as so
import test_native_call as tn
from icon_amd import _lib, _native, synth

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _ico():
    v, f = synth.icosphere(0, radius=0.55, center=(0.05, -0.1, 0.02))
    assert v.shape == (12, 3) and f.shape == (20, 3)
    return torch.from_numpy(v.astype(np.float32)).cuda(), torch.from_numpy(f.astype(np.int64)).cuda()


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


_filled = []                        # (thread, bytes filled) of every _fill


def _fill(value):
    """this thread's and this stream's scratch, as a warm-up sized it, set to ``value``"""
    buf = _native.scratch(_dev(), 1)
    assert buf.numel() > 1, "the warm-up did not size this thread's scratch"
    buf.fill_(value)
    _filled.append((threading.get_ident(), buf.numel()))


def _fill_in_backward(t, value):
    """the backward calls run on autograd's device thread, whose pool is its own: fill THAT scratch, just before the gradient of
    ``t`` reaches the function that made it"""
    if value is not None:
        t.register_hook(lambda g: _fill(value))
    return t


# ---- every scratch-taking Python entry: (value the backward's scratch is filled with, or None) -> its outputs -------------------
def _e_query_color(fill):
    from icon_amd.recon import query_color_device
    v, f = _ico()
    image = torch.linspace(-1, 1, 3 * 16 * 16, device="cuda").reshape(1, 3, 16, 16)
    return query_color_device(v, f, image, image_size=64, return_vis=True)


def _e_render_normal(fill):
    from icon_amd.render import render_normal_device
    v, f = _ico()
    v.requires_grad_(True)
    images, depth, pix = render_normal_device(v, f.int(), (0, 1, 2, 3), 64, return_depth=True, return_faces=True, differentiable=True)
    g = torch.linspace(-1, 1, images.numel(), device="cuda").reshape(images.shape)
    grad, = torch.autograd.grad(_fill_in_backward(images, fill), v, g)
    return images.detach(), depth, pix, grad


def _e_turntable(fill):
    from icon_amd.render import render_turntable_device
    v, f = _ico()
    return render_turntable_device(v, f, (0.0, 33.3, 90.0, 200.0, 359.0), 32, return_images=True, return_depth=True, return_faces=True)


def _e_silhouette(fill):
    from icon_amd.render import silhouette_device
    v, f = _ico()
    v.requires_grad_(True)
    alpha = silhouette_device(v, f, (0, 2), 32)
    g = torch.linspace(-1, 1, alpha.numel(), device="cuda").reshape(alpha.shape)
    grad, = torch.autograd.grad(_fill_in_backward(alpha, fill), v, g)
    return alpha.detach(), grad


def _cloth_inputs(B):
    from icon_amd.cloth import ClothTopology
    v, f = _ico()
    gen = torch.Generator().manual_seed(3)
    A = (torch.eye(3)[None, None] + 0.05 * torch.randn(B, 12, 3, 3, generator=gen)).cuda()
    b = (0.02 * torch.randn(B, 12, 3, 1, generator=gen)).cuda()
    return v, ClothTopology(f, num_verts=12), A, b


def _e_local_affine(fill):
    from icon_amd.cloth import local_affine_device
    v, topo, A, b = _cloth_inputs(2)
    return local_affine_device(v[None].repeat(2, 1, 1) * torch.tensor([1.0, 0.5], device="cuda")[:, None, None], A, b, topo)


def _e_mesh_priors(fill):
    from icon_amd.cloth import mesh_shape_prior_losses_device
    v, topo, _, _ = _cloth_inputs(1)
    v.requires_grad_(True)
    e, n, l = mesh_shape_prior_losses_device(v, topo, target_length=0.1)
    total = _fill_in_backward(1.5 * e + 0.5 * n + 2.0 * l, fill)
    grad, = torch.autograd.grad(total, v)
    return e.detach(), n.detach(), l.detach(), grad


_smpl_model = []


def _e_smpl(fill):
    from icon_amd.smpl import SmplModel, smpl_lbs_device
    if not _smpl_model:
        _smpl_model.append(SmplModel(*(torch.from_numpy(np.ascontiguousarray(so.case("tree")[k])).cuda() for k in so.BUFFERS)))
    betas, rot, gv, gj = (torch.from_numpy(a).cuda() for a in so.inputs("tree", 2))
    betas.requires_grad_(True), rot.requires_grad_(True)
    verts, joints = smpl_lbs_device(betas, rot, _smpl_model[0])
    total = _fill_in_backward((verts * gv).sum() + (joints * gj).sum(), fill)
    g_betas, g_rot = torch.autograd.grad(total, (betas, rot))
    return verts.detach(), joints.detach(), g_betas, g_rot


def _e_extract_cloth(fill):
    from icon_amd.garment import extract_cloth_device
    v, f = _ico()
    square = np.array([[-1.0, -1.0], [0.2, -1.0], [0.2, 1.0], [-1.0, 1.0]])
    src = torch.tensor([[0.0, 0.4, 0.0], [0.0, -0.6, 0.0], [-0.4, 0.0, 0.1]], device="cuda")
    out = extract_cloth_device(v, f, [square], src, torch.tensor([True, False, False], device="cuda"), return_index=True)
    assert out is not None and 0 < out[1].shape[0] < 20                  # some faces kept, some dropped
    return out


def _e_normal_consistency(fill):
    from icon_amd.evaluator import normal_consistency_device
    v, f = _ico()
    return normal_consistency_device(v, f, v * 0.9 + 0.03, f.int(), degs=(0, 180, 90, 270), size=32, return_images=True, return_faces=True,
                                     return_normals=True)


_scan = []


def _ico_scan():
    from icon_amd.sampling import ScanMesh
    if not _scan:
        _scan.append(ScanMesh(*_ico()))
    return _scan[0]


def _e_sample_geo(fill):
    from icon_amd.sampling import sample_geo_device
    s, l, c, extra = sample_geo_device(_ico_scan(), np.eye(4), 50, 0.05, zray_type=True, ray_sample_num=2, seed=11, return_all=True)
    plain = sample_geo_device(_ico_scan(), np.eye(4), 50, 0.05, zray_type=True, ray_sample_num=2, seed=11)     # the lists live in the scratch
    return (s, l, c, extra["all_samples"], extra["all_inside"], extra["source"], extra["vertex"]) + tuple(plain)


def _e_point_features(fill):
    from icon_amd import training
    from icon_amd.engine import IconQueryEngine
    eng = IconQueryEngine(prior_type="pifu", sdf_clip=0.05, smpl_feats=())
    B, N = 2, 1001
    rng = np.random.RandomState(5)
    stacks = [torch.from_numpy(rng.randn(B, 12, 8, 8).astype(np.float32)).cuda().requires_grad_(True) for _ in range(2)]
    pts = torch.from_numpy(rng.uniform(-1.1, 1.1, (B, 3, N)).astype(np.float32)).cuda()
    calibs = torch.eye(4, device="cuda")[None].repeat(B, 1, 1)
    rows, in_cube = training.point_features_device(eng, stacks, pts, calibs)
    g = torch.from_numpy(rng.randn(*rows[0].shape).astype(np.float32)).cuda()
    total = _fill_in_backward((rows[0] * g).sum() + 0.5 * (rows[1] * g).sum(), fill)
    grads = torch.autograd.grad(total, stacks)
    return (rows[0].detach(), rows[1].detach(), in_cube) + tuple(grads)


# name -> (entry, which of its directions take a scratch: "f" the forward - the calling thread's -, "b" the backward - autograd's)
ENTRIES = {
    "query_color_device": (_e_query_color, "f"),
    "render_normal_device": (_e_render_normal, "fb"),
    "render_turntable_device": (_e_turntable, "f"),
    "silhouette_device": (_e_silhouette, "fb"),
    "local_affine_device": (_e_local_affine, "f"),
    "mesh_shape_prior_losses_device": (_e_mesh_priors, "fb"),
    "smpl_lbs_device": (_e_smpl, "b"),
    "extract_cloth_device": (_e_extract_cloth, "f"),
    "normal_consistency_device": (_e_normal_consistency, "f"),
    "sample_geo_device": (_e_sample_geo, "f"),
    "point_features_device": (_e_point_features, "b"),
}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_a_call_needs_nothing_the_previous_user_left(name):
    """torch.empty guarantees nothing about a fresh scratch either: a call that fails here has a clear to fix, not the pool"""
    entry, takes = ENTRIES[name]
    entry(None)                                                            # the warm-up sizes the scratch of the threads that take one
    torch.cuda.synchronize()
    outs = []
    for value in (0x00, 0xff):
        del _filled[:]
        if "f" in takes:
            _fill(value)
        outs.append([t.clone() for t in entry(value if "b" in takes else None)])
        torch.cuda.synchronize()
        threads = {t for t, _ in _filled}
        assert len(threads) == len(takes), _filled                         # each direction's own thread, each filled
        assert ("b" in takes) == any(t != threading.get_ident() for t in threads)
    assert len(outs[0]) == len(outs[1]) and all(_same_bytes(a, b) for a, b in zip(*outs)), name
    assert all(torch.isfinite(t).all() for t in outs[0] if t.dtype.is_floating_point)


def _bytes(entry, *args):
    n = C.c_int64(0)
    assert getattr(_lib.lib(), entry)(*args, C.byref(n)) == 0
    return n.value


def _in_a_new_thread(body):
    """a new thread starts with an empty pool, whatever the tests before have rendered; its assertions are raised here"""
    caught = []

    def run():
        try:
            body()
            torch.cuda.synchronize()
        except BaseException as e:                                         # noqa: BLE001 - handed to the caller
            caught.append(e)

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if caught:
        raise caught[0]


def test_one_pool_across_the_families():
    """render, query_color and garment extraction had a pool each: now the largest call's tensor serves all three"""
    from icon_amd.garment import extract_cloth_device
    from icon_amd.recon import query_color_device
    from icon_amd.render import render_normal_device
    v, f = _ico()
    square = np.array([[-1.0, -1.0], [0.2, -1.0], [0.2, 1.0], [-1.0, 1.0]])
    i64, i32 = C.c_int64, C.c_int
    need = (_bytes("icon_render_bytes", i64(12), i64(20), i32(128), i32(4)), _bytes("icon_query_color_bytes", i64(12), i64(20), i32(64)),
            _bytes("icon_extract_cloth_bytes", i64(12), i64(20), i64(4), i64(1)))
    assert need[0] > need[1] and need[0] > need[2], need                  # the precondition: the first call's scratch is the largest

    def body():
        dev = _dev()
        render_normal_device(v, f, (0, 1, 2, 3), 128)
        buf = _native.scratch(dev, 1)
        assert buf.numel() == need[0]
        query_color_device(v, f, torch.zeros(1, 3, 16, 16, device="cuda"), image_size=64)
        assert _native.scratch(dev, 1) is buf
        assert extract_cloth_device(v, f, [square]) is not None
        assert _native.scratch(dev, 1) is buf

    _in_a_new_thread(body)


def _range(t):
    return t.data_ptr(), t.data_ptr() + t.numel()


def test_a_scratch_per_stream_and_per_thread():
    from icon_amd.render import render_normal_device
    v, f = _ico()
    dev = _dev()
    want = render_normal_device(v, f, (0, 2), 32, return_depth=True, return_faces=True)
    main = _native.scratch(dev, 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = render_normal_device(v, f, (0, 2), 32, return_depth=True, return_faces=True)
        other = _native.scratch(dev, 1)
    torch.cuda.synchronize()
    assert other is not main and (_range(other)[1] <= _range(main)[0] or _range(main)[1] <= _range(other)[0])
    assert _native.scratch(dev, 1) is main
    assert all(_same_bytes(a, b) for a, b in zip(got, want))
    seen = []
    t = threading.Thread(target=lambda: seen.append(_native.scratch(dev, 1024)))
    t.start()
    t.join()
    assert len(seen) == 1 and seen[0] is not main and seen[0] is not other and seen[0].data_ptr() not in (main.data_ptr(), other.data_ptr())


def test_growth_keeps_the_results():
    from icon_amd.render import render_normal_device
    v, f = _ico()

    def body():
        dev = _dev()
        first = render_normal_device(v, f, (0, 1, 2, 3), 32, return_depth=True, return_faces=True)
        small = _native.scratch(dev, 1)
        render_normal_device(v, f, (0, 1, 2, 3), 128, return_depth=True, return_faces=True)
        large = _native.scratch(dev, 1)
        assert large is not small and large.numel() > small.numel()      # it grew: the third call runs in a scratch it did not size
        third = render_normal_device(v, f, (0, 1, 2, 3), 32, return_depth=True, return_faces=True)
        assert _native.scratch(dev, 1) is large
        assert all(_same_bytes(a, b) for a, b in zip(third, first))

    _in_a_new_thread(body)


@pytest.mark.parametrize("row", [r for r in tn.SCRATCH_ROWS if r[4]], ids=lambda r: r[0])
def test_scratch_checks_of_the_entries_that_need_a_device(row):
    tn.check_scratch_row(row, scan=_ico_scan().handle.h)

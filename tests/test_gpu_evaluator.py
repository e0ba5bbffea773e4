"""icon_normal_consistency / icon_amd.evaluator on the device against the numpy statement of the rule (tests/gl_checker.py, itself
held to exact rational coverage and to the reference's own Evaluator class by tests/test_evaluator.py).  With
caller-given normals everything is compared for EQUALITY: RGBA images, winning faces, float64 errors.  The angle-weighted vertex
normals go through acos, which differs between libm and the device library: they are held to one float32 ulp, and what follows from
them to the bound derived from that.  Index types, lane mappings, the deferred path, streams, K = 1 and K = 32, and the Evaluator
class on the device against the same class over the checker."""
import ctypes as C

import numpy as np
import pytest
import torch

import gl_checker as glc

pytestmark = pytest.mark.gpu

VIEWS = dict(degs=[0, 180, 90, 270, 37.5])


def _dev(x, dtype=None):
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dtype is None else t.to(dtype)


def _option(n):
    from icon_amd import _lib
    assert _lib.lib().icon_debug_set_option(b"ev_lanes", C.c_int(n)) == 0


def _call(va, fa, na, vb, fb, nb, mats, muls, S, dtype=torch.int64):
    """-> err, rgba_a, rgba_b, pix_a, pix_b as numpy"""
    from icon_amd.evaluator import normal_consistency_device
    out = normal_consistency_device(_dev(va), _dev(fa, dtype), _dev(vb), _dev(fb, dtype), degs=None, size=S, normals_a=_dev(na), normals_b=_dev(nb),
                                    mats=mats, muls=muls, return_images=True, return_faces=True)
    return tuple(t.cpu().numpy() for t in out)


def _same(got, want):
    return len(got) == len(want) and all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, want))


def _want(va, fa, na, vb, fb, nb, mats, muls, S):
    err, A, B = glc.normal_consistency(va, fa, vb, fb, mats, muls, S, na, nb)
    return err, A[0], B[0], A[1], B[1]


def _mats(scale=1.0, offset=0.0, **kw):
    from icon_amd.evaluator import view_matrices
    m = view_matrices(kw.get("degs", VIEWS["degs"]), scale, offset)
    return m, np.ones((len(m), 3), np.float32)


def _cases():
    """name -> (va, fa, vb, fb, mats, muls): small meshes for S = 8, 16, 32"""
    out = {}
    ia, fi = glc.ico(2, 0.6)
    ib = (ia + np.random.RandomState(2).normal(0, 0.01, ia.shape)).astype(np.float32)
    out["ico"] = (ia, fi, ib, fi, *_mats())
    out["ico_scaled_offset"] = (ia, fi, ib, fi, *_mats(0.75, -0.125))
    # wider than the viewport: faces lie partly or wholly outside it (its depth stays inside the near / far planes)
    big, _ = glc.ico(2, 1.3)
    out["clipped"] = (big, fi, ia, fi, *_mats())
    # near / far: the icosphere stretched to |x|, |z| ~ 2 and a large face from z = -2 to z = 2, in front of and behind an unstretched one
    # that shares the mesh - the interpolated depth passes +1 and -1 over covered centres in every view
    deep = np.concatenate([ia * np.float32([6, 1, 6]), 0.5 * ia, [[-0.9, -0.8, -2.0], [0.9, -0.7, 2.0], [0.1, 0.9, 0.3]]]).astype(np.float32)
    fd = np.concatenate([fi, fi + len(ia), [[2 * len(ia), 2 * len(ia) + 1, 2 * len(ia) + 2]]])
    out["near_far"] = (deep, fd, ia, fi, *_mats())
    # a face with a coordinate beyond 64 (not drawn), a face that names a missing vertex (skipped), next to real ones
    v = np.concatenate([ia, [[100.0, 0.0, 0.0], [0.0, -70.0, 0.2], [0.3, 0.3, 0.9]]]).astype(np.float32)
    f = np.concatenate([[[0, 1, len(ia)], [len(ia) + 1, 2, 3], [0, 1, len(v)], [-1, 2, 3], [0, 5, len(ia) + 2]], fi])
    out["guard_and_missing"] = (v, f, ia, fi, *_mats())
    return out


@pytest.mark.parametrize("S", [8, 16, 32])
@pytest.mark.parametrize("name", ["ico", "ico_scaled_offset", "clipped", "guard_and_missing", "near_far"])
def test_gpu_images_winners_and_errors_equal_the_checker(name, S):
    va, fa, vb, fb, mats, muls = _cases()[name]
    na, nb = glc.random_normals(len(va), 1), glc.random_normals(len(vb), 2)
    want = _want(va, fa, na, vb, fb, nb, mats, muls, S)
    got = _call(va, fa, na, vb, fb, nb, mats, muls, S)
    print(f"{name} S={S}: err {got[0]}, {int((got[3] != want[3]).sum())} + {int((got[4] != want[4]).sum())} pixels with another face, "
          f"covered {int((want[3] >= 0).sum())} + {int((want[4] >= 0).sum())}")
    assert got[0].dtype == np.float64 and got[0].shape == (len(mats),) and got[1].shape == (len(mats), S, S, 4) and got[3].dtype == np.int32
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
    assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
    assert got[0].tobytes() == want[0].tobytes()
    assert (want[3] >= 0).any() and (want[0] > 0).all()
    if name == "clipped":
        clip = np.concatenate([glc.clip_f32(va, M) for M in mats])
        assert (np.abs(clip[:, :2]) > 1).any() and (np.abs(clip[:, 2]) < 1).all()
    if name == "near_far":                                                   # the case depends on the clipping: without it the checker differs, in every view
        try:
            glc.NEAR_FAR = False
            loose = glc.render(va, fa, na, mats, muls, S)
        finally:
            glc.NEAR_FAR = True
        changed = [int((loose[1][k] != want[3][k]).sum()) for k in range(len(mats))]
        clip_z = np.concatenate([glc.clip_f32(va, M)[:, 2] for M in mats])
        print(f"near_far S={S}: winners that change per view without the near / far test {changed}; clip z in [{clip_z.min():.2f}, {clip_z.max():.2f}]")
        assert min(changed) > 0 and clip_z.min() < -1 and clip_z.max() > 1
        assert any(loose[0][k].tobytes() != want[1][k].tobytes() for k in range(len(mats)))
    # int32 faces and both lane mappings: the same bytes
    assert _same(_call(va, fa, na, vb, fb, nb, mats, muls, S, torch.int32), got)
    try:
        for lanes in (1, 8):
            _option(lanes)
            assert _same(_call(va, fa, na, vb, fb, nb, mats, muls, S), got), lanes
    finally:
        _option(0)


@pytest.mark.parametrize("S", [8, 16, 32])
def test_gpu_edges_vertices_and_equal_depths(S):
    """centres exactly on every kind of edge and on a vertex, both windings, a sliver, a zero-area face, the quad and the fans
    (coplanar faces at equal depth: the lower id wins), all in one mesh against another"""
    meshes = list(glc.edge_cases(S).values()) + [glc.quad(S), glc.fan(S, 7), glc.fan(S, 12)]
    for k, (v, f) in enumerate(meshes):
        other_v, other_f = meshes[(k + 1) % len(meshes)]
        na, nb = glc.random_normals(len(v), k), glc.random_normals(len(other_v), k + 50)
        mats, muls = glc.identity_views(2)
        muls[1] = [-1, -1, 1]
        want = _want(v, f, na, other_v, other_f, nb, mats, muls, S)
        got = _call(v, f, na, other_v, other_f, nb, mats, muls, S)
        assert _same(got, want), k
        try:
            for lanes in (1, 8):
                _option(lanes)
                assert _same(_call(v, f, na, other_v, other_f, nb, mats, muls, S, torch.int32), want), (k, lanes)
        finally:
            _option(0)
    # two coplanar copies of one face: the lower id wins
    c = lambda i: glc.ndc(256 * i + 128, S)
    tri = lambda z: [[c(0), c(0), z], [c(7), c(0), z], [c(0), c(7), z]]
    v = np.array(tri(0.25) + tri(0.25), np.float32)
    f = np.array([[3, 4, 5], [0, 1, 2]])
    mats, muls = glc.identity_views(1)
    # -0 against +0, the HIGHER id carrying -0: by the bits alone it would win.  The affine sum gives clip z = +0 only from terms that
    # are all -0: a face in the positive quadrant under a view whose third row is (-0, -0, 1, -0) gets clip z = +0 from z = -0 and -0 from z = +0
    q = S // 2                                                               # the first pixel whose centre has positive coordinates
    triq = lambda z: [[c(q), c(q), z], [c(q + 3), c(q), z], [c(q), c(q + 3), z]]
    vz = np.array(triq(np.float32(-0.0)) + triq(0.0), np.float32)
    fz = np.array([[0, 1, 2], [3, 4, 5]])
    mz = mats.copy()
    mz[0, 2] = [-0.0, -0.0, 1.0, -0.0]
    signs = np.signbit(glc.clip_f32(vz, mz[0])[:, 2])
    assert not signs[:3].any() and signs[3:].all()
    for va_, fa_, m_ in ((v, f, mats), (vz, fz, mz)):
        got = _call(va_, fa_, glc.random_normals(6), va_, fa_[::-1].copy(), glc.random_normals(6, 1), m_, muls, S)
        assert set(np.unique(got[3])) == {-1, 0} and set(np.unique(got[4])) == {-1, 0}
        assert _same(got, _want(va_, fa_, glc.random_normals(6), va_, fa_[::-1].copy(), glc.random_normals(6, 1), m_, muls, S))


def test_gpu_one_face_over_the_whole_image_takes_the_deferred_path():
    S = 32
    v = np.array([[-3, -3, 0.5], [3, -3, -0.5], [0, 4, 0.1], [-0.5, -0.5, 0.9], [0.5, -0.5, 0.9], [0, 0.5, 0.9]], np.float32)
    f = np.array([[0, 1, 2], [3, 4, 5]])
    ia, fi = glc.ico(2, 0.6)
    mats, muls = _mats()
    na, nb = glc.random_normals(6), glc.random_normals(len(ia), 1)
    want = _want(v, f, na, ia, fi, nb, mats, muls, S)
    assert (want[3][0] >= 0).all() and (want[3][0] == 1).any()                # every pixel of view 0 is covered; the small face is in front
    try:
        for lanes in (0, 1, 8):
            _option(lanes)
            assert _same(_call(v, f, na, ia, fi, nb, mats, muls, S), want), lanes
    finally:
        _option(0)


def test_gpu_body_at_64():
    va, fa, na, vb, fb, nb, mats, muls, err, A, B = glc.body_case(64)
    got = _call(va, fa, na, vb, fb, nb, mats, muls, 64)
    print(f"body S=64: err {got[0]} (checker {err}), covered {int((A[1] >= 0).sum())}")
    assert _same(got, (err, A[0], B[0], A[1], B[1]))
    assert (A[1] >= 0).sum() > 1500 and (err > 0).all()


def test_gpu_angle_weighted_normals_and_what_follows_from_them():
    """the normals within one float32 ulp of the checker's; with them each view's error within 2e-6 of the checker's: a colour
    channel moves by at most about one ulp of 1 when a normal does, and d(d0^2 + d1^2 + d2^2) = 2 |d| x that over 3 channels with |d| <= 1:
    3 x 2 x 1.2e-7 = 7.2e-7 per pixel, and so for the mean; 2e-6 leaves room for the interpolation's own rounding"""
    from icon_amd.evaluator import normal_consistency_device
    for name, S in (("ico", 32), ("body", 64)):
        if name == "body":
            va, fa, _, vb, fb, _, mats, muls, _, _, _ = glc.body_case(64)
        else:
            va, fa, vb, fb, mats, muls = _cases()["ico"]
            fa = np.concatenate([fa, [[0, 1, len(va)], [2, 2, 3]]])          # a missing vertex and a degenerate face add nothing
        err, ra, rb, na, nb = normal_consistency_device(_dev(va), _dev(fa), _dev(vb), _dev(fb, torch.int32), degs=None, mats=mats, muls=muls,
                                                         size=S, return_images=True, return_normals=True)
        wa, wb = glc.vertex_normals(va, fa), glc.vertex_normals(vb, fb)
        ua, ub = glc.ulps(na.cpu().numpy(), wa), glc.ulps(nb.cpu().numpy(), wb)
        want = glc.normal_consistency(va, fa, vb, fb, mats, muls, S, wa, wb)[0]
        diff = np.abs(err.cpu().numpy() - want).max()
        print(f"{name}: normals {ua:.2f} / {ub:.2f} ulps from the checker's; NC per view off by at most {diff:.3e} (values {want})")
        assert na.dtype == torch.float32 and na.shape == (len(va), 3) and ua <= 1.0 and ub <= 1.0
        assert diff <= 2e-6
        # given back as the caller's normals, the call computes what it computed
        again = normal_consistency_device(_dev(va), _dev(fa), _dev(vb), _dev(fb), degs=None, mats=mats, muls=muls, size=S, normals_a=na, normals_b=nb,
                                          return_images=True)
        assert torch.equal(again[0], err) and torch.equal(again[1], ra) and torch.equal(again[2], rb)


def test_gpu_long_incidence_lists():
    """a hub with 200 faces around it: more than one thread sums (s1_normals_device.h kShort = 32) - the wavefront path"""
    from icon_amd.evaluator import normal_consistency_device
    n = 200
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False)
    v = np.concatenate([[[0.01, 0.02, 0.3]], np.stack([0.8 * np.cos(ang), 0.8 * np.sin(ang), 0.05 * np.cos(5 * ang)], 1)]).astype(np.float32)
    f = np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)])
    f = f[np.random.RandomState(0).permutation(n)]
    _, nrm = normal_consistency_device(_dev(v), _dev(f), size=16, degs=[0], return_normals=True)
    u = glc.ulps(nrm.cpu().numpy(), glc.vertex_normals(v, f))
    print(f"hub of {n} faces: {u:.2f} ulps")
    assert u <= 1.0


def test_gpu_identical_meshes_two_runs_a_side_stream_and_view_counts():
    from icon_amd.evaluator import normal_consistency_device
    va, fa, vb, fb, _, _ = _cases()["ico"]
    a, b = (_dev(va), _dev(fa)), (_dev(vb), _dev(fb))
    S = 32
    assert (normal_consistency_device(*a, *a, size=S).cpu().numpy() == 0).all()
    degs32 = list(np.arange(32) * 11.25)
    first = normal_consistency_device(*a, *b, degs=degs32, size=S, return_images=True, return_faces=True)
    second = normal_consistency_device(*a, *b, degs=degs32, size=S, return_images=True, return_faces=True)
    assert first[0].shape == (32,) and all(torch.equal(x, y) for x, y in zip(first, second))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        third = normal_consistency_device(*a, *b, degs=degs32, size=S, return_images=True, return_faces=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, third))
    one = normal_consistency_device(*a, *b, degs=[degs32[5]], size=S, return_images=True)
    assert one[0].shape == (1,) and torch.equal(one[0][0], first[0][5]) and torch.equal(one[1][0], first[1][5])
    # against the checker at four of the 32 (computed normals: the bound of the test above)
    want = glc.normal_consistency(va, fa, vb, fb, *_mats(degs=degs32[::8]), S)[0]
    assert np.abs(first[0].cpu().numpy()[::8] - want).max() <= 2e-6
    # the single-mesh form renders only
    img = normal_consistency_device(*a, degs=degs32[:3], size=S)
    assert img.shape == (3, S, S, 4) and torch.equal(img, first[1][:3])


def test_gpu_evaluator_class_equals_the_same_class_over_the_checker(monkeypatch):
    """Evaluator on the device against Evaluator on host tensors with the checker in the native call's place (what
    tests/test_evaluator.py holds to the reference's own class).  Its normals are computed ones: the maps may move by what one ulp
    of a unit normal moves a colour (2 x 1.2e-7 through the normalisation, doubled by 2 (img - 0.5)): 1e-6; NC by 2e-6 per side"""
    from icon_amd import evaluator as ev
    S = 32
    dev = ev.Evaluator(torch.device("cuda:0"), size=S)
    dev.set_mesh(glc.result_dict())
    dev.space_transfer()
    assert dev.verts_pr.is_cuda and dev.src_mesh.vertices.is_cuda and dev.tgt_mesh.faces.is_cuda
    got = {bits: dev.calculate_normal_consist(*[bool(bits >> i & 1) for i in range(4)]) for bits in (1, 6, 15)}
    demo = dev.calculate_normal_consist(return_demo=True)
    v, f = glc.ico(2, 0.7)
    maps = dev.render_normal(_dev(v)[None], _dev(f)[None])
    lst = dev.render_mesh_list([dev.src_mesh, dev.tgt_mesh])
    host = ev.Evaluator("cpu", size=S)
    host.set_mesh({k: (x.cpu() if torch.is_tensor(x) else x) for k, x in glc.result_dict().items()})
    host.space_transfer()
    host.verts_gt = dev.verts_gt.cpu()                                       # the 3 x 3 product of space_transfer: the device's bits
    host.tgt_mesh = ev.EvalMesh(host.verts_gt, host.faces_gt)
    assert torch.equal(host.verts_pr, dev.verts_pr.cpu())
    monkeypatch.setattr(ev, "normal_consistency_device", glc.checker_backend)
    for bits, nc in got.items():
        want = host.calculate_normal_consist(*[bool(bits >> i & 1) for i in range(4)])
        print(f"sides {bits:04b}: NC {nc!r} on the device, {want!r} over the checker")
        assert isinstance(nc, float) and abs(nc - want) <= 2e-6 * bin(bits).count("1")
    want_demo = host.calculate_normal_consist(return_demo=True)
    assert demo.shape == want_demo.shape == (2 * S, 4 * S, 4) and np.abs(demo - want_demo).max() <= 1e-6
    assert np.array_equal(demo[:, :, 3], want_demo[:, :, 3])
    want_lst = host.render_mesh_list([host.src_mesh, host.tgt_mesh])
    assert lst.shape == want_lst.shape and np.abs(lst - want_lst).max() <= 1e-6
    want_maps = host.render_normal(torch.from_numpy(v)[None], torch.from_numpy(f)[None])
    for k in ("T_normal_F", "T_normal_B"):
        d = (maps[k].cpu() - want_maps[k]).abs().max().item()
        print(f"{k}: max |difference| {d:.2e}")
        assert maps[k].is_cuda and maps[k].shape == (1, 3, S, S) and d <= 1e-6


def test_gpu_bad_input_raises_before_any_launch():
    from icon_amd.evaluator import IconAmdError, normal_consistency_device
    v, f = _dev(glc.ico(1)[0]), _dev(glc.ico(1)[1])
    with pytest.raises(IconAmdError, match="HIP device"):
        normal_consistency_device(v.cpu(), f.cpu(), v, f)
    with pytest.raises(IconAmdError, match="device"):
        normal_consistency_device(v, f, v, f, normals_a=v.cpu())
    with pytest.raises(IconAmdError, match="shape"):
        normal_consistency_device(v, f, v, f, normals_b=v[:-1])
    with pytest.raises(IconAmdError, match="views"):
        normal_consistency_device(v, f, v, f, degs=range(33))
    with pytest.raises(IconAmdError, match="size"):
        normal_consistency_device(v, f, v, f, size=2049)

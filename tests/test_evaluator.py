"""The evaluator (icon_amd.evaluator) - CPU side.  The numpy statement of the rule the device is compared with
(tests/gl_checker.py) against an independent statement of the coverage in exact rational arithmetic, its watertightness, its
angle-weighted normals against a loop written differently; the reference's OWN Evaluator class, run verbatim over a fake OpenGL
renderer that is the checker, against this module's plumbing over the same checker; and the host contract of the Python and C
entries without a device.  PARITY UNPINNED: neither OpenGL nor trimesh is installed here."""
import ast
import ctypes as C
import math
import os
import sys
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

import gl_checker as glc
from icon_amd import _lib
from icon_amd import evaluator as ev
from icon_amd._lib import IconAmdError
from oracle import ref_loader

S8 = 8


# ---- coverage -------------------------------------------------------------------------------------------------------------
def _covered_rational(x, y, px, py):
    """is the point (px, py) the face's (corners x, y: integers, either winding)?  Independent of the edge functions' tie rule:
    the point moved by (+e, -e^2), e tiny, lies STRICTLY inside - a point on a non-horizontal edge is decided by the step to
    the right (a left edge owns it), one on a horizontal edge by the much smaller step down (a top edge owns it)"""
    e = Fraction(1, 10 ** 9)
    qx, qy = Fraction(px) + e, Fraction(py) - e * e * e
    area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    if area == 0:
        return False
    sgn = 1 if area > 0 else -1
    for a, b in ((0, 1), (1, 2), (2, 0)):
        cross = (x[b] - x[a]) * (qy - y[a]) - (y[b] - y[a]) * (qx - x[a])
        if cross * sgn <= 0:
            return False
    return True


def _coverage_checker(v, face, S):
    """[S,S] bool (window rows): the centres the checker gives the face, depth left out (z = 0)"""
    clip = glc.clip_f32(v, glc.IDENTITY)
    clip[:, 2] = 0
    out = np.zeros((S, S), bool)
    st = glc.face_setup(clip, face, S)
    fr = st and glc.face_fragments(st, clip[:, 2], S)
    if fr:
        out[fr[1], fr[0]] = True
    return out


def _coverage_rational(v, face, S):
    clip = glc.clip_f32(v, glc.IDENTITY)
    x, y = [int(t) for t in glc.snap(clip[face, 0], S)], [int(t) for t in glc.snap(clip[face, 1], S)]
    return np.array([[_covered_rational(x, y, 256 * c + 128, 256 * w + 128) for c in range(S)] for w in range(S)])


@pytest.mark.parametrize("name", list(glc.edge_cases(S8)))
def test_coverage_equals_the_rational_statement(name):
    v, f = glc.edge_cases(S8)[name]
    total = 0
    for face in f:
        got, want = _coverage_checker(v, face, S8), _coverage_rational(v, face, S8)
        assert np.array_equal(got, want), (name, face, np.argwhere(got != want))
        total += int(want.sum())
    print(f"{name}: {total} centres covered")
    if name != "sliver":
        assert total > 0                                                    # zero_area: its second face is a real one
    if name.startswith("axis"):
        # the left edge owns its centres, the bottom edge and the hypotenuse (a right edge) do not: columns 1.., window rows 2..
        want = np.zeros((S8, S8), bool)
        for w in range(2, 6):
            want[w, 1:7 - w] = True
        assert np.array_equal(_coverage_checker(v, f[0], S8), want)


def test_snapped_corners_are_where_the_cases_put_them():
    v, _ = glc.edge_cases(S8)["axis_ccw"]
    assert glc.snap(v[:, 0], S8).tolist() == [384, 1664, 384] and glc.snap(v[:, 1], S8).tolist() == [384, 384, 1664]
    assert glc.snap(np.float32(-1), 2048) == 0 and glc.snap(np.float32(1), 2048) == 256 * 2048
    assert glc.snap(np.float32(2.5 / 1024 - 1), S8) == 2 and glc.snap(np.float32(3.5 / 1024 - 1), S8) == 4      # ties to even


def test_watertight_quad_and_fan():
    v, f = glc.quad(S8)
    count = sum(_coverage_checker(v, face, S8).astype(int) for face in f)
    want = np.zeros((S8, S8), int)
    want[2:7, 1:6] = 1                                                      # left and top edges own their centres, right and bottom do not
    assert np.array_equal(count, want)
    for n in (3, 7, 12):
        v, f = glc.fan(S8, n)
        count = sum(_coverage_checker(v, face, S8).astype(int) for face in f)
        rat = sum(_coverage_rational(v, face, S8).astype(int) for face in f)
        assert np.array_equal(count, rat) and count.max() == 1 and count[4, 3] == 1
        cc, ww = np.meshgrid(np.arange(S8), np.arange(S8))
        inner = np.hypot(cc - 3, ww - 4) * 256 < 900 * math.cos(math.pi / n) - 2
        assert inner.sum() >= 1 and (count[inner] == 1).all()
    # through the renderer: every face of the quad at one depth, the lower id wins nothing it does not own
    v, f = glc.quad(S8)
    _, pix = glc.render(v, f, glc.random_normals(4), *glc.identity_views(), S8)
    assert (pix[0] >= 0).sum() == 25 and np.array_equal(np.flipud(pix[0] >= 0), want.astype(bool))


def test_depth_rule_and_clipping():
    c = lambda i: glc.ndc(256 * i + 128, S8)
    tri = lambda z: [[c(0), c(0), z], [c(7), c(0), z], [c(0), c(7), z]]
    v = np.array(tri(0.0) + tri(0.0) + tri(-0.5) + tri(1.5) + tri(np.float32(-0.0)), np.float32)
    f = np.arange(15).reshape(5, 3)
    n = glc.random_normals(15)
    _, pix = glc.render(v, f[[1, 0]], n, *glc.identity_views(), S8)           # equal depth: the lower id
    assert set(np.unique(pix)) == {-1, 0}
    _, pix = glc.render(v, f[[4, 0]], n, *glc.identity_views(), S8)           # -0 against +0: equal, the lower id
    assert set(np.unique(pix)) == {-1, 0}
    _, pix = glc.render(v, f[[0, 2, 3]], n, *glc.identity_views(), S8)        # clip z = -(-0.5) = 0.5 loses; -1.5 is beyond the near plane
    assert set(np.unique(pix)) == {-1, 0}
    _, pix = glc.render(-v, f[[0, 2]], n, *glc.identity_views(), S8)
    assert set(np.unique(pix)) == {-1, 1}
    rgba, pix = glc.render(v, f[:1], n, *glc.identity_views(), S8)
    assert (rgba[0][pix[0] < 0] == np.float32([1, 1, 1, 0])).all() and (rgba[0][pix[0] >= 0][:, 3] == 1).all()
    assert np.abs(np.linalg.norm(rgba[0][pix[0] >= 0][:, :3] * 2 - 1, axis=1) - 1).max() < 1e-6      # normalised per fragment


# ---- vertex normals -------------------------------------------------------------------------------------------------------------
def _normals_loop(v, f):
    """the same definition written the slow way: per face its unit normal and its three corner angles with numpy's own cross /
    norm / math.acos, added to the corners in face order"""
    v = v.astype(np.float64)
    s = np.zeros((len(v), 3))
    for a, b, c in f:
        if min(a, b, c) < 0 or max(a, b, c) >= len(v):
            continue
        n = np.cross(v[b] - v[a], v[c] - v[a])
        ln = np.linalg.norm(n)
        if not ln > 0:
            continue
        n = n / ln
        for i, (p, q, r) in zip((a, b, c), ((a, b, c), (b, c, a), (c, a, b))):
            u, w = v[q] - v[p], v[r] - v[p]
            s[i] += math.acos(max(-1.0, min(1.0, float(np.dot(u / np.linalg.norm(u), w / np.linalg.norm(w)))))) * n
    ln = np.linalg.norm(s, axis=1, keepdims=True)
    return np.where(ln > 0, s / np.where(ln > 0, ln, 1), 0.0)


@pytest.mark.parametrize("mesh", ["ico", "body", "bad"])
def test_angle_weighted_normals_against_a_loop(mesh):
    v, f = glc.body() if mesh == "body" else glc.ico(2)
    if mesh == "bad":                                                        # a missing vertex, a degenerate face, a lone vertex
        v = np.concatenate([v, [[0.1, 0.2, 0.3]]]).astype(np.float32)
        f = np.concatenate([f, [[0, 1, len(v)], [2, 2, 3], [4, 5, -1]]])
    got, want = glc.vertex_normals(v, f), _normals_loop(v, f)
    d = glc.ulps(got, want.astype(np.float32))
    print(f"{mesh}: {d:.2f} float32 ulps between the checker and the loop, max |diff| to float64 {np.abs(got - want).max():.2e}")
    assert got.dtype == np.float32 and d <= 1.0
    assert np.abs(got - want).max() <= 6e-8                                  # half a float32 ulp below 1
    if mesh == "bad":
        assert (got[-1] == 0).all()


def test_a_sphere_has_radial_normals():
    """the angle-weighted normal of an inscribed mesh is first-order in the edge length away from the sphere's: 4.6e-3, 2.3e-3,
    1.2e-3 at 642, 2,562 and 10,242 vertices - the 40,962-vertex sphere is the first below the bar"""
    v, f = glc.sphere(6, radius=0.7)
    assert np.abs(np.linalg.norm(v, axis=1) - 0.7).max() < 1e-6
    n = glc.vertex_normals(v, f)
    radial = v / np.linalg.norm(v, axis=1, keepdims=True)
    print(f"sphere of {len(v)} vertices: max |normal - radial| = {np.abs(n - radial).max():.2e}")
    assert np.abs(n - radial).max() <= 1e-3
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6


# ---- the views and the error ---------------------------------------------------------------------------------------------
def test_view_matrices_are_formed_in_float64_and_rounded_once():
    m = ev.view_matrices([0, 180, 90, 270, 37.5], scale_factor=0.5, offset=0.25)
    assert m.dtype == np.float32 and m.shape == (5, 3, 4)
    assert m[0].tolist() == [[0.5, 0, 0, 0], [0, 0.5, 0, 0.25], [0, 0, 0.5, 0]]
    for k, deg in enumerate([0, 180, 90, 270, 37.5]):
        a = deg / 180.0 * np.pi
        want = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]) * 0.5
        assert np.array_equal(m[k, :, :3], want.astype(np.float32)), deg
        assert m[k, :, 3].tolist() == [0, 0.25, 0]
    with pytest.raises(IconAmdError, match="finite"):
        ev.view_matrices([0, float("nan")])
    r = ev.euler_to_rot_mat(0.3, -0.4, 0.2)                                   # Rz Ry Rx: x first
    assert np.allclose(r @ r.T, np.eye(3), atol=1e-15) and np.allclose(r, ev.euler_to_rot_mat(0, 0, 0.2) @ ev.euler_to_rot_mat(0, -0.4, 0) @ ev.euler_to_rot_mat(0.3, 0, 0))


def test_error_tree_is_a_sum_and_identical_images_give_zero():
    rs = np.random.RandomState(0)
    for S in (8, 33, 64):
        a, b = rs.rand(S, S, 4).astype(np.float32), rs.rand(S, S, 4).astype(np.float32)
        want = ((a[:, :, :3].astype(np.float64) - b[:, :, :3]) ** 2).sum(2).mean()
        assert abs(glc.view_error(a, b) - want) <= 1e-6 * want                 # each pixel's term is a float32
        assert glc.view_error(a, a) == 0.0
    assert glc.halve(np.arange(5.0), 8) == 10.0 and glc.halve(np.array([1e16, 1.0, -1e16, 1.0]), 4) == 2.0     # (x0 + x2) + (x1 + x3)


# ---- the reference's own Evaluator over the checker ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference_evaluator():
    """lib/dataset/Evaluator.py imported verbatim: ref_loader's stubs, plus a `lib.common.render` that needs no pytorch3d, a
    trimesh.Trimesh stand-in (vertices, faces, the checker's vertex_normals; NO vertex merge) and, in the OpenGL renderer's place,
    a fake whose four methods are the numpy checker.  euler_to_rot_mat is the reference's own function, taken out of
    normal_render.py's syntax tree (the module itself imports OpenGL)"""
    if not ref_loader.available():
        pytest.skip("the reference tree is not present")
    before, was_loaded = dict(sys.modules), ref_loader._loaded is not None
    ref_loader.load()

    class Trimesh:
        def __init__(self, vertices=None, faces=None, **kw):
            self.vertices, self.faces = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)

        @property
        def vertex_normals(self):
            return glc.vertex_normals(self.vertices.astype(np.float32), self.faces).astype(np.float64)

    class Render:
        def __init__(self, size=512, device=None):
            self.size, self.device = size, device

    sys.modules["trimesh"].Trimesh = Trimesh
    stub = types.ModuleType("lib.common.render")
    stub.Render = Render
    sys.modules["lib.common.render"] = stub
    sys.modules.pop("lib.dataset.Evaluator", None)
    import lib.dataset.Evaluator as ref_mod                                 # noqa: E402  (reference module)

    path = os.path.join(ref_loader.REFERENCE_ROOT, "lib", "renderer", "gl", "normal_render.py")
    fn = next(n for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.FunctionDef) and n.name == "euler_to_rot_mat")
    ns = {"np": np, "math": math}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)

    class FakeNormalRender:
        def __init__(self, S):
            self.S = S

        def euler_to_rot_mat(self, r_x, r_y, r_z):
            return ns["euler_to_rot_mat"](self, r_x, r_y, r_z)

        def set_matrices(self, projection, modelview):
            assert np.array_equal(projection, np.diag([1.0, 1.0, -1.0, 1.0])) and np.array_equal(modelview[3], [0, 0, 0, 1])
            self.M = modelview[:3, :4].astype(np.float32)

        def set_normal_mesh(self, vertices, faces, norms, face_normals):
            assert face_normals is faces
            self.mesh = (vertices.astype(np.float32), faces, np.asarray(norms).astype(np.float32))

        def draw(self):
            self.image = glc.render_cached(*self.mesh, self.M, np.ones(3, np.float32), self.S)[0]

        def get_color(self):
            return self.image.copy()

    yield ref_mod, FakeNormalRender
    # leave the process as it was found: the loader's stand-ins for packages that are not installed (kaolin, trimesh, ...) stay in
    # sys.modules for good, and a later test that asks importlib whether such a package exists would meet a module without a spec
    for name in ("lib.dataset.Evaluator", "lib.common.render"):
        sys.modules.pop(name, None)
        if name in before:
            sys.modules[name] = before[name]
    if was_loaded:
        del sys.modules["trimesh"].Trimesh
    else:
        for name, mod in list(sys.modules.items()):
            if name not in before and (getattr(mod, "__spec__", None) is None or name == "lib" or name.startswith("lib.")):
                del sys.modules[name]
        ref_loader._loaded = None                                            # the next load() makes its stand-ins again


def test_the_reference_evaluator_over_the_checker_agrees_with_this_module(reference_evaluator, monkeypatch):
    ref_mod, Fake = reference_evaluator
    S = 32
    monkeypatch.setattr(ref_mod.Evaluator, "_normal_render", Fake(S))
    monkeypatch.setattr(ev, "normal_consistency_device", glc.checker_backend)
    for scale, offset in ((1.0, 0.0), (0.5, 0.125)):
        ref = ref_mod.Evaluator(torch.device("cpu"))
        mine = ev.Evaluator(torch.device("cpu"), size=S)
        assert mine._normal_render is not None and mine.init_gl() is None and mine.offset == ref.offset and mine.scale_factor is ref.scale_factor
        ref.set_mesh({k: (v.clone() if torch.is_tensor(v) else v) for k, v in glc.result_dict().items()}, scale_factor=scale, offset=offset)
        mine.set_mesh(glc.result_dict(), scale_factor=scale, offset=offset)
        ref.space_transfer()
        mine.space_transfer()
        assert mine.verts_pr.numpy().tobytes() == np.asarray(ref.verts_pr, np.float32).tobytes()
        assert np.abs(mine.verts_gt.numpy() - ref.verts_gt).max() <= 2e-7      # a 3 x 3 product: the two libraries may add in another order
        mine.verts_gt = torch.from_numpy(np.asarray(ref.verts_gt, np.float32))  # from here on the same bits go in
        mine.tgt_mesh = ev.EvalMesh(mine.verts_gt, mine.faces_gt)
        for mesh_r, mesh_m in ((ref.src_mesh, mine.src_mesh), (ref.tgt_mesh, mine.tgt_mesh)):
            assert np.array_equal(mesh_r.vertices.astype(np.float32), mesh_m.vertices.numpy()) and np.array_equal(mesh_r.faces, mesh_m.faces.numpy())
        # _render_normal, with and without normals
        for deg in (0, 37.5, 180):
            assert mine._render_normal(mine.src_mesh, deg).numpy().tobytes() == ref._render_normal(ref.src_mesh, deg).tobytes()
        nrm = glc.random_normals(len(ref.tgt_mesh.vertices), 7)
        assert mine._render_normal(mine.tgt_mesh, 90, norms=torch.from_numpy(nrm)).numpy().tobytes() == \
            ref._render_normal(ref.tgt_mesh, 90, norms=nrm.astype(np.float64)).tobytes()
        # calculate_normal_consist: every combination of the four flags, the demo's layout
        worst = 0.0
        for bits in range(16):
            flags = [bool(bits >> i & 1) for i in range(4)]
            want, got = ref.calculate_normal_consist(*flags), mine.calculate_normal_consist(*flags)
            assert isinstance(got, float) or (bits == 0 and got == 0)
            if bits:
                worst = max(worst, abs(got - float(want)) / float(want))
                # the reference sums float32 pairwise, this module float64: log2(S^2) * 2^-24 < 1e-5
                assert float(want) > 1e-3 and abs(got - float(want)) <= 1e-5 * float(want), (flags, got, want)
                demo_r, demo_m = ref.calculate_normal_consist(*flags, return_demo=True), mine.calculate_normal_consist(*flags, return_demo=True)
                assert demo_m.shape == (2 * S, sum(flags) * S, 4) and demo_m.tobytes() == np.ascontiguousarray(demo_r).tobytes()
            else:
                assert want == 0
        print(f"scale {scale}, offset {offset}: NC relative difference to the reference's float32 mean <= {worst:.2e}")
        # render_mesh_list resets scale and offset, like the reference
        lst_r, lst_m = ref.render_mesh_list([ref.src_mesh, ref.tgt_mesh]), mine.render_mesh_list([mine.src_mesh, mine.tgt_mesh])
        assert lst_m.shape == (2 * S, 4 * S, 4) and lst_m.tobytes() == np.ascontiguousarray(lst_r).tobytes()
        assert (mine.offset, mine.scale_factor) == (ref.offset, ref.scale_factor) == (0.0, 1.0)
        # render_normal: [1,V,3] / [1,F,3] in, the two masked maps out
        v, f = torch.from_numpy(glc.ico(2, 0.7)[0])[None], torch.from_numpy(glc.ico(2, 0.7)[1])[None]
        out_r, out_m = ref.render_normal(v, f), mine.render_normal(v, f)
        assert set(out_m) == set(out_r) == {"T_normal_F", "T_normal_B"}
        for k in out_r:
            assert out_m[k].shape == (1, 3, S, S) and out_m[k].dtype == torch.float32 and torch.equal(out_m[k], out_r[k]), k
        assert out_m["T_normal_F"].abs().max() <= 1 and (out_m["T_normal_F"] != 0).any() and not torch.equal(out_m["T_normal_F"], out_m["T_normal_B"])


def test_save_demo_img_writes_the_demo(tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.setattr(ev, "normal_consistency_device", glc.checker_backend)
    mine = ev.Evaluator("cpu", size=16)
    mine.set_mesh(glc.result_dict())
    mine.space_transfer()
    path = str(tmp_path / "demo.png")
    nc = mine.calculate_normal_consist(left=False, right=False, save_demo_img=path)
    demo = mine.calculate_normal_consist(left=False, right=False, return_demo=True)
    assert isinstance(nc, float) and nc > 0
    assert np.array_equal(np.array(Image.open(path)), (demo * 255).astype(np.uint8))
    out = mine.export_mesh(str(tmp_path), "x")
    lines = open(out).read().splitlines()
    nv = len(mine.tgt_mesh.vertices) + len(mine.src_mesh.vertices)
    assert sum(l.startswith("v ") for l in lines) == nv and lines[0].endswith(" 1 0 0") and max(int(t) for l in lines if l.startswith("f ") for t in l.split()[1:]) == nv


def test_calc_acc_equals_the_reference(reference_evaluator):
    ref_mod, _ = reference_evaluator
    ref, mine = ref_mod.Evaluator(torch.device("cpu")), ev.Evaluator("cpu")
    g = torch.Generator().manual_seed(0)
    for use_sdf in (False, True):
        for thres in (0.5, 0.3):
            out = torch.rand(2, 1, 500, generator=g)
            out[0, 0, :20] = thres
            tgt = torch.rand(2, 1, 500, generator=g) if use_sdf else (torch.rand(2, 1, 500, generator=g) > 0.6).float()
            for o, t in ((out, tgt), (torch.zeros_like(out), torch.zeros_like(tgt))):
                a, b = ref.calc_acc(o, t, thres, use_sdf), mine.calc_acc(o, t, thres, use_sdf)
                assert len(a) == len(b) == 4 and all(torch.equal(x, y) for x, y in zip(a, b))


# ---- the host contract ---------------------------------------------------------------------------------------------------
def test_symbols_and_byte_counts_without_a_device():
    assert "icon_normal_consistency_bytes" in _lib.SYMBOLS and "icon_normal_consistency" in _lib.SYMBOLS
    lib = _lib.lib()
    n = C.c_int64(0)
    args = lambda Va, Fa, Vb, Fb, S, K: (C.c_int64(Va), C.c_int64(Fa), C.c_int64(Vb), C.c_int64(Fb), C.c_int(S), C.c_int(K), C.byref(n))
    assert lib.icon_normal_consistency_bytes(*args(100, 200, 0, 0, 64, 4)) == 0
    one = n.value
    assert lib.icon_normal_consistency_bytes(*args(100, 200, 50, 60, 64, 4)) == 0 and n.value > one >= 4 * 64 * 64 * 8
    assert n.value % 256 == 0
    for bad in ((100, 200, 0, 0, 64, 33), (100, 200, 0, 0, 64, 0), (100, 200, 0, 0, 4096, 4), (0, 200, 0, 0, 64, 4), (100, 200, 5, 0, 64, 4)):
        assert lib.icon_normal_consistency_bytes(*args(*bad)) == 1 and b"icon_normal_consistency" in lib.icon_last_error(), bad
    assert lib.icon_normal_consistency_bytes(*args(100, 200, 0, 0, 64, 4)[:-1], None) == 1
    # the call itself refuses bad arguments before it touches the device
    z, p = C.c_void_p(0), C.c_void_p(256)
    call = lambda **kw: lib.icon_normal_consistency(kw.get("va", p), C.c_int64(3), p, C.c_int64(1), C.c_int(0), z, kw.get("vb", z), C.c_int64(kw.get("Vb", 0)),
                                                    kw.get("fb", z), C.c_int64(0), C.c_int(0), z, p, p, C.c_int(kw.get("K", 1)), C.c_int(kw.get("S", 8)),
                                                    kw.get("err", z), z, z, z, z, z, z, kw.get("scratch", p), C.c_int64(kw.get("nbytes", 0)), z)
    assert call(va=z) == 1 and b"null" in lib.icon_last_error()
    assert call(err=p) == 1 and b"single mesh" in lib.icon_last_error()
    assert call(vb=p) == 1 and b"second mesh" in lib.icon_last_error()
    assert call(K=33) == 1 and call(S=4096) == 1
    assert call(scratch=C.c_void_p(260)) == 1 and b"aligned" in lib.icon_last_error()
    assert call() == 1 and b"scratch smaller" in lib.icon_last_error()
    assert lib.icon_debug_set_option(b"ev_lanes", C.c_int(7)) == 1 and lib.icon_debug_set_option(b"ev_lanes", C.c_int(0)) == 0


def test_bad_input_raises_before_any_launch():
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64)
    call = ev.normal_consistency_device
    with pytest.raises(IconAmdError, match="size"):
        call(v, f, v, f, size=4096)
    with pytest.raises(IconAmdError, match="views"):
        call(v, f, v, f, degs=list(range(33)))
    with pytest.raises(IconAmdError, match="views"):
        call(v, f, v, f, degs=[])
    with pytest.raises(IconAmdError, match=r"\[K,3,4\]"):
        call(v, f, v, f, mats=np.zeros((2, 4, 4)))
    with pytest.raises(IconAmdError, match="muls"):
        call(v, f, v, f, muls=np.zeros((3, 3)))
    with pytest.raises(IconAmdError, match=r"\[V,3\]"):
        call(torch.zeros(4, 2), f, v, f)
    with pytest.raises(IconAmdError, match=r"\[F,3\]"):
        call(v, torch.zeros(2, 4, dtype=torch.int64), v, f)
    with pytest.raises(IconAmdError, match="integer"):
        call(v, f.float(), v, f)
    with pytest.raises(IconAmdError, match="both verts and faces"):
        call(v, f, v, None)
    with pytest.raises(IconAmdError, match="normals_b"):
        call(v, f, normals_b=v)
    with pytest.raises(IconAmdError, match="device|normals"):
        call(v, f, v, f, normals_a=torch.zeros(3, 3))                         # CPU tensors (or, with a device, the normals' shape)
    with pytest.raises(IconAmdError):
        call(v, f, v, f)                                                      # host tensors: there is no CPU path

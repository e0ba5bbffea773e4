"""icon_amd.garment on the device - extract_cloth_device / nearest_vertex_device / transfer_labels_device / extract_cloth over
icon_extract_cloth and icon_nearest_vertex (csrc/garment.hip) - against the float64 statement of the rule (tests/garment_oracle.py;
DESIGN.md 4.19, pinned to matplotlib, sklearn and the reference's own function by tests/test_garment.py), by EQUALITY: the
selected set, the nearest index, vert_ids, the face array and the bytes of the output vertices.

The shapes are the smallest at which each kernel can go wrong: polygon lengths around the containment kernel's LDS tile, vertex
and face counts around a workgroup, source counts around the nearest-vertex kernel's tile and its per-wave split.  Every case
but the explicitly degenerate ones asserts, on the ORACLE's side, that between 5 % and 95 % of the vertices are selected, that a
selected vertex is removed by its label and that one is kept (garment_cases.not_vacuous).  Two kinds of case cannot meet all
three and say so where they stand: V = 1 (a single vertex is selected or not) and Vs = 1 (all vertices share one label)."""
import numpy as np
import pytest
import torch

import garment_cases as gc
import garment_oracle as go
from common import assets, golden

pytestmark = pytest.mark.gpu

TRIANGLE = np.array([[-1.0, -0.8], [1.0, -0.7], [0.0, 1.1]])


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _faces_dev(faces, dtype=torch.int64, view=False):
    f = _dev(faces).to(dtype)
    if view:                                                               # the same values behind other strides
        wide = torch.zeros((f.shape[0], 6), dtype=dtype, device=f.device)
        wide[:, ::2] = f
        f = wide[:, ::2]
        assert not f.is_contiguous()
    return f


def _same(out, o):
    """(verts, faces, vert_ids) of the device against the oracle's dict"""
    if o["verts"] is None:
        assert out is None
        return
    assert out is not None
    v, f, ids = out
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and ids.dtype == torch.int32 and v.is_cuda and f.is_cuda and ids.is_cuda
    assert np.array_equal(ids.cpu().numpy(), o["vert_ids"])
    assert np.array_equal(f.cpu().numpy(), o["faces"])
    assert v.cpu().numpy().tobytes() == np.ascontiguousarray(o["verts"], dtype=np.float32).tobytes()


def _check(verts, faces, polys, src=None, rem=None, dtype=torch.int64, view=False, vacuous_ok=False):
    from icon_amd import garment as gm
    o = go.extract(verts, faces, polys, src, rem)
    if not vacuous_ok:
        gc.not_vacuous(o, src is not None)
    v = _dev(verts)
    _same(gm.extract_cloth_device(v, _faces_dev(faces, dtype, view), polys, _dev(src), _dev(rem), return_index=True), o)
    # the selected set on its own: one degenerate face per vertex, no source mesh - vert_ids is then the selection
    every = np.repeat(np.arange(len(verts))[:, None], 3, 1)
    sel = gm.extract_cloth_device(v, _dev(every), polys, return_index=True)
    got = np.zeros(len(verts), dtype=bool)
    if sel is not None:
        got[sel[2].cpu().numpy()] = True
    assert np.array_equal(got, o["selected"])
    if src is not None:                                                    # the nearest index of the selected vertices, -1 elsewhere
        nn = gm.nearest_vertex_device(v, _dev(src), only=_dev(o["selected"]))
        assert nn.dtype == torch.int32 and np.array_equal(nn.cpu().numpy(), o["nn"])
    return o


def _case(seed, V=1000, F=1500, Vs=300, lattice=False):
    rng = np.random.RandomState(seed)
    verts = gc.cloud(rng, V, lattice)
    faces = gc.faces_covering(rng, V, F)
    src, rem = gc.source(rng, verts, Vs)
    return rng, verts, faces, src, rem


# ---- polygons ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, "tile-1", "tile", "tile+1", "2tile+5"])
def test_polygon_lengths(n):
    from icon_amd.garment import POLY_TILE as T
    n = {3: 3, "tile-1": T - 1, "tile": T, "tile+1": T + 1, "2tile+5": 2 * T + 5}[n]
    rng, verts, faces, src, rem = _case(100 + n)
    _check(verts, faces, [TRIANGLE if n == 3 else gc.star_polygon(rng, n)], src, rem)


@pytest.mark.parametrize("count", [1, 2, 5])
def test_polygon_counts(count):
    """overlapping polygons of lengths on both sides of the tile, among them one far from every vertex and one of 2 vertices: any
    polygon selects, the union is what counts"""
    from icon_amd.garment import POLY_TILE as T
    rng, verts, faces, src, rem = _case(200 + count)
    pool = [gc.star_polygon(rng, T + 3, 0.2, 0.7, (-0.3, 0.1)), gc.star_polygon(rng, 40, 0.2, 0.6, (0.2, -0.2)),
            gc.star_polygon(rng, 7, center=(5.0, 5.0)), np.array([[-1.0, -1.0], [1.0, 1.0]]), gc.star_polygon(rng, 2 * T + 1, 0.1, 0.5, (0.6, 0.6))]
    polys = pool[:count]
    o = _check(verts, faces, polys, src, rem)
    if count >= 2:
        a, b = go.contains(polys[0], verts[:, :2]), go.contains(polys[1], verts[:, :2])
        assert (a & b).any() and (a & ~b).any() and (b & ~a).any()          # they do overlap
        assert np.array_equal(o["selected"], go.selected([p for p in polys if len(p) > 2 and p.max() < 4], verts))


def test_lattice_points():
    """vertices on the polygons' corners and edges and at their y values: the comparisons decide, there is no tolerance"""
    rng, verts, faces, src, rem = _case(300, lattice=True)
    for n in (4, 9, 33):
        poly = gc.lattice_polygon(rng, n)
        verts[:n, :2] = poly
        verts[n:2 * n, :2] = 0.5 * (poly + np.roll(poly, -1, 0))
        o = _check(verts, faces, [poly], src, rem)
        assert o["selected"][:2 * n].any() and not o["selected"][:2 * n].all()   # boundary points fall on both sides of the rule


# ---- V and F -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [255, 257, 5000])
@pytest.mark.parametrize("F", [1, 257, 9000])
def test_vertex_and_face_counts(V, F):
    rng, verts, faces, src, rem = _case(400 + V + F, V, F, 300)
    polys = [gc.star_polygon(rng, 50)]
    if F == 1:
        faces[0] = np.nonzero(go.extract(verts, faces, polys, src, rem)["keep_v"])[0][0]     # the one face is a kept one
    _check(verts, faces, polys, src, rem, dtype=torch.int32 if (V + F) % 2 else torch.int64, view=F == 257)
    _check(verts, faces, polys, src, rem, dtype=torch.int64 if (V + F) % 2 else torch.int32, view=F != 257)


def test_both_scans_enter_a_second_round():
    """V = F = SCAN_ROUND + 300: the one-workgroup scan of the block counts takes 8,192 counts of 256 entries per round, so the
    vertices' scan and the faces' scan both carry a total into a second round.  Kept vertices and kept faces lie on both sides of
    entry SCAN_ROUND (the oracle's side): without them the carry would be added to nothing"""
    from icon_amd.garment import SCAN_ROUND as R
    rng = np.random.RandomState(7)
    verts = gc.cloud(rng, R + 300)
    faces = gc.faces_covering(rng, R + 300, R + 300)
    o = _check(verts, faces, [TRIANGLE])
    for kept in (o["vert_ids"], np.nonzero(o["keep_f"])[0]):
        assert (kept < R).any() and (kept >= R).any()


def test_single_vertex():
    """V = 1 cannot meet the 5 % - 95 % condition: the vertex inside (kept / removed by its label) and outside"""
    src = np.array([[0.0, 0.0, 0.0], [2.0, 2.0, 0.0]], np.float32)
    face = np.zeros((1, 3), np.int64)
    for xy, rem, kept in (((0.0, 0.0), (False, True), True), ((0.0, 0.0), (True, False), False), ((3.0, 3.0), (False, False), False)):
        verts = np.array([[xy[0], xy[1], 0.1]], np.float32)
        o = _check(verts, face, [TRIANGLE], src, np.array(rem), vacuous_ok=True)
        assert (o["verts"] is not None) == kept


# ---- the nearest source vertex ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Vs", ["split-1", "split", "split+1", "tile-1", "tile", "tile+1", 6890])
def test_source_counts_and_ties(Vs):
    """source vertices duplicated across the boundaries of the per-wave split and of the LDS tile, queries ON them: the tie goes
    to the lowest index whatever wave or tile holds it"""
    from icon_amd.garment import SRC_SPLIT as S, SRC_TILE as T
    Vs = {"split-1": S - 1, "split": S, "split+1": S + 1, "tile-1": T - 1, "tile": T, "tile+1": T + 1}.get(Vs, Vs)
    rng, verts, faces, src, rem = _case(500 + Vs, 1000, 1500, Vs)
    wanted = [(T - 1, T), (S - 1, S), (S + 1, T + S + 1), (0, Vs - 1), (2 * T - 1, 5 * T), (5 * T + S - 1, 5 * T + S), (7, 13 * T + 100),
              (3, Vs // 2), (S - 4, S - 3)]          # across a tile, across a split, same wave in two tiles, far apart, within one wave
    pairs, used = [], set()
    for a, b in wanted:                                                    # those the source holds, no vertex in two pairs
        if b < Vs and not {a, b} & used:
            pairs.append((a, b))
            used |= {a, b}
    for k, (a, b) in enumerate(pairs):
        src[a, :2] = rng.uniform((-0.3, -0.5), (0.3, 0.2)).astype(np.float32)    # well inside the triangle: every pair's query is selected
        src[b] = src[a]
        rem[b] = not rem[a]                                                # the wrong index would flip the vertex
        verts[k] = src[a]                                                  # a query at distance 0 from both
        verts[100 + k] = src[a] + np.float32(0.001)
    o = _check(verts, faces, [TRIANGLE], src, rem)
    assert o["selected"][:len(pairs)].all() and all(o["nn"][k] == a for k, (a, b) in enumerate(pairs))
    kinds = {"split": any(a // S != b // S and a // T == b // T for a, b in pairs), "tile": any(a // T != b // T for a, b in pairs),
             "wave": any(a // T != b // T and a % T // S == b % T // S for a, b in pairs)}
    assert kinds["split"] == (Vs > S) and kinds["tile"] == (Vs > T) and kinds["wave"] == (Vs > T + S + 1)


def test_single_source_vertex():
    """Vs = 1: every vertex has the one label - all kept or all removed"""
    rng, verts, faces, src, rem = _case(600, 500, 700, 1)
    for flag in (False, True):
        o = _check(verts, faces, [TRIANGLE], src, np.array([flag]), vacuous_ok=True)
        assert 0.05 <= o["selected"].mean() <= 0.95 and (o["verts"] is None) == flag


def test_standalone_nearest_and_labels():
    from icon_amd import garment as gm
    rng, verts, faces, src, rem = _case(700, 3000, 10, 1300)
    want = go.nearest(verts, src)
    nn = gm.nearest_vertex_device(_dev(verts), _dev(src))
    assert nn.dtype == torch.int32 and nn.shape == (3000,) and np.array_equal(nn.cpu().numpy(), want)
    only = rng.uniform(size=3000) < 0.3
    only[64:256] = False                                                   # whole workgroups without a query
    for mask in (_dev(only), _dev(only.astype(np.uint8))):
        got = gm.nearest_vertex_device(_dev(verts), _dev(src), only=mask).cpu().numpy()
        assert np.array_equal(got, np.where(only, want, -1))
    labels = rng.randint(0, 24, 1300)
    for lab in (labels.astype(np.int64), labels.astype(np.int8), labels.astype(np.float32)):
        got = gm.transfer_labels_device(_dev(verts), _dev(src), _dev(lab))
        assert got.dtype == _dev(lab).dtype and np.array_equal(got.cpu().numpy(), lab[want])
    assert gm.nearest_vertex_device(_dev(verts.astype(np.float64)), _dev(src.astype(np.float64))).equal(nn)     # float64 in: rounded first


# ---- nothing, everything, bad faces ------------------------------------------------------------------------------------------
def test_nothing_and_everything():
    from icon_amd import garment as gm
    rng, verts, faces, src, rem = _case(800, 1000, 1500, 300)
    box = np.array([[-2.0, -2.0], [2.0, -2.0], [2.0, 2.0], [-2.0, 2.0]])
    v, f = _dev(verts), _dev(faces)
    assert gm.extract_cloth_device(v, f, [gc.star_polygon(rng, 9, center=(5.0, 5.0))], _dev(src), _dev(rem)) is None      # nothing selected
    assert gm.extract_cloth_device(v, f, []) is None and gm.extract_cloth_device(v, f, [box[:2]]) is None
    assert gm.extract_cloth_device(v, f, [box], _dev(src), _dev(np.ones(300, dtype=bool))) is None                        # everything removed
    for out in (gm.extract_cloth_device(v, f, [box], return_index=True),                                                  # everything kept:
                gm.extract_cloth_device(v, f.int(), [box], _dev(src), _dev(np.zeros(300, dtype=bool)), return_index=True)):   # the mesh comes back
        assert out[0].equal(v) and out[1].equal(f.int()) and out[2].equal(torch.arange(1000, dtype=torch.int32, device="cuda"))
    assert len(gm.extract_cloth_device(v, f, [box])) == 2


def test_bad_face():
    """a face naming a missing vertex is dropped by the device entry (nothing faults, the rest is the oracle's); the host entry
    refuses it before any launch"""
    from icon_amd import garment as gm
    from icon_amd._lib import IconAmdError
    rng, verts, faces, src, rem = _case(900, 1000, 1500, 300)
    inside = np.nonzero(go.extract(verts, faces, [TRIANGLE], src, rem)["keep_v"])[0]
    faces[10] = (inside[0], 1000, inside[1])
    faces[11] = (-1, inside[0], inside[1])
    faces[12] = (inside[0], inside[1], 2 ** 31 + 5)
    o = _check(verts, faces, [TRIANGLE], src, rem)
    assert not o["keep_f"][10:13].any()
    _check(verts, faces[:13], [TRIANGLE], src, rem)                        # the bad faces as the last of the array
    with pytest.raises(IconAmdError, match="face index out of range"):
        gm.extract_cloth((verts, faces), dict(coord_normalized=[TRIANGLE / 50.0], type_id=1), *_infer())


def test_one_device():
    """tensors on the host beside tensors on the device are refused, by both device entries"""
    from icon_amd import garment as gm
    from icon_amd._lib import IconAmdError
    rng, verts, faces, src, rem = _case(950, 100, 150, 30)
    with pytest.raises(IconAmdError, match="must live on one HIP device"):
        gm.extract_cloth_device(torch.from_numpy(verts), _dev(faces), [TRIANGLE])
    with pytest.raises(IconAmdError, match="must live on one HIP device"):
        gm.extract_cloth_device(_dev(verts), _dev(faces), [TRIANGLE], torch.from_numpy(src), _dev(rem))
    with pytest.raises(IconAmdError, match="must live on one HIP device"):
        gm.nearest_vertex_device(_dev(verts), torch.from_numpy(src))


# ---- the sizes of the real call ----------------------------------------------------------------------------------------------
def _infer():
    import test_garment as tg
    return tg.K_INFER, tg.R_INFER, tg.T_INFER


def test_body_size():
    """6,890 source vertices (the synthetic body, parts split into 24 height bands, every other band removed) against 20,000
    vertices of the synthetic subject's 257^3 mesh - the band of the surface around the chest - and a torso polygon: 1.4e8 pairs"""
    from icon_amd.recon import clean_mesh, export_mesh_device
    from test_gpu_parity import make_engine, T
    a = assets("body")
    occ = make_engine(a).eval_slab(T(a.features), 257, 0, 257)
    v, f = clean_mesh(*export_mesh_device(occ, 0.5))
    v = ((v.float() - 128.0) / 128.0).cpu().numpy()
    f = f.cpu().numpy().astype(np.int64)
    pick = np.sort(np.argsort(np.abs(v[:, 1] - 0.15), kind="stable")[:20000])
    remap = np.full(len(v), -1, np.int64)
    remap[pick] = np.arange(len(pick))
    faces = remap[f]
    faces = faces[(faces >= 0).all(1)]
    verts = np.ascontiguousarray(v[pick])
    body = np.ascontiguousarray(a.smpl_verts[0], dtype=np.float32)
    assert body.shape == (6890, 3) and len(verts) == 20000 and len(faces) > 20000
    band = np.clip(((body[:, 1] + 1.0) * 12.0).astype(np.int64), 0, 23)
    torso = np.array([[-0.2, 0.5], [0.0, 0.42], [0.2, 0.5], [0.24, 0.1], [0.18, -0.3], [-0.18, -0.3], [-0.24, 0.1]])
    o = _check(verts, faces, [torso], body, band % 2 == 1, dtype=torch.int32)
    assert o["selected"].sum() > 2000


def test_drop_in_against_the_stored_run(tmp_path):
    """extract_cloth with the matrices of apps/infer.py:576-585 gives what the reference's function gave (tests/golden/
    extract_cloth_ref.npz), from host arrays, mesh objects and device tensors, from the part dict and from (names, labels)"""
    import test_garment as tg
    from icon_amd import garment as gm
    g, lab = golden("extract_cloth_ref.npz"), golden("smpl_part_labels.npz")
    case = tg.stored_case()
    names, labels = [str(n) for n in lab["names"]], lab["labels"]
    table = {n: np.nonzero(labels == k)[0].tolist() for k, n in enumerate(names)}
    K, R, t = _infer()
    for type_id in tg.GOLDEN_TYPES:
        seg = dict(coord_normalized=case["coords"], type_id=type_id)
        runs = [gm.extract_cloth((case["verts"], case["faces"]), seg, K, R, t, (case["body"], case["body_faces"]), (names, labels)),
                gm.extract_cloth(tg._Mesh(_dev(case["verts"]), _dev(case["faces"])), seg, K, R, t, tg._Mesh(case["body"], case["body_faces"]), table)]
        for out in runs:
            assert isinstance(out.vertices, np.ndarray) and out.vertices.tobytes() == g[f"out_verts_{type_id}"].tobytes()
            assert np.array_equal(out.faces, g[f"out_faces_{type_id}"]) and np.array_equal(case["verts"][out.vert_ids], out.vertices)
    path = tmp_path / "garment.obj"
    out.export(str(path))
    lines = path.read_text().split("\n")
    vs = np.array([l.split()[1:] for l in lines if l.startswith("v ")], dtype=np.float64).astype(np.float32)
    fs = np.array([l.split()[1:] for l in lines if l.startswith("f ")], dtype=np.int64)
    assert np.array_equal(vs, out.vertices) and np.array_equal(fs - 1, out.faces)
    # smpl=None: the polygons alone decide (the reference dies there)
    o = go.extract(case["verts"], case["faces"], go.polygons_to_model_plane(case["coords"], K, R, t))
    alone = gm.extract_cloth((case["verts"], case["faces"]), dict(coord_normalized=case["coords"]), K, R, t)
    assert np.array_equal(alone.vert_ids, o["vert_ids"]) and np.array_equal(alone.faces, o["faces"]) and len(alone.faces) > len(out.faces)
    assert gm.extract_cloth((case["verts"], case["faces"]), dict(coord_normalized=[c + 1.0 for c in case["coords"]]), K, R, t) is None


# ---- determinism, streams, the C ABI -------------------------------------------------------------------------------------------
def test_determinism_and_streams():
    from icon_amd import garment as gm
    rng, verts, faces, src, rem = _case(1000, 5000, 9000, 700)
    polys = [gc.star_polygon(rng, 300), gc.star_polygon(rng, 30, 0.2, 0.5, (0.5, 0.5))]
    other = [gc.star_polygon(rng, 300)]
    o, o2 = go.extract(verts, faces, polys, src, rem), go.extract(verts, faces, other, src, rem)
    gc.not_vacuous(o)
    v, f, s, r = _dev(verts), _dev(faces), _dev(src), _dev(rem)
    first = gm.extract_cloth_device(v, f, polys, s, r, return_index=True)
    first = [x.clone() for x in first]
    again = gm.extract_cloth_device(v, f, polys, s, r, return_index=True)
    assert all(a.equal(b) for a, b in zip(first, again))
    _same(again, o)
    from icon_amd import _native
    pool = _native._tls.pool
    before = set(pool)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for st, p in zip(streams, (polys, other)):
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            outs.append(gm.extract_cloth_device(v, f, p, s, r, return_index=True))
    torch.cuda.synchronize()
    new = [k for k in pool if k not in before]
    assert len(new) == 2 and pool[new[0]].data_ptr() != pool[new[1]].data_ptr()       # a scratch per stream
    _same(outs[0], o)
    _same(outs[1], o2)


def test_c_abi_refusals():
    import ctypes as C
    from icon_amd import _lib
    L = _lib.lib()
    n = C.c_int64(0)
    assert L.icon_extract_cloth_bytes(C.c_int64(70000), C.c_int64(140000), C.c_int64(600), C.c_int64(3), C.byref(n)) == 0
    assert 0 < n.value < 70000 * 16 + 140000 * 2 + 8192                      # a few bytes per vertex and face
    assert L.icon_extract_cloth_bytes(C.c_int64(0), C.c_int64(1), C.c_int64(0), C.c_int64(0), C.byref(n)) == 1
    assert L.icon_extract_cloth_bytes(C.c_int64(1), C.c_int64(1), C.c_int64(0), C.c_int64(0), None) == 1
    assert L.icon_nearest_vertex(None, C.c_int64(1), None, C.c_int64(1), None, None, None) == 1 and b"null" in L.icon_last_error()
    v = torch.zeros(8, 3, device="cuda")
    f = torch.zeros(2, 3, dtype=torch.int32, device="cuda")
    xy = torch.zeros(3, 2, dtype=torch.float64, device="cuda")
    off = torch.tensor([0, 3], dtype=torch.int32, device="cuda")
    ov, of, ids = torch.empty_like(v), torch.empty_like(f), torch.empty(8, dtype=torch.int32, device="cuda")
    assert L.icon_extract_cloth_bytes(C.c_int64(8), C.c_int64(2), C.c_int64(3), C.c_int64(1), C.byref(n)) == 0
    scratch = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    hc = (C.c_int64 * 2)()

    def call(nbytes, src=None, Vs=0, rem=None):
        return L.icon_extract_cloth(_lib.ptr(v), C.c_int64(8), _lib.ptr(f), C.c_int64(2), C.c_int(0), _lib.ptr(xy), _lib.ptr(off), C.c_int64(3),
                                    C.c_int64(1), _lib.ptr(src), C.c_int64(Vs), _lib.ptr(rem), _lib.ptr(ov), _lib.ptr(of), _lib.ptr(ids), hc,
                                    _lib.ptr(scratch), C.c_int64(nbytes), None)
    assert call(n.value - 1) == 1 and b"scratch" in L.icon_last_error()
    assert call(n.value, src=v, Vs=8) == 1 and b"go together" in L.icon_last_error()
    assert call(n.value) == 0 and hc[0] == 0 and hc[1] == 0                    # a degenerate polygon selects nothing

"""CPU checker of the evaluator's normal maps and normal consistency (icon_amd.evaluator): the rule of
csrc/raster_gl_device.h restated in numpy - float32 expressions in the order the kernels evaluate them (numpy does not contract),
coverage in exact integers, the error's float64 halving tree - and the meshes its tests run on.  What the device is held to by
equality (images, winners, errors) and to one float32 ulp (the angle-weighted vertex normals: acos differs between libraries).

PARITY UNPINNED, like 4.13: neither OpenGL nor trimesh is installed here.  The rasteriser is restated from the OpenGL
specification (fixed-point snapping, top-left fill rule, GL_LESS), trimesh's vertex_normals FROM MEMORY."""
from functools import lru_cache

import numpy as np

from icon_amd import synth

GUARD = np.float32(64.0)
NEAR_FAR = True          # False (tests only): fragments beyond clip z = -1 / +1 are kept - shows that a case depends on the clipping
F32 = np.float32


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def clip_f32(verts, M):
    """verts [V,3] f32, M [3,4] f32 -> clip coordinates [V,3] f32: p_r = ((M_r0 x + M_r1 y) + M_r2 z) + M_r3, z negated"""
    v, M = np.asarray(verts, F32), np.asarray(M, F32)
    p = np.stack([((M[r, 0] * v[:, 0] + M[r, 1] * v[:, 1]) + M[r, 2] * v[:, 2]) + M[r, 3] for r in range(3)], 1)
    p[:, 2] = -p[:, 2]
    return p.astype(F32)


def cam_normals_f32(normals, M, mul):
    n, M, mul = np.asarray(normals, F32), np.asarray(M, F32), np.asarray(mul, F32)
    return np.stack([((M[r, 0] * n[:, 0] + M[r, 1] * n[:, 1]) + M[r, 2] * n[:, 2]) * mul[r] for r in range(3)], 1).astype(F32)


def snap(x, S):
    """float32 clip coordinate(s) -> int64 1/256-pixel units: rint((x * 0.5 + 0.5) * 256 S) in float64, ties to even"""
    return np.rint((np.asarray(x, np.float64) * 0.5 + 0.5) * float(256 * S)).astype(np.int64)


def face_setup(clip, face, S):
    """-> None (not drawn) or (ids [3] counter-clockwise, x [3], y [3] as Python ints, A2 > 0)"""
    V = len(clip)
    ids = [int(i) for i in face]
    if any(i < 0 or i >= V for i in ids):
        return None
    c = clip[ids]
    if not (np.abs(c[:, :2]) <= GUARD).all():                               # NaN and inf fail too
        return None
    x, y = [int(t) for t in snap(c[:, 0], S)], [int(t) for t in snap(c[:, 1], S)]
    A2 = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    if A2 == 0:
        return None
    if A2 < 0:
        ids, x, y, A2 = [ids[0], ids[2], ids[1]], [x[0], x[2], x[1]], [y[0], y[2], y[1]], -A2
    return ids, x, y, A2


def _edge(ax, ay, bx, by, px, py):
    """the edge function of a -> b on int64 arrays of pixel centres, and the fill rule's verdict"""
    dx, dy = bx - ax, by - ay
    E = dx * (py - ay) - dy * (px - ax)
    return E, (E > 0) | ((E == 0) & (dy < 0 or (dy == 0 and dx < 0)))


def face_fragments(setup, z, S):
    """the pixels a set-up face covers inside the image: (cols, window rows, b [n,3] f32, depth [n] f32), near / far clipped"""
    ids, x, y, A2 = setup
    c0, c1 = max(0, (min(x) + 127) >> 8), min(S - 1, (max(x) - 128) >> 8)
    w0, w1 = max(0, (min(y) + 127) >> 8), min(S - 1, (max(y) - 128) >> 8)
    if c0 > c1 or w0 > w1:
        return None
    cc, ww = np.meshgrid(np.arange(c0, c1 + 1, dtype=np.int64), np.arange(w0, w1 + 1, dtype=np.int64))
    px, py = 256 * cc + 128, 256 * ww + 128
    E0, in0 = _edge(x[1], y[1], x[2], y[2], px, py)
    E1, in1 = _edge(x[2], y[2], x[0], y[0], px, py)
    E2, in2 = _edge(x[0], y[0], x[1], y[1], px, py)
    m = in0 & in1 & in2
    if not m.any():
        return None
    b = np.stack([(E[m].astype(np.float64) / float(A2)).astype(F32) for E in (E0, E1, E2)], 1)
    zz = z[ids]
    with np.errstate(invalid="ignore", over="ignore"):
        d = (b[:, 0] * zz[0] + b[:, 1] * zz[1]) + b[:, 2] * zz[2]
        keep = ((d >= F32(-1.0)) & (d <= F32(1.0))) if NEAR_FAR else (d == d)
    d = np.where(d == 0, F32(0.0), d).astype(F32)                           # -0 and +0 are one depth
    return cc[m][keep], ww[m][keep], b[keep], d[keep]


def render_view(verts, faces, normals, M, mul, S):
    """one view -> rgba [S,S,4] f32 (image orientation), pix [S,S] int32.  Faces are drawn in index order under GL_LESS: a later
    face replaces a pixel only with a strictly smaller depth - the smallest (z, face id) wins"""
    clip = clip_f32(verts, M)
    cn = cam_normals_f32(normals, M, mul)
    depth = np.full((S, S), np.inf, np.float64)
    rgba = np.tile(np.array([1, 1, 1, 0], F32), (S, S, 1))
    pix = np.full((S, S), -1, np.int32)
    # (only to save time: the faces whose pixel box is empty are left out before the loop - face_fragments would return None for them)
    fs = np.asarray(faces, np.int64).reshape(-1, 3)
    inside = ((fs >= 0) & (fs < len(clip))).all(1)
    safe = np.where(np.abs(clip[:, :2]) <= GUARD, clip[:, :2], F32(0))
    sx, sy = snap(safe[:, 0], S)[np.where(inside[:, None], fs, 0)], snap(safe[:, 1], S)[np.where(inside[:, None], fs, 0)]
    boxed = inside & (np.maximum(0, (sx.min(1) + 127) >> 8) <= np.minimum(S - 1, (sx.max(1) - 128) >> 8)) & \
        (np.maximum(0, (sy.min(1) + 127) >> 8) <= np.minimum(S - 1, (sy.max(1) - 128) >> 8))
    for f in np.flatnonzero(boxed):
        face = fs[f]
        st = face_setup(clip, face, S)
        fr = st and face_fragments(st, clip[:, 2], S)
        if not fr:
            continue
        cc, ww, b, d = fr
        rows = S - 1 - ww
        win = d < depth[rows, cc]
        if not win.any():
            continue
        rows, cc, b, d = rows[win], cc[win], b[win], d[win]
        n0, n1, n2 = (cn[i] for i in st[0])
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            c = (b[:, 0:1] * n0 + b[:, 1:2] * n1) + b[:, 2:3] * n2
            ln = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
            rgb = np.where(ln[:, None] == 0, F32(0.5), (c / ln[:, None] + F32(1.0)) * F32(0.5)).astype(F32)
        depth[rows, cc] = d
        rgba[rows, cc, :3] = rgb
        rgba[rows, cc, 3] = 1.0
        pix[rows, cc] = f
    return rgba, pix


def render(verts, faces, normals, mats, muls, S):
    """-> rgba [K,S,S,4] f32, pix [K,S,S] int32; normals None: the angle-weighted ones"""
    if normals is None:
        normals = vertex_normals(verts, faces)
    out = [render_view(verts, faces, normals, M, mul, S) for M, mul in zip(mats, muls)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def halve(x, n):
    """float64 sum of x zero-padded to n (a power of two) by halving: x[i] + x[i + n/2] until one is left"""
    y = np.zeros(n, np.float64)
    y[:len(x)] = x
    while len(y) > 1:
        h = len(y) // 2
        y = y[:h] + y[h:]
    return y[0]


def view_error(a, b):
    """rgba images [S,S,4] f32 of one view -> float64: per pixel ((d0 d0 + d1 d1) + d2 d2) in float32; chunks of 1,024 pixels in
    image order halved in float64; the partial sums halved, zero-padded to 4,096; over S^2"""
    S = a.shape[0]
    d = (a[:, :, :3] - b[:, :, :3]).astype(F32).reshape(-1, 3)
    e = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float64)
    parts = [halve(e[i:i + 1024], 1024) for i in range(0, len(e), 1024)]
    return halve(np.array(parts), 4096) / float(S * S)


def normal_consistency(va, fa, vb, fb, mats, muls, S, na=None, nb=None):
    """-> err [K] f64, (rgba_a, pix_a), (rgba_b, pix_b)"""
    A, B = render(va, fa, na, mats, muls, S), render(vb, fb, nb, mats, muls, S)
    return np.array([view_error(x, y) for x, y in zip(A[0], B[0])]), A, B


def angle_terms(verts, faces):
    """[F,3,3] float64: per face and corner, corner angle x unit face normal; 0 for a face that is degenerate or names a missing
    vertex - in the operation order of csrc/raster_gl_device.h gl_angle_term"""
    v, f = np.asarray(verts, F32).astype(np.float64), np.asarray(faces, np.int64)
    ok = ((f >= 0) & (f < len(v))).all(1)
    fs = np.where(ok[:, None], f, 0)
    p0, p1, p2 = v[fs[:, 0]], v[fs[:, 1]], v[fs[:, 2]]
    e01, e02, e12 = p1 - p0, p2 - p0, p2 - p1
    cr = np.stack([e01[:, 1] * e02[:, 2] - e01[:, 2] * e02[:, 1], e01[:, 2] * e02[:, 0] - e01[:, 0] * e02[:, 2],
                   e01[:, 0] * e02[:, 1] - e01[:, 1] * e02[:, 0]], 1)
    ln = lambda e: np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    L = ln(cr)
    good = ok & (L > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        u01, u02, u12 = e01 / ln(e01)[:, None], e02 / ln(e02)[:, None], e12 / ln(e12)[:, None]
        dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        dots = np.stack([dot(u01, u02), -dot(u01, u12), dot(u02, u12)], 1)
        ang = np.arccos(np.minimum(np.maximum(dots, -1.0), 1.0))
        out = ang[:, :, None] * (cr / L[:, None])[:, None, :]
    out[~good] = 0.0
    return out


def vertex_normals(verts, faces):
    """[V,3] f32: the angle-weighted vertex normals of DESIGN.md 4.20 - the addends of a vertex in ascending 3 face + corner order,
    float64; the sum over its length where that is > 0, else 0; rounded once"""
    V, f = len(verts), np.asarray(faces, np.int64)
    terms = angle_terms(verts, faces).reshape(-1, 3)
    ok = np.repeat(((f >= 0) & (f < V)).all(1), 3)
    keys = np.flatnonzero(ok)                                               # ascending 3 face + corner
    vid = f.reshape(-1)[keys]
    order = np.argsort(vid, kind="stable")                                  # by vertex, keys still ascending inside a vertex
    keys, vid = keys[order], vid[order]
    first = np.flatnonzero(np.r_[True, vid[1:] != vid[:-1]]) if len(vid) else np.zeros(0, np.int64)
    rank = np.arange(len(vid)) - np.repeat(first, np.diff(np.r_[first, len(vid)]))
    s = np.zeros((V, 3), np.float64)
    for r in range(int(rank.max()) + 1 if len(rank) else 0):
        m = rank == r
        s[vid[m]] += terms[keys[m]]                                         # one addend per vertex per round: the order is kept
    ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where((ln > 0)[:, None], s / ln[:, None], 0.0)
    return n.astype(F32)


# ---- meshes -------------------------------------------------------------------------------------------------------------------
def ico(level=2, radius=0.8):
    v, f = synth.icosphere(level, radius=radius)
    return np.ascontiguousarray(v, F32), np.ascontiguousarray(f, np.int64)


def sphere(level=3, radius=0.7):
    """a true sphere about the origin with the icosphere's faces: synth.icosphere's squash and rotation undone"""
    v, f = synth.icosphere(level, radius=1.0, center=(0.0, 0.0, 0.0))
    u = (v.astype(np.float64) @ synth._rotation(np.random.RandomState(7), 11.0)) / np.array([0.7, 1.2, 0.5])
    u = u / np.linalg.norm(u, axis=1, keepdims=True) * radius
    return np.ascontiguousarray(u, F32), np.ascontiguousarray(f, np.int64)


def body():
    a = synth.make_assets("body")
    return np.ascontiguousarray(a.smpl_verts[0], F32), np.ascontiguousarray(a.smpl_faces[0], np.int64)


def ndc(px, S):
    """the clip coordinate that snaps exactly to 1/256-pixel position px (an integer) at size S = 8: exact in float32"""
    return F32(px / (128.0 * S) - 1.0)


def edge_cases(S=8):
    """at S = 8 (a pixel is 1/4 of clip space, 1/256 pixel = 2^-10: every coordinate below is exact in float32): faces whose
    edges and vertices pass exactly through pixel centres.  name -> (verts, faces)"""
    P = lambda *pts: np.array([[ndc(x, S), ndc(y, S), z] for x, y, z in pts], F32)
    c = lambda i: 256 * i + 128                                             # the centre of pixel i
    cases = {
        # an axis-aligned right triangle: its left edge on the centres of column 1, its bottom edge on those of row 1 (a left edge
        # and a bottom edge: one owns its centres, the other does not), its hypotenuse through centres too
        "axis_ccw": (P((c(1), c(1), 0.0), (c(6), c(1), 0.0), (c(1), c(6), 0.0)), [[0, 1, 2]]),
        "axis_cw": (P((c(1), c(1), 0.0), (c(6), c(1), 0.0), (c(1), c(6), 0.0)), [[0, 2, 1]]),
        # top edge on the centres of row 6 and a right edge on column 6
        "top_right": (P((c(6), c(6), 0.25), (c(1), c(6), 0.25), (c(6), c(1), -0.25)), [[0, 1, 2]]),
        # a vertex exactly on a pixel centre, the two faces that share its edges around it
        "vertex": (P((c(3), c(3), 0.0), (c(7), c(2), 0.1), (c(5), c(7), 0.2), (c(0), c(6), 0.3)), [[0, 1, 2], [0, 2, 3]]),
        # a sliver thinner than a pixel that crosses several centres' rows, and a zero-area face (three points on one line)
        "sliver": (P((10, 300, 0.0), (2000, 340, 0.0), (2000, 300, 0.0)), [[0, 1, 2]]),
        "zero_area": (P((c(1), c(1), 0.0), (c(3), c(3), 0.0), (c(5), c(5), 0.0), (c(1), c(5), 0.0)), [[0, 1, 2], [0, 1, 3]]),
    }
    return {k: (v, np.array(f, np.int64)) for k, (v, f) in cases.items()}


def quad(S=8):
    """a grid-aligned quad of two triangles over pixels 1..6: corners ON pixel centres, the diagonal through centres"""
    c = lambda i: 256 * i + 128
    v = np.array([[ndc(c(1), S), ndc(c(1), S), 0], [ndc(c(6), S), ndc(c(1), S), 0], [ndc(c(6), S), ndc(c(6), S), 0],
                  [ndc(c(1), S), ndc(c(6), S), 0]], F32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int64)


def fan(S=8, n=7):
    """n triangles around a hub placed on the centre of pixel (3, 4), rim vertices on 1/256-pixel positions outside the image's core;
    alternating windings"""
    hub = (256 * 3 + 128, 256 * 4 + 128)
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False) + 0.3
    rim = [(int(round(hub[0] + 900 * np.cos(a))), int(round(hub[1] + 900 * np.sin(a)))) for a in ang]
    v = np.array([[ndc(hub[0], S), ndc(hub[1], S), 0.0]] + [[ndc(x, S), ndc(y, S), 0.1 * k] for k, (x, y) in enumerate(rim)], F32)
    f = [[0, 1 + k, 1 + (k + 1) % n] if k % 2 == 0 else [0, 1 + (k + 1) % n, 1 + k] for k in range(n)]
    return v, np.array(f, np.int64)


IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F32)


def identity_views(K=1):
    return np.tile(IDENTITY, (K, 1, 1)), np.ones((K, 3), F32)


def random_normals(V, seed=0):
    n = np.random.RandomState(seed).normal(size=(V, 3))
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)


@lru_cache(maxsize=None)
def body_case(S=64):
    """the 6,890-vertex synthetic body at S = 64 from 0, 180, 90, 270 degrees against a perturbed copy, caller-given normals:
    (va, fa, na, vb, fb, nb, mats, muls, err, A, B)"""
    from icon_amd.evaluator import view_matrices
    va, fa = body()
    vb = (va + np.random.RandomState(1).normal(0, 0.004, va.shape)).astype(F32)
    na, nb = vertex_normals(va, fa), vertex_normals(vb, fa)
    mats, muls = view_matrices([0, 180, 90, 270]), np.ones((4, 3), F32)
    err, A, B = normal_consistency(va, fa, vb, fa, mats, muls, S, na, nb)
    return va, fa, na, vb, fa, nb, mats, muls, err, A, B


# ---- shared by tests/test_evaluator.py and tests/test_gpu_evaluator.py -----------------------------------------------------------
def ulps(a, b):
    """the largest distance of two float32 arrays in units of the last place of the larger magnitude's binade (0 and -0 are one)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    spacing = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return float((np.abs(a.astype(np.float64) - b.astype(np.float64)) / spacing).max())


_cache = {}


def render_cached(v, f, n, M, mul, S):
    v, n, M, mul = (np.ascontiguousarray(x, np.float32) for x in (v, n, M, mul))
    f = np.ascontiguousarray(f, np.int64)
    key = (v.tobytes(), f.tobytes(), n.tobytes(), M.tobytes(), mul.tobytes(), S)
    if key not in _cache:
        _cache[key] = render_view(v, f, n, M, mul, S)
    return _cache[key]


def checker_backend(verts_a, faces_a, verts_b=None, faces_b=None, degs=(0, 180, 90, 270), size=512, *, normals_a=None, normals_b=None,
                     scale_factor=1.0, offset=0.0, mats=None, muls=None, return_images=False, return_faces=False, return_normals=False):
    """normal_consistency_device's signature and results on HOST tensors, computed by the checker"""
    from icon_amd import evaluator as ev
    import torch
    mats, muls = ev._check_views(degs, mats, muls, scale_factor, offset)
    def maps(v, f, n):
        v, f = v.numpy().astype(np.float32), f.numpy()
        n = vertex_normals(v, f) if n is None else n.numpy().astype(np.float32)
        return np.stack([render_cached(v, f, n, M, mul, size)[0] for M, mul in zip(mats, muls)])
    A = maps(verts_a, faces_a, normals_a)
    if verts_b is None:
        return torch.from_numpy(A)
    B = maps(verts_b, faces_b, normals_b)
    err = torch.from_numpy(np.array([view_error(x, y) for x, y in zip(A, B)]))
    return (err, torch.from_numpy(A), torch.from_numpy(B)) if return_images else err


def result_dict():
    """what ICON.test_step hands Evaluator.set_mesh: a prediction in voxel units, a ground truth before its calibration"""
    import torch
    vp, fp = ico(2, radius=0.75)
    vg, fg = ico(1, radius=0.8)
    rs = np.random.RandomState(4)
    vp = vp + rs.normal(0, 0.01, vp.shape).astype(np.float32)
    calib = np.eye(4, dtype=np.float32)
    calib[:3, :3] = np.float32([[0.9, 0.05, 0], [-0.05, 0.9, 0.02], [0, -0.02, 0.95]])
    calib[:3, 3] = np.float32([0.01, -0.02, 0.03])
    return {"verts_pr": torch.from_numpy(((vp + 1) * 128).astype(np.float32)), "faces_pr": torch.from_numpy(fp),
            "verts_gt": torch.from_numpy(vg * np.float32(1.05)), "faces_gt": torch.from_numpy(fg),
            "recon_size": 256, "calib": torch.from_numpy(calib)}

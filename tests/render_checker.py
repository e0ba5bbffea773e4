"""CPU checkers of the forward renderer (icon_amd.render) and the meshes its tests run on.

Two independent statements:

* ``render_f32`` - the rule of DESIGN.md 4.13 in the float32 expressions csrc/render_normal.hip evaluates, in numpy (IEEE
  float32 per operation, no contraction): the device is compared with it for EQUALITY of face ids, depths and colours.
* ``render_blend_f64`` - pytorch3d's published pipeline for the settings lib/common/render.py uses, in float64, sharing no code
  with the first: look_at_view_transform -> FoVOrthographicCameras' projection matrix -> the naive rasteriser (signed squared
  edge distances of every pixel to every face, the 30 nearest candidates by depth) -> softmax_rgb_blend(sigma 1e-4, gamma
  1e-8, background 0.5, znear -256, zfar 256) -> (rgb - 0.5) * 2.
"""
import numpy as np

import color_checker as cc
from common import orc, synth

F32 = np.float32
BLUR = float(np.log(1.0 / 1e-4) * 1e-7)            # RasterizationSettings.blur_radius of Render.init_renderer
BLUR_F32 = F32(BLUR)
BLUR_R_F32 = np.sqrt(BLUR_F32)                     # float32 square root: the bounding box grows by this
EPS_F32 = F32(1e-8)                                # pytorch3d's kEpsilon
CAM_EYES = [(0.0, 0.0, 100.0), (100.0, 0.0, 0.0), (0.0, 0.0, -100.0), (-100.0, 0.0, 0.0)]     # Render.load_meshes


def good_faces(faces, V):
    f = np.asarray(faces, np.int64)
    return ((f >= 0) & (f < V)).all(1)


# ---------------------------------------------------------------------------------------------
# statement 1: the float32 rule
# ---------------------------------------------------------------------------------------------
def _ef(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def _seg(px, py, ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    with np.errstate(all="ignore"):
        t = (dx * (px - ax) + dy * (py - ay)) / l2
    tt = np.minimum(np.maximum(t, F32(0)), F32(1))
    deg = l2 <= EPS_F32
    qx, qy = np.where(deg, bx, ax + tt * dx), np.where(deg, by, ay + tt * dy)
    ex, ey = px - qx, py - qy
    return ex * ex + ey * ey


def _eval_f32(X, Y, D, den, box, px, py):
    """the per-pixel rule (rn_eval): candidate mask, clamped barycentrics, depth.  Everything float32, shapes broadcast."""
    xlo, xhi, ylo, yhi = box
    inbox = (px >= xlo) & (px <= xhi) & (py >= ylo) & (py <= yhi)
    w0 = _ef(px, py, X[1], Y[1], X[2], Y[2]) / den
    w1 = _ef(px, py, X[2], Y[2], X[0], Y[0]) / den
    w2 = _ef(px, py, X[0], Y[0], X[1], Y[1]) / den
    inside = (w0 > 0) & (w1 > 0) & (w2 > 0)
    d01 = _seg(px, py, X[0], Y[0], X[1], Y[1])
    d02 = _seg(px, py, X[0], Y[0], X[2], Y[2])
    d12 = _seg(px, py, X[1], Y[1], X[2], Y[2])
    near = np.minimum(np.minimum(d01, d02), d12) < BLUR_F32
    c0, c1, c2 = (np.maximum(np.minimum(w, F32(1)), F32(0)) for w in (w0, w1, w2))
    s = np.maximum((c0 + c1) + c2, F32(1e-5))
    b0, b1, b2 = c0 / s, c1 / s, c2 / s
    pz = (b0 * D[0] + b1 * D[1]) + b2 * D[2]
    ok = inbox & (inside | near) & ~(pz < 0)
    for a in (w0, b0, pz):
        assert a.dtype == np.float32
    return ok, (b0, b1, b2), pz


def _centre(i, S):
    return F32(-1) + (2 * i + 1).astype(F32) / F32(S)


def _view_f32(v, cam):
    xa, za = (v[:, 2], v[:, 0]) if cam & 1 else (v[:, 0], v[:, 2])
    X = -xa if cam in (0, 3) else xa
    D = F32(100) - za if cam < 2 else F32(100) + za
    return X, v[:, 1], D


def render_f32(verts, faces, cam_ids, S, flip=None):
    """-> pix_to_face [n,S,S] int32, depth [n,S,S] float32, image [n,3,S,S] float32.  Faces naming a missing vertex are skipped;
    the S1 normals are oracle.vertex_normals of the remaining faces (their order is kept, so the sums are the same)."""
    v = np.ascontiguousarray(verts, np.float32)
    f_all = np.asarray(faces, np.int64)
    good = good_faces(f_all, len(v))
    nrm = orc.vertex_normals(v, np.ascontiguousarray(f_all[good]))
    fid = np.nonzero(good)[0]
    f = f_all[good]
    n = len(cam_ids)
    flip = (n == 2) if flip is None else flip
    pix = np.full((n, S, S), -1, np.int32)
    depth = np.full((n, S, S), -1, np.float32)
    image = np.zeros((n, 3, S, S), np.float32)
    fS = F32(S)
    for k, cam in enumerate(cam_ids):
        Xv, Yv, Dv = _view_f32(v, cam)
        X, Y, D = [Xv[f[:, c]] for c in range(3)], [Yv[f[:, c]] for c in range(3)], [Dv[f[:, c]] for c in range(3)]
        area = _ef(X[2], Y[2], X[0], Y[0], X[1], Y[1])
        den = area + EPS_F32
        xlo = np.minimum(X[0], np.minimum(X[1], X[2])) - BLUR_R_F32
        xhi = np.maximum(X[0], np.maximum(X[1], X[2])) + BLUR_R_F32
        ylo = np.minimum(Y[0], np.minimum(Y[1], Y[2])) - BLUR_R_F32
        yhi = np.maximum(Y[0], np.maximum(Y[1], Y[2])) + BLUR_R_F32
        i0 = np.floor(np.minimum(np.maximum((xlo + F32(1)) * F32(0.5) * fS, F32(0)), fS)).astype(np.int64)
        i1 = np.floor(np.minimum(np.maximum((xhi + F32(1)) * F32(0.5) * fS, F32(-1)), fS - F32(1))).astype(np.int64)
        j0 = np.floor(np.minimum(np.maximum((ylo + F32(1)) * F32(0.5) * fS, F32(0)), fS)).astype(np.int64)
        j1 = np.floor(np.minimum(np.maximum((yhi + F32(1)) * F32(0.5) * fS, F32(-1)), fS - F32(1))).astype(np.int64)
        live = (np.abs(area) > EPS_F32) & (i0 <= i1) & (j0 <= j1)
        w, h = i1 - i0 + 1, j1 - j0 + 1
        zb = np.full(S * S, np.iinfo(np.uint64).max, np.uint64)
        side = np.maximum(w, h)
        K = 2
        while live.any():
            K *= 2
            sel_all = np.nonzero(live & (side <= K))[0]
            live[sel_all] = False
            step = max(1, (1 << 21) // (K * K))
            for s0 in range(0, len(sel_all), step):
                sel = sel_all[s0:s0 + step]
                g = np.arange(K)
                i = i0[sel, None, None] + g[None, None, :]                       # mirrored column index
                j = j0[sel, None, None] + g[None, :, None]
                inwin = (g[None, None, :] < w[sel, None, None]) & (g[None, :, None] < h[sel, None, None])
                e = lambda a: a[sel, None, None]
                ok, _, pz = _eval_f32([e(a) for a in X], [e(a) for a in Y], [e(a) for a in D], e(den),
                                      (e(xlo), e(xhi), e(ylo), e(yhi)), _centre(i, S), _centre(j, S))
                ok = ok & inwin
                key = (np.ascontiguousarray(np.broadcast_to(pz, ok.shape)).view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
                    np.broadcast_to(fid[sel, None, None].astype(np.uint64), ok.shape)
                at = np.broadcast_to((S - 1 - j) * S + (S - 1 - i), ok.shape)
                np.minimum.at(zb, at[ok], key[ok])
        hit = np.nonzero(zb != np.iinfo(np.uint64).max)[0]
        win = (zb[hit] & np.uint64(0xffffffff)).astype(np.int64)                 # original face ids
        loc = np.searchsorted(fid, win)                                          # position among the good faces
        row, col = hit // S, hit % S
        g1 = lambda a: a[loc]
        ok, b, pz = _eval_f32([g1(a) for a in X], [g1(a) for a in Y], [g1(a) for a in D], g1(den),
                              (g1(xlo), g1(xhi), g1(ylo), g1(yhi)), _centre(S - 1 - col, S), _centre(S - 1 - row, S))
        assert ok.all() and np.array_equal(pz.view(np.uint32).astype(np.uint64), zb[hit] >> np.uint64(32))
        cs = S - 1 - col if (flip and cam == 2) else col
        pix[k, row, cs] = win
        depth[k, row, cs] = pz
        for ch in range(3):
            t = [(nrm[f[loc, c], ch] + F32(1)) * F32(0.5) for c in range(3)]
            image[k, ch, row, cs] = (((b[0] * t[0] + b[1] * t[1]) + b[2] * t[2]) - F32(0.5)) * F32(2)
    return pix, depth, image


# ---------------------------------------------------------------------------------------------
# statement 2: pytorch3d's pipeline in float64
# ---------------------------------------------------------------------------------------------
def look_at_f64(eye):
    """look_at_view_transform(eye, at=0, up=+y) -> R [3,3], T [3]: view = world @ R + T"""
    eye = np.asarray(eye, np.float64)
    unit = lambda a: a / max(np.linalg.norm(a), 1e-5)
    z_axis = unit(-eye)
    x_axis = unit(np.cross(np.array([0.0, 1.0, 0.0]), z_axis))
    y_axis = unit(np.cross(z_axis, x_axis))
    R = np.stack([x_axis, y_axis, z_axis], 1)
    return R, -(R.T @ eye)


def ortho_matrix_f64(znear=100.0, zfar=-100.0, max_x=100.0, min_x=-100.0, max_y=100.0, min_y=-100.0, scale=100.0):
    K = np.zeros((4, 4))
    K[0, 0] = 2.0 / (max_x - min_x) * scale
    K[1, 1] = 2.0 / (max_y - min_y) * scale
    K[0, 3] = -(max_x + min_x) / (max_x - min_x)
    K[1, 3] = -(max_y + min_y) / (max_y - min_y)
    K[2, 2] = 1.0 / (zfar - znear) * scale
    K[2, 3] = -znear / (zfar - znear)
    K[3, 3] = 1.0
    return K


def project_f64(verts, cam):
    """-> NDC x, NDC y (+x left, +y up), view depth - what MeshRasterizer.transform hands to the rasteriser"""
    R, T = look_at_f64(CAM_EYES[cam])
    view = np.asarray(verts, np.float64) @ R + T
    ndc = np.concatenate([view, np.ones((len(view), 1))], 1) @ ortho_matrix_f64().T
    return ndc[:, 0], ndc[:, 1], view[:, 2]


def vertex_normals_f64(verts, faces):
    v = np.asarray(verts, np.float64)
    fn = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    out = np.zeros_like(v)
    for c in range(3):
        np.add.at(out, faces[:, c], fn)
    return out / np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-6)


def render_blend_f64(verts, faces, cam_ids, S, flip=None, faces_per_pixel=30, sigma=1e-4, gamma=1e-8, background=0.5,
                     znear=-256.0, zfar=256.0, rows_per_chunk=4):
    """-> pix_to_face [n,S,S] int64, depth [n,S,S], image [n,3,S,S], edge_d2 [n,S,S]: the squared distance of each pixel centre
    to the nearest projected edge of any face (float64; what the outlier condition of the tests asks about).
    Every pixel of a chunk of rows is tested against EVERY face whose y extent, grown by a pixel pitch (a thousand blur radii at
    these sizes), meets the chunk - the others cannot be candidates there."""
    faces = np.asarray(faces, np.int64)
    faces = faces[good_faces(faces, len(verts))]
    col = (vertex_normals_f64(verts, faces) + 1.0) * 0.5
    n = len(cam_ids)
    flip = (n == 2) if flip is None else flip
    pix = np.full((n, S, S), -1, np.int64)
    depth = np.full((n, S, S), -1.0)
    image = np.zeros((n, 3, S, S))
    edge_d2 = np.full((n, S, S), np.inf)
    blur_r = np.sqrt(BLUR)
    for k, cam in enumerate(cam_ids):
        x, y, z = project_f64(verts, cam)
        fx, fy, fz = x[faces], y[faces], z[faces]                                 # [F,3]
        area_all = (fx[:, 2] - fx[:, 0]) * (fy[:, 1] - fy[:, 0]) - (fy[:, 2] - fy[:, 0]) * (fx[:, 1] - fx[:, 0])
        for r0 in range(0, S, rows_per_chunk):
            rows = np.arange(r0, min(S, r0 + rows_per_chunk))
            py_rows = 1.0 - (2.0 * rows + 1.0) / S
            pitch = 2.0 / S
            keep = np.nonzero((fy.min(1) - pitch <= py_rows.max()) & (fy.max(1) + pitch >= py_rows.min()) &
                              ~((area_all <= 1e-8) & (area_all >= -1e-8)))[0]
            if not len(keep):
                continue
            px = np.tile(1.0 - (2.0 * np.arange(S) + 1.0) / S, len(rows))[:, None]     # [P,1]
            py = np.repeat(py_rows, S)[:, None]
            X, Y, Z = fx[keep][None], fy[keep][None], fz[keep][None]                   # [1,F',3]
            area = area_all[keep][None] + 1e-8

            def edge(a, b):
                return (px - X[..., a]) * (Y[..., b] - Y[..., a]) - (py - Y[..., a]) * (X[..., b] - X[..., a])
            w = np.stack([edge(1, 2), edge(2, 0), edge(0, 1)], -1) / area[..., None]   # [P,F',3]
            inside = (w > 0).all(-1)

            def seg(a, b):
                dx, dy = X[..., b] - X[..., a], Y[..., b] - Y[..., a]
                l2 = dx * dx + dy * dy
                with np.errstate(all="ignore"):
                    t = np.clip((dx * (px - X[..., a]) + dy * (py - Y[..., a])) / l2, 0.0, 1.0)
                qx, qy = X[..., a] + t * dx, Y[..., a] + t * dy
                d = (px - qx) ** 2 + (py - qy) ** 2
                return np.where(l2 <= 1e-8, (px - X[..., b]) ** 2 + (py - Y[..., b]) ** 2, d)
            dist = np.minimum(np.minimum(seg(0, 1), seg(0, 2)), seg(1, 2))
            edge_d2[k, rows] = dist.min(1).reshape(len(rows), S)
            inbox = (px >= X.min(-1) - blur_r) & (px <= X.max(-1) + blur_r) & (py >= Y.min(-1) - blur_r) & (py <= Y.max(-1) + blur_r)
            wc = np.clip(w, 0.0, 1.0)
            wc = wc / np.maximum(wc.sum(-1, keepdims=True), 1e-5)
            pz = (wc * Z).sum(-1)
            cand = inbox & (inside | (dist < BLUR)) & (pz >= 0)
            pp, ff = np.nonzero(cand)
            if not len(pp):
                continue
            order = np.lexsort((keep[ff], pz[pp, ff], pp))                        # by pixel, then depth, then face id
            pp, ff = pp[order], ff[order]
            first = np.r_[True, pp[1:] != pp[:-1]]
            start = np.nonzero(first)[0]
            rank = np.arange(len(pp)) - np.repeat(start, np.diff(np.r_[start, len(pp)]))
            top = rank < faces_per_pixel
            pp, ff, rank = pp[top], ff[top], rank[top]
            # softmax_rgb_blend
            sd = np.where(inside[pp, ff], -dist[pp, ff], dist[pp, ff])
            prob = 1.0 / (1.0 + np.exp(sd / sigma))
            z_inv = (zfar - pz[pp, ff]) / (zfar - znear)
            P = len(rows) * S
            z_inv_max = np.zeros(P)
            np.maximum.at(z_inv_max, pp, z_inv)
            z_inv_max = np.maximum(z_inv_max, 1e-10)
            wnum = prob * np.exp((z_inv - z_inv_max[pp]) / gamma)
            delta = np.maximum(np.exp((1e-10 - z_inv_max) / gamma), 1e-10)
            denom = np.bincount(pp, wnum, P) + delta
            texel = (wc[pp, ff][:, :, None] * col[faces[keep[ff]]]).sum(1)        # [M,3]
            covered = np.bincount(pp, minlength=P) > 0
            r_out = r0 + np.arange(P) // S
            c_out = np.arange(P) % S
            if flip and cam == 2:
                c_out = S - 1 - c_out
            for ch in range(3):
                rgb = (np.bincount(pp, wnum * texel[:, ch], P) + delta * background) / denom
                image[k, ch, r_out[covered], c_out[covered]] = ((rgb - 0.5) * 2.0)[covered]
            head = rank == 0
            depth[k, r_out[pp[head]], c_out[pp[head]]] = pz[pp[head], ff[head]]
            pix[k, r_out[pp[head]], c_out[pp[head]]] = keep[ff[head]]
        if flip and cam == 2:
            edge_d2[k] = edge_d2[k][:, ::-1]
    return pix, depth, image, edge_d2


# ---------------------------------------------------------------------------------------------
# meshes (the builders of color_checker, plus two of our own)
# ---------------------------------------------------------------------------------------------
def quads():
    """two crossing quads.  A (faces 0, 1: wound in OPPOSITE senses) overhangs the image on every side - its triangles' pixel
    boxes are the whole image: the deferred-face list, and the clipping of a box to the image; B stands in front of part of A for
    camera 0 and cuts through it along x = 0.4175.  Both are tilted, so every camera sees them under an angle."""
    o = 1.3e-3
    # A's triangles do not share vertices: wound in opposite senses, their normals would cancel at a shared vertex
    a = np.array([[-1.3, -1.25, 0.0], [1.3, -1.25, 0.0], [1.3, 1.35, 0.0], [-1.3, -1.25, 0.0], [-1.3, 1.35, 0.0], [1.3, 1.35, 0.0]])
    a[:, 2] = 0.3 * a[:, 0] + 0.1 * a[:, 1]
    b = np.array([[0.05 + o, -0.8 + o, 0.0], [0.9 + o, -0.8 + o, 0.0], [0.9 + o, 0.7 + o, 0.0], [0.05 + o, 0.7 + o, 0.0]])
    b[:, 2] = 0.2505 - 0.3 * b[:, 0] + 0.1 * b[:, 1]
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [6, 8, 9]], np.int64)
    return np.concatenate([a, b]).astype(np.float32), f


def bad_mesh():
    """ico() followed by two zero-area faces and one face naming vertex V: renders as ico() does.  (The zero-area faces repeat their
    FIRST vertex: one of S1's edge vectors is then exactly zero and so is the face's term in the normals.  A face [a, b, b] has
    u x u, which S1's fused multiply-add leaves at a rounding residue - added to the normals by the device and the oracle alike.)"""
    v, f = cc.ico()
    extra = np.array([[5, 5, 9], [7, 8, 7], [0, 1, len(v)]], np.int64)
    return v, np.concatenate([f, extra])


def body():
    return cc.body()


SPHERE_CENTRE, SPHERE_RADIUS = (0.05, -0.1, 0.02), 0.55


def sphere():
    """a TRUE sphere with the level-3 icosphere's faces (synth.icosphere squashes and rotates its own: undone here)"""
    v, f = synth.icosphere(3, radius=1.0, center=(0.0, 0.0, 0.0))
    R = synth._rotation(np.random.RandomState(7), 11.0)
    u = (v.astype(np.float64) @ R) / np.array([0.7, 1.2, 0.5])
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * SPHERE_RADIUS + np.array(SPHERE_CENTRE)).astype(np.float32), f.astype(np.int64)


# name -> (builder, image size, cameras)
CASES = {
    "ico": (cc.ico, 64, (0, 1, 2, 3)),
    "ico_odd": (cc.ico, 63, (0, 1, 2, 3)),
    "ico_offset": (cc.ico_offset, 64, (0, 1, 2, 3)),
    "fan": (cc.fan, 64, (0, 2)),
    "quads": (quads, 32, (0, 1, 2, 3)),
    "body": (body, 128, (0, 2)),
    "bad": (bad_mesh, 64, (0, 2)),
}

_cache = {}


def case(name):
    """-> verts, faces, S, cams, (pix, depth, image) of render_f32 - computed once per process, shared by the tests, never written to"""
    if name not in _cache:
        fn, S, cams = CASES[name]
        v, f = fn()
        out = render_f32(v, f, cams, S)
        for a in out:
            a.setflags(write=False)
        _cache[name] = (v, f, S, cams, out)
    return _cache[name]

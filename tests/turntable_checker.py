"""CPU checker of the turntable renderer (icon_amd.render.render_turntable_device): the rule of 4.13 behind the
projection of a camera at any azimuth, in the float32 expressions csrc/turntable.hip evaluates, in numpy (IEEE float32 per
operation, no contraction).  The device is compared with it for EQUALITY of face ids, depths, colours and frame bytes.  Everything
after the projection is render_checker's (``_ef``, ``_seg``, ``_eval_f32``, ``_centre``, ``good_faces``); tests/test_turntable.py holds
this statement against pytorch3d's pipeline in float64 (render_checker.render_blend_f64) at the same angles."""
import math

import numpy as np

import color_checker as cc
import render_checker as rc
from common import orc

F32 = np.float32
ANGLES = [0, 37, 90, 123.5, 200, 270, 359]


def eye_f64(angle):
    """the reference's camera position at ``angle`` degrees (lib/common/render.py get_rendered_video; mesh_y_center = 0)"""
    return (100.0 * math.cos(np.pi / 180 * angle), 0.0, 100.0 * math.sin(np.pi / 180 * angle))


def project_f32(v, c, s):
    """-> X, Y, D of the float32 vertices ``v`` for the float32 pair (c, s): each product rounded, then subtracted, in this order"""
    c, s = F32(c), F32(s)
    x, z = v[:, 0], v[:, 2]
    X = z * c - x * s
    D = (F32(100) - x * c) - z * s
    assert X.dtype == np.float32 and D.dtype == np.float32
    return X, v[:, 1], D


def frame_bytes(t):
    """t = (n + 1) * 0.5 blended, float32 -> the video's byte: (uint8) min(max(t * 255, 0), 255), truncated"""
    return np.minimum(np.maximum(t * F32(255), F32(0)), F32(255)).astype(np.uint8)


def render_f32(verts, faces, cos_sin, S):
    """-> pix_to_face [n,S,S] int32, depth [n,S,S] float32, image [n,3,S,S] float32, frames [n,S,S,3] uint8 for the float32 pairs
    ``cos_sin [n,2]``.  Faces naming a missing vertex are skipped; the S1 normals are oracle.vertex_normals of the remaining faces."""
    v = np.ascontiguousarray(verts, np.float32)
    f_all = np.asarray(faces, np.int64)
    good = rc.good_faces(f_all, len(v))
    nrm = orc.vertex_normals(v, np.ascontiguousarray(f_all[good]))
    fid = np.nonzero(good)[0]
    f = f_all[good]
    cos_sin = np.asarray(cos_sin, np.float32).reshape(-1, 2)
    n = len(cos_sin)
    pix = np.full((n, S, S), -1, np.int32)
    depth = np.full((n, S, S), -1, np.float32)
    image = np.zeros((n, 3, S, S), np.float32)
    frames = np.full((n, S, S, 3), 127, np.uint8)
    assert frame_bytes(F32(0.5)) == 127
    fS = F32(S)
    R = rc.BLUR_R_F32
    for k, (c, s) in enumerate(cos_sin):
        Xv, Yv, Dv = project_f32(v, c, s)
        X, Y, D = [Xv[f[:, q]] for q in range(3)], [Yv[f[:, q]] for q in range(3)], [Dv[f[:, q]] for q in range(3)]
        area = rc._ef(X[2], Y[2], X[0], Y[0], X[1], Y[1])
        den = area + rc.EPS_F32
        xlo, xhi = np.minimum(X[0], np.minimum(X[1], X[2])) - R, np.maximum(X[0], np.maximum(X[1], X[2])) + R
        ylo, yhi = np.minimum(Y[0], np.minimum(Y[1], Y[2])) - R, np.maximum(Y[0], np.maximum(Y[1], Y[2])) + R
        i0 = np.floor(np.minimum(np.maximum((xlo + F32(1)) * F32(0.5) * fS, F32(0)), fS)).astype(np.int64)
        i1 = np.floor(np.minimum(np.maximum((xhi + F32(1)) * F32(0.5) * fS, F32(-1)), fS - F32(1))).astype(np.int64)
        j0 = np.floor(np.minimum(np.maximum((ylo + F32(1)) * F32(0.5) * fS, F32(0)), fS)).astype(np.int64)
        j1 = np.floor(np.minimum(np.maximum((yhi + F32(1)) * F32(0.5) * fS, F32(-1)), fS - F32(1))).astype(np.int64)
        live = (np.abs(area) > rc.EPS_F32) & (i0 <= i1) & (j0 <= j1)
        w, h = i1 - i0 + 1, j1 - j0 + 1
        zb = np.full(S * S, np.iinfo(np.uint64).max, np.uint64)
        side = np.maximum(w, h)
        K = 2
        while live.any():                                                        # faces by the size of their pixel box: K x K windows
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
                ok, _, pz = rc._eval_f32([e(a) for a in X], [e(a) for a in Y], [e(a) for a in D], e(den),
                                         (e(xlo), e(xhi), e(ylo), e(yhi)), rc._centre(i, S), rc._centre(j, S))
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
        ok, b, pz = rc._eval_f32([g1(a) for a in X], [g1(a) for a in Y], [g1(a) for a in D], g1(den),
                                 (g1(xlo), g1(xhi), g1(ylo), g1(yhi)), rc._centre(S - 1 - col, S), rc._centre(S - 1 - row, S))
        assert ok.all() and np.array_equal(pz.view(np.uint32).astype(np.uint64), zb[hit] >> np.uint64(32))
        pix[k, row, col] = win
        depth[k, row, col] = pz
        for ch in range(3):
            t = [(nrm[f[loc, q], ch] + F32(1)) * F32(0.5) for q in range(3)]
            tx = (b[0] * t[0] + b[1] * t[1]) + b[2] * t[2]
            assert tx.dtype == np.float32
            image[k, ch, row, col] = (tx - F32(0.5)) * F32(2)
            frames[k, row, col, ch] = frame_bytes(tx)
    return pix, depth, image, frames


# name -> (builder, image size); every case is rendered at ANGLES
CASES = {
    "ico": (cc.ico, 64),
    "ico_odd": (cc.ico, 63),
    "fan": (cc.fan, 64),
    "quads": (rc.quads, 32),
    "bad": (rc.bad_mesh, 64),
    "body": (rc.body, 128),
}

_cache = {}


def case(name):
    """-> verts, faces, S, (pix, depth, image, frames) of render_f32 at ANGLES - computed once per process, shared by the tests,
    never written to"""
    if name not in _cache:
        from icon_amd.render import turntable_cos_sin
        fn, S = CASES[name]
        v, f = fn()
        out = render_f32(v, f, turntable_cos_sin(ANGLES), S)
        for a in out:
            a.setflags(write=False)
        _cache[name] = (v, f, S, out)
    return _cache[name]

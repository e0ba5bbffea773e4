"""Oracle of the training rows: numpy and the single-subject oracle (oracle/oracle.py) only, no icon_amd code.

Forward: ``point_feat`` of HGPIFuNet.query (lib/net/HGPIFuNet.py:329-359) for every feature stack of a call - the rows of the
single-subject oracle per subject and stack, the batch-global outlier cmap list applied by its definition exactly as
tests/batch_oracle.py applies it - and the strict ``in_cube`` (:274-275).

Backward: the gradient of the image channels of those rows into the planes.  A point touches the four texels of its bilinear tap
(grid_sample, align_corners=True, zero padding); the weights are the float32 statement the forward uses (``taps``, which
``sample`` pins to the forward oracle's image channels bit for bit); each term is the float32 product weight * grad, accumulated
in float64 by ``np.add.at``; the point's ``feat_select`` half (vis 1 -> front half, lib/dataset/mesh_util.py:266-277) decides
which half of the C planes its channels land in; taps outside the image contribute nothing."""
from __future__ import annotations

import numpy as np

from oracle import oracle as orc
from batch_oracle import project

ALL_FEATS = ("sdf", "norm", "vis", "cmap")
F32 = np.float32


def _dummy_mlp(c0: int) -> orc.Mlp:
    """the oracle's row builders evaluate an MLP on the way: one linear layer of the right width (its output is not used)"""
    return orc.Mlp({"filters.0.weight": np.zeros((1, c0, 1), F32), "filters.0.bias": np.zeros(1, F32)}, res_layers=())


def cin_of(C: int, prior: str, smpl_feats=ALL_FEATS) -> int:
    if prior == "pifu":
        return C + 1
    return (C // 2 if "vis" in smpl_feats else C) + 1 + (3 if "cmap" in smpl_feats else 0) + (3 if "norm" in smpl_feats else 0)


def forward(S, stacks, pts, sdf_clip=0.05, cmap_local=False, smpl_feats=ALL_FEATS, prior="icon"):
    """S: batch_subjects.subjects()-style dict; stacks: list of planes [B,C,H,W]; pts [B,n,3] WORLD points
    -> dict(rows [S,B,Cin,n] f32, in_cube [B,1,n] f32, xyz [B,n,3] f32 projected, half [B,n] int (0: front half),
            outlier [B,n] bool, K: length of the batch-global outlier list)"""
    pts = np.ascontiguousarray(pts, F32)
    B, n = pts.shape[:2]
    Cc = stacks[0].shape[1]
    cin = cin_of(Cc, prior, smpl_feats)
    mlp = _dummy_mlp(cin)
    has_cmap, has_norm, has_vis = "cmap" in smpl_feats, "norm" in smpl_feats, "vis" in smpl_feats
    xyz = np.stack([project(S["calibs"][b], pts[b]) for b in range(B)])
    rows = np.empty((len(stacks), B, cin, n), F32)
    half = np.zeros((B, n), np.int64)
    outlier = np.zeros((B, n), bool)
    signs = []
    if prior == "pifu":
        for s, planes in enumerate(stacks):
            for b in range(B):
                rows[s, b] = orc.query_vol(planes[b], None, mlp, pts[b], calib=S["calibs"][b])[1].T
        K = 0
    else:
        try:
            orc.set_smpl_feats(has_cmap, has_norm, has_vis)
            for b in range(B):
                v, f, cm, vs, cal = S["smpl_verts"][b], S["smpl_faces"][b], S["smpl_cmap"][b], S["smpl_vis"][b], S["calibs"][b]
                for s, planes in enumerate(stacks):
                    rows[s, b] = orc.query_icon(v, f, cm, vs, planes[b], mlp, pts[b], sdf_clip=sdf_clip, calib=cal, cmap_local=True)[1].T
                o = orc.cal_sdf(v, f, cm, vs, xyz[b])
                outlier[b] = np.abs(o["sdf"]) >= F32(sdf_clip)             # the rule itself, float32 (oracle/icon_oracle.c)
                signs.append(np.sign(o["sdf"][outlier[b]]).astype(F32))
                if has_vis:
                    half[b] = (o["vis"] == 0.0).astype(np.int64)          # feat_select: vis 1 -> front half
        finally:
            orc.set_smpl_feats(True, True, True)
        K = int(outlier.sum())
        if has_cmap and not cmap_local and K > 0:
            # smpl_cmap[outlier.repeat(1,1,3)] = smpl_sdf[outlier].repeat(1,1,3) over the subject-major list of the whole batch
            olist = np.concatenate(signs)
            flat = outlier.reshape(-1)
            j = (np.cumsum(flat) - 1)[flat]
            c = cin - 3 - (3 if has_norm else 0)
            bb, pp = np.nonzero(outlier)
            for k in range(3):
                rows[:, bb, c + k, pp] = olist[(3 * j + k) % K][None, :]
    in_cube = ((xyz > -1.0) & (xyz < 1.0)).all(2).astype(F32)[:, None, :]
    return dict(rows=rows, in_cube=in_cube, xyz=xyz, half=half, outlier=outlier, K=K)


def taps(x, y, H: int, W: int, dtype=F32):
    """ATen's grid_sample unnormalisation and corner weights, operation by operation (csrc/common.h: bilinear_taps), in ``dtype``:
    float32 is the statement of the forward and of the device; float64 (from the same float32 coordinates) is what a float64
    grid_sample forms -> x0, y0 (int64, the north-west texel), w [4, ...] (nw, ne, sw, se), inside [4, ...] bool"""
    T = dtype
    x, y = np.asarray(x, F32).astype(T), np.asarray(y, F32).astype(T)
    one, two = T(1.0), T(2.0)
    ix = ((x + one) / two) * T(W - 1)
    iy = ((y + one) / two) * T(H - 1)
    fx, fy = np.floor(ix), np.floor(iy)
    big = T(2.0 ** 30)                                       # (far outside: every tap is outside whatever the integer is)
    x0, y0 = np.clip(fx, -big, big).astype(np.int64), np.clip(fy, -big, big).astype(np.int64)
    x1f, y1f, x0f, y0f = (x0 + 1).astype(T), (y0 + 1).astype(T), x0.astype(T), y0.astype(T)
    w = np.stack([(x1f - ix) * (y1f - iy), (ix - x0f) * (y1f - iy), (x1f - ix) * (iy - y0f), (ix - x0f) * (iy - y0f)]).astype(T)
    bx0, bx1 = (x0 >= 0) & (x0 < W), (x0 + 1 >= 0) & (x0 + 1 < W)
    by0, by1 = (y0 >= 0) & (y0 < H), (y0 + 1 >= 0) & (y0 + 1 < H)
    inside = np.stack([bx0 & by0, bx1 & by0, bx0 & by1, bx1 & by1])
    return x0, y0, w, inside


def sample(planes, xyz, half, csel: int):
    """the image channels of the rows from ``taps`` in the forward's float32 statement ((t00 nw + t01 ne) + t10 sw) + t11 se:
    planes [B,C,H,W], xyz [B,n,3], half [B,n] -> [B,csel,n] f32"""
    B, Cc, H, W = planes.shape
    n = xyz.shape[1]
    out = np.empty((B, csel, n), F32)
    x0, y0, w, inside = taps(xyz[..., 0], xyz[..., 1], H, W)
    for b in range(B):
        ch = half[b][None, :] * csel + np.arange(csel)[:, None]                     # [csel, n] plane of every output channel
        acc = None
        for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            yy, xx = np.clip(y0[b] + dy, 0, H - 1), np.clip(x0[b] + dx, 0, W - 1)
            t = np.where(inside[k, b][None, :], planes[b][ch, yy[None, :], xx[None, :]], F32(0.0)).astype(F32)
            term = (t * w[k, b][None, :]).astype(F32)
            acc = term if acc is None else (acc + term).astype(F32)
        out[b] = acc
    return out


def backward(grad_rows, xyz, half, shape, n_select: int, with_abs: bool = False, dtype=F32):
    """grad_rows [S,B,Cin,n] (the image channels are the first C // n_select), xyz [B,n,3] f32, half [B,n]
    -> grad_planes [S,B,C,H,W] float64 (and, with_abs, sum |w g| per texel [S,B,C,H,W] and the number of terms per texel [B,H,W]).
    ``dtype``: the format of the weights, of grad_rows and of each product (float32: the device's rule; float64: the exact rule)"""
    S, B, Cc, H, W = shape
    csel = Cc // n_select
    n = xyz.shape[1]
    g = np.asarray(grad_rows).astype(dtype)
    out = np.zeros((S, B, Cc, H, W), np.float64)
    mag = np.zeros((S, B, Cc, H, W), np.float64) if with_abs else None
    count = np.zeros((B, H, W), np.int64) if with_abs else None
    x0, y0, w, inside = taps(xyz[..., 0], xyz[..., 1], H, W, dtype)
    for b in range(B):
        for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            m = inside[k, b]
            if not m.any():
                continue
            p = np.nonzero(m)[0]
            yy, xx = y0[b][p] + dy, x0[b][p] + dx
            if with_abs:
                np.add.at(count[b], (yy, xx), 1)
            for s in range(S):
                for c in range(csel):
                    prod = (w[k, b][p] * g[s, b, c, p]).astype(dtype).astype(np.float64)   # the product in ``dtype``
                    cc = half[b][p] * csel + c
                    np.add.at(out[s, b], (cc, yy, xx), prod)
                    if with_abs:
                        np.add.at(mag[s, b], (cc, yy, xx), np.abs(prod))
    return (out, mag, count) if with_abs else out

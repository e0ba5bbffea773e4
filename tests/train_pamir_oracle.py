"""Oracle of the pamir training rows: numpy, tests/train_oracle.py's 2-D functions and the single-subject oracle
(oracle/oracle.py) only, no icon_amd code.

Forward: ``point_feat = cat(index(im_feat, xy), index(vol_feat, xyz))`` of HGPIFuNet.query (lib/net/HGPIFuNet.py:348-359) per pair of
(feature stack, volume) - the rows of the single-subject oracle's pamir branch per subject and stack - and the strict ``in_cube``.

``taps3`` / ``sample3`` restate ATen's grid_sampler_3d (trilinear, zeros padding, align_corners=True) operation by operation, as
csrc/common.h: trilinear_taps states it: x indexes W, y indexes H, z indexes D; corner k = 4 dz + 2 dy + dx (z0 before z1; inside a
z: y0x0, y0x1, y1x0, y1x1); weight (x-term * y-term) * z-term; the sample is the eight products added left to right.

Backward: the gradient of the volume channels of the rows into the volumes.  A point touches the eight voxels of its tap; the weights
are ``taps3``'s in ``dtype``; each term is the product weight * grad in ``dtype``, accumulated in float64 by ``np.add.at``; taps
outside the volume contribute nothing."""
from __future__ import annotations

import numpy as np

import train_oracle as to
from batch_oracle import project
from oracle import oracle as orc

F32 = np.float32
CORNERS = tuple((k >> 2, (k >> 1) & 1, k & 1) for k in range(8))           # (dz, dy, dx) of corner k


def taps3(x, y, z, D: int, H: int, W: int, dtype=F32):
    """-> x0, y0, z0 (int64, the north-west-front voxel), w [8, ...] in corner order, inside [8, ...] bool"""
    T = dtype
    one, two, big = T(1.0), T(2.0), T(2.0 ** 30)
    idx, lo, hi, ok = [], [], [], []
    for v, size in ((x, W), (y, H), (z, D)):
        v = np.asarray(v, F32).astype(T)
        iv = ((v + one) / two) * T(size - 1)
        v0 = np.clip(np.floor(iv), -big, big).astype(np.int64)
        idx.append(v0)
        lo.append(((v0 + 1).astype(T) - iv).astype(T))                       # weight term of the lower corner: (x1 - ix)
        hi.append((iv - v0.astype(T)).astype(T))                             # of the upper corner: (ix - x0)
        ok.append(((v0 >= 0) & (v0 < size), (v0 + 1 >= 0) & (v0 + 1 < size)))
    w, inside = [], []
    for dz, dy, dx in CORNERS:
        wx, wy, wz = (hi[0] if dx else lo[0]), (hi[1] if dy else lo[1]), (hi[2] if dz else lo[2])
        w.append(((wx * wy).astype(T) * wz).astype(T))
        inside.append(ok[0][dx] & ok[1][dy] & ok[2][dz])
    return idx[0], idx[1], idx[2], np.stack(w), np.stack(inside)


def sample3(vols, xyz):
    """the volume channels of the rows in the forward's float32 statement: vols [B,Cv,D,H,W], xyz [B,n,3] -> [B,Cv,n] f32"""
    B, Cv, D, H, W = vols.shape
    x0, y0, z0, w, inside = taps3(xyz[..., 0], xyz[..., 1], xyz[..., 2], D, H, W)
    out = np.empty((B, Cv, xyz.shape[1]), F32)
    for b in range(B):
        acc = None
        for k, (dz, dy, dx) in enumerate(CORNERS):
            zz, yy, xx = np.clip(z0[b] + dz, 0, D - 1), np.clip(y0[b] + dy, 0, H - 1), np.clip(x0[b] + dx, 0, W - 1)
            t = np.where(inside[k, b][None, :], vols[b][:, zz, yy, xx], F32(0.0)).astype(F32)
            term = (t * w[k, b][None, :]).astype(F32)
            acc = term if acc is None else (acc + term).astype(F32)
        out[b] = acc
    return out


def forward(calibs, stacks, vols, pts):
    """calibs [B,4,4]; stacks: list of planes [B,C,H,W]; vols: list of volumes [B,Cv,D,H,W], one per stack; pts [B,n,3] WORLD points
    -> dict(rows [S,B,C+Cv,n] f32 - the single-subject oracle's pamir rows -, in_cube [B,1,n] f32, xyz [B,n,3] f32 projected)"""
    pts = np.ascontiguousarray(pts, F32)
    B, n = pts.shape[:2]
    assert len(stacks) == len(vols)
    cin = stacks[0].shape[1] + vols[0].shape[1]
    mlp = to._dummy_mlp(cin)
    xyz = np.stack([project(calibs[b], pts[b]) for b in range(B)])
    rows = np.empty((len(stacks), B, cin, n), F32)
    for s, (planes, vol) in enumerate(zip(stacks, vols)):
        for b in range(B):
            rows[s, b] = orc.query_vol(planes[b], vol[b], mlp, pts[b], calib=calibs[b])[1].T
    in_cube = ((xyz > -1.0) & (xyz < 1.0)).all(2).astype(F32)[:, None, :]
    return dict(rows=rows, in_cube=in_cube, xyz=xyz)


def backward3(grad_rows, xyz, shape, n_planes: int, with_abs: bool = False, dtype=F32):
    """grad_rows [S,B,Cin,n] (the volume channels are n_planes .. n_planes + Cv - 1), xyz [B,n,3] f32, shape (S,B,Cv,D,H,W)
    -> grad_vols float64 (and, with_abs, sum |w g| per voxel [S,B,Cv,D,H,W] and the number of terms per voxel [B,D,H,W])"""
    S, B, Cv, D, H, W = shape
    g = np.asarray(grad_rows).astype(dtype)
    out = np.zeros(shape, np.float64)
    mag = np.zeros(shape, np.float64) if with_abs else None
    count = np.zeros((B, D, H, W), np.int64) if with_abs else None
    x0, y0, z0, w, inside = taps3(xyz[..., 0], xyz[..., 1], xyz[..., 2], D, H, W, dtype)
    for b in range(B):
        for k, (dz, dy, dx) in enumerate(CORNERS):
            p = np.nonzero(inside[k, b])[0]
            if not len(p):
                continue
            zz, yy, xx = z0[b][p] + dz, y0[b][p] + dy, x0[b][p] + dx
            if with_abs:
                np.add.at(count[b], (zz, yy, xx), 1)
            for s in range(S):
                for c in range(Cv):
                    prod = (w[k, b][p] * g[s, b, n_planes + c, p]).astype(dtype).astype(np.float64)     # the product in ``dtype``
                    np.add.at(out[s, b, c], (zz, yy, xx), prod)
                    if with_abs:
                        np.add.at(mag[s, b, c], (zz, yy, xx), np.abs(prod))
    return (out, mag, count) if with_abs else out

"""A float64 oracle for the batched query() contract (HGPIFuNet.query at B > 1, lib/net/HGPIFuNet.py:268-367), assembled from
the single-subject oracle (oracle/oracle.py) and numpy only: no icon_amd code and no torch operator touches the data.

Per subject the single-subject oracle gives the MLP input rows under the per-point cmap rule and the sdf of every point;
the batch-global outlier list (:303-305) is then applied by its definition.  tests/test_batch_oracle.py pins the result to
the reference's own batched run (tests/golden/query_batch_outputs.npz) and, at B = 1, to orc.query_icon bit for bit."""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import oracle as orc

ALL_FEATS = ("sdf", "norm", "vis", "cmap")


def project(calib, pts) -> np.ndarray:
    """orthogonal() as the oracle computes it (orc_project): world points [n,3] -> projected [n,3] float32"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    cal = np.ascontiguousarray(np.asarray(calib, np.float32).reshape(-1, 4)[:3])
    xyz = np.empty_like(pts)
    orc.lib().orc_project(cal.ctypes.data_as(C.c_void_p), pts.ctypes.data_as(C.c_void_p), C.c_int64(len(pts)), xyz.ctypes.data_as(C.c_void_p))
    return xyz


def batch_query_icon(S, planes, mlp, pts, sdf_clip, cmap_local, subset=None, smpl_feats=ALL_FEATS):
    """S: batch_subjects.subjects()-style dict of [B,...] arrays; planes [B,C,H,W]; mlp: orc.Mlp; pts [B,n,3] WORLD points;
    subset: indices into the subject-major call order 0 .. B*n (None: every point).
    -> (occ [B,n], or [len(subset)] in the subset's order; K: length of the batch-global outlier list; outliers per subject [B])"""
    pts = np.ascontiguousarray(pts, np.float32)
    B, n = pts.shape[:2]
    idx = np.arange(B * n, dtype=np.int64) if subset is None else np.asarray(subset, np.int64).reshape(-1)
    clip = np.float32(sdf_clip)
    has_cmap, has_norm = "cmap" in smpl_feats, "norm" in smpl_feats
    X, xyz_sel, signs, outlier = [None] * B, [None] * B, [], []
    where = [np.nonzero(idx // n == b)[0] for b in range(B)]          # rows of the result that subject b fills
    try:
        orc.set_smpl_feats(has_cmap, has_norm, "vis" in smpl_feats)
        for b in range(B):
            v, f, cm, vs, K = S["smpl_verts"][b], S["smpl_faces"][b], S["smpl_cmap"][b], S["smpl_vis"][b], S["calibs"][b]
            local = idx[where[b]] - b * n
            _, X[b] = orc.query_icon_subset(v, f, cm, vs, planes[b], mlp, pts[b], local, sdf_clip=sdf_clip, calib=K, cmap_local=True)
            xyz = project(K, pts[b])
            sdf = orc.cal_sdf(v, f, cm, vs, xyz)["sdf"]
            out = np.abs(sdf) >= clip                                  # the rule itself (oracle/icon_oracle.c:572), float32
            outlier.append(out)
            signs.append(np.sign(sdf[out]).astype(np.float32))        # +1 / -1 / 0
            xyz_sel[b] = xyz[local]
    finally:
        orc.set_smpl_feats(True, True, True)
    counts = np.array([int(o.sum()) for o in outlier], np.int64)
    K = int(counts.sum())
    rows = np.empty((len(idx), X[0].shape[1]), np.float32)
    xyz = np.empty((len(idx), 3), np.float32)
    for b in range(B):
        rows[where[b]], xyz[where[b]] = X[b], xyz_sel[b]
    if has_cmap and not cmap_local and K > 0:
        # smpl_cmap[outlier.repeat(1,1,3)] = smpl_sdf[outlier].repeat(1,1,3): the list of ALL subjects' outlier signs, subject-major,
        # tiled three times and consumed row-major - the outlier of global rank j gets olist[(3j + k) % K] in cmap channel k
        olist = np.concatenate(signs)
        flat = np.concatenate(outlier)
        rank = np.cumsum(flat) - 1                                     # global rank of an outlier at its call position
        c = rows.shape[1] - 3 - (3 if has_norm else 0)                 # [img | sdf | cmap r g b | norm x y z]
        hit = flat[idx]
        j = rank[idx][hit]
        for k in range(3):
            rows[hit, c + k] = olist[(3 * j + k) % K]
    occ = mlp.forward(rows, f64=True)[:, 0]
    in_cube = ((xyz > -1.0) & (xyz < 1.0)).all(1).astype(np.float32)   # strict (HGPIFuNet.py:274-275,363)
    occ = in_cube * occ
    return (occ.reshape(B, n) if subset is None else occ), K, counts

"""The garment-extraction rule in plain numpy float64 - what icon_amd.garment's native calls are held to, by
EQUALITY.  tests/test_garment.py pins this statement to matplotlib's Path.contains_points, to sklearn's 1-nearest-neighbour
classifier and to the reference's own extract_cloth; tests/test_gpu_garment.py compares the device with it.

Written independently of icon_amd/garment.py: nothing is imported from the package."""
import numpy as np

BASE = ("rightHand", "leftToeBase", "leftFoot", "rightFoot", "head", "leftHandIndex1", "rightHandIndex1", "rightToeBase", "leftHand",
        "rightHand")
FOREARMS, ARMS, LEGS = ("leftForeArm", "rightForeArm"), ("leftArm", "rightArm"), ("leftLeg", "rightLeg")
EXTRA = {1: FOREARMS, 3: FOREARMS, 10: FOREARMS, 7: LEGS + FOREARMS + ARMS}
EXTRA.update({k: FOREARMS + ARMS for k in (5, 6, 8, 9, 12, 13)})


def parts_to_remove(type_id):
    return list(BASE + EXTRA.get(type_id, ()))


def part_labels(vert_segmentation, n_verts):
    """later keys overwrite earlier ones, as the reference's y[val] = key does"""
    names = list(vert_segmentation)
    labels = np.full(n_verts, -1, np.int32)
    for k, name in enumerate(names):
        labels[np.asarray(vert_segmentation[name], dtype=np.int64)] = k
    assert (labels >= 0).all()
    return names, labels


def polygons_to_model_plane(coord_normalized, K, R, t):
    ext = np.zeros((3, 4))
    ext[:3, :3] = R
    ext[:, 3] = t
    P_inv = np.linalg.pinv(np.asarray(K)[:3, :3] @ ext)
    out = []
    for polygon in coord_normalized:
        polygon = np.asarray(polygon, dtype=np.float64)
        h = np.hstack((polygon, np.ones((len(polygon), 1))))
        X = (P_inv @ h[:, :, None]).reshape(len(polygon), 4)
        out.append((X[:, :3] / X[:, 3, None])[:, :2])
    return out


def contains(poly, pts):
    """rule 2: poly [n,2], pts [N,2] (any float type, widened) -> bool [N]"""
    poly, pts = np.asarray(poly, dtype=np.float64).reshape(-1, 2), np.asarray(pts).astype(np.float64)
    odd = np.zeros(len(pts), dtype=bool)
    n = len(poly)
    if n < 3:
        return odd
    tx, ty = pts[:, 0], pts[:, 1]
    for e in range(n):
        (x0, y0), (x1, y1) = poly[e], poly[(e + 1) % n]
        f0, f1 = y0 >= ty, y1 >= ty
        odd ^= (f0 != f1) & ((((y1 - ty) * (x0 - x1)) >= ((x1 - tx) * (y0 - y1))) == f1)
    return odd


def selected(polygons, verts):
    sel = np.zeros(len(verts), dtype=bool)
    for p in polygons:
        sel |= contains(p, np.asarray(verts)[:, :2])
    return sel


def nearest(verts, src, chunk=512):
    """rule 3: the lowest j minimising ((dx*dx + dy*dy) + dz*dz) in float64 -> int64 [V]"""
    q, s = np.asarray(verts).astype(np.float64), np.asarray(src).astype(np.float64)
    out = np.empty(len(q), np.int64)
    for a in range(0, len(q), chunk):
        d = q[a:a + chunk, None, :] - s[None, :, :]
        d *= d
        out[a:a + chunk] = ((d[:, :, 0] + d[:, :, 1]) + d[:, :, 2]).argmin(1)          # argmin: the first of equal minima
    return out


def extract(verts, faces, polygons, src=None, src_remove=None):
    """rules 2-6 -> dict(selected, nn, keep_v, keep_f, verts, faces, vert_ids); verts / faces / vert_ids are None when no face is
    kept.  nn is -1 where the vertex is not selected (its label cannot matter) and None without a source mesh."""
    verts, faces = np.asarray(verts), np.asarray(faces).astype(np.int64)
    V = len(verts)
    sel = selected(polygons, verts)
    nn = None
    keep_v = sel.copy()
    if src is not None:
        nn = np.full(V, -1, np.int64)
        if sel.any():
            nn[sel] = nearest(verts[sel], src)
        keep_v[sel] = ~np.asarray(src_remove).astype(bool)[nn[sel]]
    ok = ((faces >= 0) & (faces < V)).all(1)
    keep_f = np.zeros(len(faces), dtype=bool)
    keep_f[ok] = keep_v[faces[ok]].any(1)
    out = dict(selected=sel, nn=nn, keep_v=keep_v, keep_f=keep_f, verts=None, faces=None, vert_ids=None)
    if keep_f.any():
        kept = faces[keep_f]
        ids = np.unique(kept)                                                 # ascending
        remap = np.full(V, -1, np.int64)
        remap[ids] = np.arange(len(ids))
        out.update(verts=verts[ids], faces=remap[kept].astype(np.int32), vert_ids=ids.astype(np.int32))
    return out

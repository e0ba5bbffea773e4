"""Deterministic batches of subjects for the batched query() (tests/test_gpu_batch_query.py, tools/make_golden_batch.py).

Every subject is the synthetic body (icon_amd.synth, "body") under its own rotation, scale and translation, with its own
smpl_vis / smpl_cmap (recomputed from the moved vertices), its own feature planes and its own non-identity calibration.
The faces are shared, as SMPL's are (check_sign takes subject 0's faces for every subject, lib/dataset/mesh_util.py:393)."""
from __future__ import annotations

import hashlib

import numpy as np

from icon_amd import synth

B_GOLDEN, N_GOLDEN = 4, 8000
# variants of the fixtures: (smpl_feats, plane channels, plane size, stacks, prior)
VARIANTS = {
    "full": (("sdf", "norm", "vis", "cmap"), 12, 128, 2, "icon"),     # icon-filter / icon-nofilter (num_stack 2)
    "sdf": (("sdf",), 6, 128, 1, "icon"),                             # icon-mvp smpl_feats
    "nofilter": (("sdf", "norm", "vis", "cmap"), 6, 512, 1, "icon"),  # use_filter False: raw normal maps at image size
    "pifu": ((), 6, 128, 1, "pifu"),
}


def _rot(axis: int, a: float) -> np.ndarray:
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def subjects(B: int = B_GOLDEN, seed: int = 0) -> dict:
    """smpl_feat_dict arrays [B,...] (verts f32, faces i64, cmap f32, vis f32), calibs [B,4,4] f32 and the derivation
    parameters [B,9] (rotation y, x, scale, translation xyz, calibration rotation z, scale, z shift)"""
    a = synth.make_assets("body")
    v0 = a.smpl_verts[0].astype(np.float64)
    f = a.smpl_faces[0]
    c = 0.5 * (v0.min(0) + v0.max(0))
    rng = np.random.RandomState(seed + 4242)
    verts, vis, cmap, calibs, params = [], [], [], [], []
    for _ in range(B):
        ay, ax, s = rng.uniform(-0.6, 0.6), rng.uniform(-0.2, 0.2), rng.uniform(0.85, 1.05)
        t = rng.uniform(-0.06, 0.06, 3)
        cz, cs, ct = rng.uniform(-0.15, 0.15), rng.uniform(0.9, 1.1), rng.uniform(-0.05, 0.05)
        v = (((v0 - c) @ (_rot(1, ay) @ _rot(0, ax)).T) * s + c + t).astype(np.float32)
        vs, cm = synth.make_vis_cmap(v, f)
        K = np.eye(4)
        K[:3, :3] = cs * _rot(2, cz)
        K[:3, 3] = [0.5 * ct, -0.5 * ct, ct]
        verts.append(v); vis.append(vs); cmap.append(cm); calibs.append(K.astype(np.float32))
        params.append([ay, ax, s, *t, cz, cs, ct])
    return dict(smpl_verts=np.stack(verts), smpl_faces=np.repeat(f[None], B, 0), smpl_cmap=np.stack(cmap),
                smpl_vis=np.stack(vis), calibs=np.stack(calibs), params=np.asarray(params, np.float64))


def planes(B: int, channels: int, size: int, stack: int = 0) -> np.ndarray:
    """[B, channels, size, size] f32: subject b's planes of feature stack `stack`"""
    return np.concatenate([synth.make_feature_planes(channels, size, synth.SEED + 97 * b + 1009 * stack) for b in range(B)])


def state_dict(variant: str) -> dict:
    feats, C, _, _, prior = VARIANTS[variant]
    if variant == "full":
        return synth.make_assets("body").state_dict
    if prior == "pifu":
        return synth.make_mlp_state_dict(synth.SEED + 7, dims=(C + 1, 512, 256, 128, 1), sdf_channel=None)
    img = C // 2 if "vis" in feats else C
    c0 = img + 1 + (3 if "cmap" in feats else 0) + (3 if "norm" in feats else 0)
    return synth.make_mlp_state_dict(synth.SEED + 5 + len(feats), dims=(c0, 512, 256, 128, 1))


def candidate_points(S: dict, n: int, seed: int = 0) -> np.ndarray:
    """[B, n, 3] f32 WORLD points of every subject: near its surface (drawn in the projected space the mesh lives in, mapped
    back through the inverse calibration), far field, and outside the cube"""
    out = []
    for b in range(S["smpl_verts"].shape[0]):
        K = S["calibs"][b].astype(np.float64)
        rng = np.random.RandomState(seed + 31 * b + 7)
        xyz = synth.stratified_points(S["smpl_verts"][b], S["smpl_faces"][b], n - n // 8, seed=seed + 13 * b).astype(np.float64)
        xyz = np.concatenate([xyz, rng.uniform(-1.4, 1.4, (n - len(xyz), 3))])
        world = (xyz - K[:3, 3]) @ np.linalg.inv(K[:3, :3]).T
        out.append(world[rng.permutation(n)].astype(np.float32))
    return np.stack(out)


def sha1(*arrays) -> str:
    h = hashlib.sha1()
    for x in arrays:
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()

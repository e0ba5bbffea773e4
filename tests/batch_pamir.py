"""Deterministic PaMIR batches for the batched query() (tests/test_gpu_batch_pamir.py, tools/make_golden_batch_pamir.py).

Every subject is the tetrahedralised synthetic body (icon_amd.synth.make_tetra_body: surface vertices, then one interior vertex)
under its own rotation, scale and translation about the body's centre, kept inside the [-0.5,0.5] cube the voxeliser samples.
The tetrahedra are shared, as SMPL's are, and so is the surface code table (smpl_vertex_code).  Every subject has its own
feature planes [6,128,128] (regenerated from seeds) and its own non-identity calibration.  The padded tensors carry pad counts
that differ across subjects: the reference strips every subject with subject 0's (lib/net/HGPIFuNet.py:316-319)."""
from __future__ import annotations

import numpy as np

from batch_subjects import _rot, sha1
from icon_amd import synth

B_GOLDEN, N_GOLDEN = 4, 8000
PAD_V = (5, 7, 5, 3)                # voxel_verts / voxel_faces padding per subject (entries 1.. are ignored by the reference)
PAD_F = (9, 4, 9, 6)
PLANES_C, PLANES_SIZE = 6, 128      # hourglass_dim 6 (configs/train/pamir.yaml)
VOL_RES, SIGMA = 128, 0.05          # lib/net/HGPIFuNet.py:109-118


def tetra_body():
    """(voxel_verts [V,3], voxel_tets [T,4], vertex_code [Vs,3]) of the unmoved synthetic body"""
    a = synth.make_assets("body", prior_type="pamir")
    return synth.make_tetra_body(a.smpl_verts[0], a.smpl_faces[0], a.smpl_cmap[0])


def subjects(B: int = B_GOLDEN, seed: int = 0) -> dict:
    """verts [B,V,3] f32 (unpadded), tets [T,4] i64, code [Vs,3] f32, calibs [B,4,4] f32, params [B,9] f64 (rotation y, x,
    scale, translation xyz, calibration rotation z, scale, z shift)"""
    vv, tets, code = tetra_body()
    v0 = vv.astype(np.float64)
    c = 0.5 * (v0.min(0) + v0.max(0))
    rng = np.random.RandomState(seed + 5151)
    verts, calibs, params = [], [], []
    for _ in range(B):
        ay, ax, s = rng.uniform(-0.6, 0.6), rng.uniform(-0.2, 0.2), rng.uniform(0.8, 0.95)
        t = rng.uniform(-0.04, 0.04, 3)
        cz, cs, ct = rng.uniform(-0.15, 0.15), rng.uniform(0.9, 1.1), rng.uniform(-0.05, 0.05)
        v = (((v0 - c) @ (_rot(1, ay) @ _rot(0, ax)).T) * s + c + t).astype(np.float32)
        assert np.abs(v).max() < 0.5, "a subject leaves the voxeliser's [-0.5,0.5] cube"
        K = np.eye(4)
        K[:3, :3] = cs * _rot(2, cz)
        K[:3, 3] = [0.5 * ct, -0.5 * ct, ct]
        verts.append(v); calibs.append(K.astype(np.float32))
        params.append([ay, ax, s, *t, cz, cs, ct])
    return dict(verts=np.stack(verts), tets=tets, code=code, calibs=np.stack(calibs), params=np.asarray(params, np.float64))


def padded(S: dict, pad_v=PAD_V, pad_f=PAD_F) -> dict:
    """smpl_feat_dict arrays as a batch delivers them: every subject padded to a common length with subject 0's count (zeros),
    pad_v_num / pad_f_num [B] int64 as given"""
    B = S["verts"].shape[0]
    vv = np.concatenate([S["verts"], np.zeros((B, pad_v[0], 3), np.float32)], 1)
    tets = np.concatenate([S["tets"], np.zeros((pad_f[0], 4), np.int64)])
    return dict(voxel_verts=vv, voxel_faces=np.repeat(tets[None], B, 0), pad_v_num=np.asarray(pad_v[:B], np.int64),
                pad_f_num=np.asarray(pad_f[:B], np.int64))


def planes(B: int) -> np.ndarray:
    """[B,6,128,128] f32: subject b's image feature planes"""
    return np.concatenate([synth.make_feature_planes(PLANES_C, PLANES_SIZE, synth.SEED + 577 * b + 3) for b in range(B)])


def state_dict() -> dict:
    """the pamir regressor: [img(6) | vol(7)] -> 1 (the B = 1 fixture's, tools/make_golden.py section j)"""
    return synth.make_mlp_state_dict(synth.SEED + 1, sdf_channel=None)


def candidate_points(S: dict, n: int, seed: int = 0) -> np.ndarray:
    """[B, n, 3] f32 WORLD points: drawn in the projected space (uniform over [-1.05,1.05]^3, and a quarter near the body's
    box), mapped back through subject b's inverse calibration"""
    out = []
    for b in range(S["calibs"].shape[0]):
        K = S["calibs"][b].astype(np.float64)
        rng = np.random.RandomState(seed + 37 * b + 11)
        xyz = np.concatenate([rng.uniform(-1.05, 1.05, (n - n // 4, 3)), rng.uniform(-0.55, 0.55, (n // 4, 3))])
        world = (xyz - K[:3, 3]) @ np.linalg.inv(K[:3, :3]).T
        out.append(world[rng.permutation(n)].astype(np.float32))
    return np.stack(out)


def subjects_sha1(S: dict) -> str:
    return sha1(S["verts"], S["tets"], S["code"], S["calibs"], planes(S["verts"].shape[0]))

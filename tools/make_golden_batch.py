#!/usr/bin/env python3
"""Reference fixtures of the batched query() (tests/golden/query_batch_inputs.npz, query_batch_outputs.npz).

The reference's own HGPIFuNet.query (lib/net/HGPIFuNet.py:268-367) at B = 4 subjects x N = 8,000 points (tests/batch_subjects.py),
loaded through oracle/ref_loader.  The loader binds kaolin's two leaves to oracle restatements that take one subject; here
they are rebound - in THIS process only - to loops over the subjects of the same oracle.Accel leaves (check_sign with
subject 0's faces for every subject, as the reference passes them: lib/dataset/mesh_util.py:393).

Points whose result would hang on one float32 ulp - | |sdf| - sdf_clip | < 1e-5 (the outlier flag flips, and with it the
batch-global cmap tiling of every later subject) or a projected coordinate within 1e-6 of +-1 (in_cube) - are redrawn.

usage: python tools/make_golden_batch.py [--check]   (--check: regenerate in memory and compare with the committed files)"""
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_subjects as bs  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SDF_CLIP = 0.05


@contextlib.contextmanager
def reference():
    """the reference modules with the two kaolin leaves taking [B, ...] (per-subject loops over oracle.Accel) for the duration
    of the block - the loader's own leaves are restored after it (other users of ref_loader in the process see no change)"""
    ref = ref_loader.load()
    mu = ref.mesh_util

    def point_to_mesh_distance(points, triangles):
        d2s, idxs = [], []
        for b in range(points.shape[0]):
            verts = triangles[b].detach().cpu().numpy().astype(np.float32).reshape(-1, 3)
            faces = np.arange(len(verts), dtype=np.int64).reshape(-1, 3)
            d2, idx = orc.Accel(verts, faces).nearest(points[b].detach().cpu().numpy())
            d2s.append(torch.from_numpy(d2)); idxs.append(torch.from_numpy(idx))
        return torch.stack(d2s), torch.stack(idxs), torch.zeros(points.shape[0], points.shape[1], dtype=torch.int32)

    def check_sign(verts, faces, points, hash_resolution=512):
        f = faces.detach().cpu().numpy()
        return torch.stack([torch.from_numpy(orc.Accel(verts[b].detach().cpu().numpy(), f).check_sign(points[b].detach().cpu().numpy()))
                            for b in range(verts.shape[0])])

    saved = (mu.point_to_mesh_distance, mu.check_sign)
    mu.point_to_mesh_distance, mu.check_sign = point_to_mesh_distance, check_sign
    try:
        yield ref
    finally:
        mu.point_to_mesh_distance, mu.check_sign = saved


def projected(points, calibs):
    """orthogonal() as the reference computes it (torch.baddbmm on CPU float32): [B,3,N]"""
    p, K = torch.from_numpy(points), torch.from_numpy(calibs)
    return torch.baddbmm(K[:, :3, 3:4], K[:, :3, :3], p).numpy()


def draw_points(S, n, seed=0):
    """[B,3,n] world points with no ulp-sensitive point; returns (points, redrawn count)"""
    B = S["smpl_verts"].shape[0]
    keep = [np.zeros((0, 3), np.float32) for _ in range(B)]
    redrawn, rnd = 0, 0
    while min(len(k) for k in keep) < n:
        cand = bs.candidate_points(S, n, seed + 1000 * rnd)                       # [B,n,3]
        xyz = projected(cand.transpose(0, 2, 1).copy(), S["calibs"])               # [B,3,n]
        for b in range(B):
            q = xyz[b].T
            d2, _ = orc.Accel(S["smpl_verts"][b], S["smpl_faces"][0]).nearest(np.ascontiguousarray(q))
            sdf = np.sqrt(d2.astype(np.float32)) / np.sqrt(np.float32(3.0))
            ok = (np.abs(sdf - SDF_CLIP) >= 1e-5) & (np.abs(np.abs(q) - 1.0) >= 1e-6).all(1)
            redrawn += int((~ok).sum())
            keep[b] = np.concatenate([keep[b], cand[b][ok]])[:n]
        rnd += 1
    return np.stack(keep).transpose(0, 2, 1).copy(), redrawn


def run_reference(ref, S, points, variant, subjects=None):
    """HGPIFuNet.query of the reference on the batch (or on the listed subjects only) -> [stacks][B',1,N]"""
    feats, C, size, stacks, prior = bs.VARIANTS[variant]
    sel = list(range(points.shape[0])) if subjects is None else list(subjects)
    B = S["smpl_verts"].shape[0]
    a = bs.synth.make_assets("body")
    netG, cfg = ref_loader.build_netG(a)
    c0 = bs.state_dict(variant)["filters.0.weight"].shape[1]
    netG.if_regressor = ref.MLP(filter_channels=[c0, 512, 256, 128, 1], name="if", res_layers=[2, 3, 4], norm="batch", last_op=None).eval()
    missing, unexpected = netG.if_regressor.load_state_dict({k: torch.from_numpy(v) for k, v in bs.state_dict(variant).items()}, strict=False)
    assert not unexpected and all("num_batches_tracked" in m for m in missing), (missing, unexpected)
    netG.prior_type = prior
    netG.smpl_feats = list(feats)
    netG.smpl_feat_dict = {k: torch.from_numpy(np.ascontiguousarray(S[k][sel])) for k in ("smpl_verts", "smpl_faces", "smpl_cmap", "smpl_vis")}
    features = [torch.from_numpy(bs.planes(B, C, size, k)[sel]) for k in range(stacks)]
    with torch.no_grad():
        out = netG.query(features=features, points=torch.from_numpy(np.ascontiguousarray(points[sel])),
                         calibs=torch.from_numpy(np.ascontiguousarray(S["calibs"][sel])), regressor=netG.if_regressor)
    return [o.numpy() for o in out]


def generate():
    with reference() as ref:
        return _generate(ref)


def _generate(ref):
    S = bs.subjects(bs.B_GOLDEN)
    points, redrawn = draw_points(S, bs.N_GOLDEN)
    print(f"points: {points.shape}, {redrawn} candidates redrawn (|sdf| within 1e-5 of the clip or a coordinate within 1e-6 of +-1)")
    planes_sha = bs.sha1(*[bs.planes(bs.B_GOLDEN, C, size, k) for _, C, size, stacks, _ in bs.VARIANTS.values() for k in range(stacks)])
    inp = dict(points=points, calibs=S["calibs"], params=S["params"], sdf_clip=np.float32(SDF_CLIP),
               sha1_subjects=np.array(bs.sha1(S["smpl_verts"], S["smpl_vis"], S["smpl_cmap"], S["calibs"])), sha1_planes=np.array(planes_sha))
    out = {}
    for variant in bs.VARIANTS:
        for k, o in enumerate(run_reference(ref, S, points, variant)):
            out[f"occ_{variant}_{k}"] = o.astype(np.float32)
            print(f"{variant} stack {k}: occ {o.min():.4f} .. {o.max():.4f}")
    return inp, out


def main():
    inp, out = generate()
    if "--check" in sys.argv:
        for name, d in (("query_batch_inputs.npz", inp), ("query_batch_outputs.npz", out)):
            g = np.load(os.path.join(OUT, name))
            for k, v in d.items():
                assert np.array_equal(g[k], v), (name, k)
        print("fixtures reproduced")
        return
    np.savez_compressed(os.path.join(OUT, "query_batch_inputs.npz"), **inp)
    np.savez_compressed(os.path.join(OUT, "query_batch_outputs.npz"), **out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Reference fixture of the batched query() with the pamir prior (tests/golden/query_batch_pamir.npz).

The reference's own HGPIFuNet(prior_type="pamir").query (lib/net/HGPIFuNet.py:268-367) on CPU at B = 4 subjects x N = 8,000 points
(tests/batch_pamir.py), built by tools/make_golden.py:pamir_reference_net: its Voxelization wrapper (lib/net/voxelize.py:64-137) and
its VolumeEncoder (lib/net/VE.py:114-183) as they are.  The voxelize_cuda leaf that function installs takes one subject; here it is
rebound - in THIS process only - to a loop over the subjects of the same oracle voxeliser (orc.semantic_voxelize), which receives
the tetrahedra as positions [B,T,4,3] exactly as the wheel does.  Everything between - the padding strip with subject 0's counts,
update_param with subject 0's tetrahedra, vertices_to_tetrahedrons, the tiled code table, the permute, ve(vol,
intermediate_output=False), index(vol_feat, xyz) - is reference code.

Stored: points [4,3,8000], calibs, pads, occ [4,1,8000], the encoder's state dict (ve.*), vol_feat[:, :, ::4, ::4, ::4] and the hash
of the derived subjects (planes regenerated from seeds, not stored).  Points with a projected coordinate within 1e-6 of +-1 (in_cube
hangs on one ulp there) are redrawn.

usage: python tools/make_golden_batch_pamir.py [--check]   (--check: regenerate in memory and compare with the committed file)"""
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import batch_pamir as bp  # noqa: E402
from icon_amd import synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "query_batch_pamir.npz")


def batch_leaf(smpl_vertices, smpl_vertex_code, smpl_tetrahedrons, occ_volume, semantic_volume, weight_sum_volume, sigma):
    """voxelize_cuda.forward_semantic_voxelization at any batch size (wheel signature, lib/net/voxelize.py:57-59): surface vertices
    [B,Vs,3], their codes [B,Vs,3], tetrahedra as POSITIONS [B,T,4,3] -> semantic_volume [B,res,res,res,3], one subject at a time"""
    res = semantic_volume.shape[1]
    for b in range(smpl_vertices.shape[0]):
        vs = smpl_vertices[b].numpy().astype(np.float32)
        tp = smpl_tetrahedrons[b].numpy().astype(np.float32).reshape(-1, 3)
        allv = np.concatenate([vs, tp], 0)
        tidx = (len(vs) + np.arange(len(tp), dtype=np.int64)).reshape(-1, 4)
        out = orc.semantic_voxelize(allv, len(vs), smpl_vertex_code[b].numpy().astype(np.float32), tidx, res=res, sigma=float(sigma))
        semantic_volume[b].copy_(torch.from_numpy(out))
    return occ_volume, semantic_volume, weight_sum_volume


@contextlib.contextmanager
def reference_net():
    """(netG, ref) - the reference pamir network with the B-aware leaf for the duration of the block"""
    import make_golden as mg
    from oracle import ref_loader
    a = synth.make_assets("body", prior_type="pamir")
    netG, _, _ = mg.pamir_reference_net(a)
    missing, unexpected = netG.if_regressor.load_state_dict({k: torch.from_numpy(v) for k, v in bp.state_dict().items()}, strict=False)
    assert not unexpected and all("num_batches_tracked" in m for m in missing), (missing, unexpected)
    mod = sys.modules["voxelize_cuda"]
    saved = mod.forward_semantic_voxelization
    mod.forward_semantic_voxelization = batch_leaf
    try:
        yield netG, ref_loader.load()
    finally:
        mod.forward_semantic_voxelization = saved


def projected(points, calibs):
    """orthogonal() as the reference computes it (torch.baddbmm on CPU float32): [B,3,N]"""
    p, K = torch.from_numpy(points), torch.from_numpy(calibs)
    return torch.baddbmm(K[:, :3, 3:4], K[:, :3, :3], p).numpy()


def draw_points(S, n, seed=0):
    """[B,3,n] world points, none with a projected coordinate within 1e-6 of +-1; returns (points, redrawn count)"""
    B = S["calibs"].shape[0]
    keep = [np.zeros((0, 3), np.float32) for _ in range(B)]
    redrawn, rnd = 0, 0
    while min(len(k) for k in keep) < n:
        cand = bp.candidate_points(S, n, seed + 1000 * rnd)
        xyz = projected(cand.transpose(0, 2, 1).copy(), S["calibs"])
        for b in range(B):
            ok = (np.abs(np.abs(xyz[b].T) - 1.0) >= 1e-6).all(1)
            redrawn += int((~ok).sum())
            keep[b] = np.concatenate([keep[b], cand[b][ok]])[:n]
        rnd += 1
    return np.stack(keep).transpose(0, 2, 1).copy(), redrawn


def run_reference(netG, S, points, d=None):
    """HGPIFuNet.query of the reference on the batch -> (occ [B,1,N], vol_feat [B,Cv,32,32,32]); `d` overrides smpl_feat_dict arrays"""
    B = points.shape[0]
    d = d if d is not None else bp.padded(S)
    netG.smpl_feat_dict = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}
    with torch.no_grad():
        occ = netG.query(features=[torch.from_numpy(bp.planes(B))], points=torch.from_numpy(np.ascontiguousarray(points)),
                         calibs=torch.from_numpy(np.ascontiguousarray(S["calibs"])), regressor=netG.if_regressor)
        assert len(occ) == 1
        # what query() fed the regressor's volume half (HGPIFuNet.py:316-325), recomputed from the same tensors
        vv = netG.smpl_feat_dict["voxel_verts"][:, :-netG.smpl_feat_dict["pad_v_num"][0], :]
        vf = netG.smpl_feat_dict["voxel_faces"][:, :-netG.smpl_feat_dict["pad_f_num"][0], :]
        netG.voxelization.update_param(batch_size=vf.shape[0], smpl_tetra=vf[0].detach().cpu().numpy())
        vol_feat = netG.ve(netG.voxelization(vv), intermediate_output=False)[-1]
    return occ[0].numpy(), vol_feat.numpy()


def generate():
    S = bp.subjects(bp.B_GOLDEN)
    points, redrawn = draw_points(S, bp.N_GOLDEN)
    print(f"points: {points.shape}, {redrawn} candidates redrawn (a projected coordinate within 1e-6 of +-1)")
    with reference_net() as (netG, _):
        occ, vol_feat = run_reference(netG, S, points)
        ve_sd = {"ve." + k: v.numpy() for k, v in netG.ve.state_dict().items() if "num_batches_tracked" not in k}
    print(f"occ {occ.min():.4f} .. {occ.max():.4f}, vol_feat |max| {np.abs(vol_feat).max():.3f}")
    return dict(points=points, calibs=S["calibs"], params=S["params"], pad_v_num=np.asarray(bp.PAD_V, np.int64),
                pad_f_num=np.asarray(bp.PAD_F, np.int64), occ=occ.astype(np.float32),
                vol_feat_sample=np.ascontiguousarray(vol_feat[:, :, ::4, ::4, ::4]).astype(np.float32),
                sha1_subjects=np.array(bp.subjects_sha1(S)), **ve_sd)


def main():
    out = generate()
    if "--check" in sys.argv:
        g = np.load(OUT)
        assert sorted(g.files) == sorted(out)
        for k, v in out.items():
            assert np.array_equal(g[k], v), k
        print("fixture reproduced")
        return
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

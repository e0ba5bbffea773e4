#!/usr/bin/env python3
"""ms per batched pamir query() stage at B subjects x N points (default 8 x 8,000: configs/train/pamir.yaml's batch_size and
num_sample_geo) against a loop of B single-subject calls, split as HGPIFuNet.query's pamir branch runs (lib/net/HGPIFuNet.py:314-354):
  voxelise - the semantic volume at 128^3 (semantic_voxelization_batch: one launch per kernel over the B subjects; loop:
             semantic_voxelization per subject),
  encode   - ve(vol, intermediate_output=False)[-1] on PyTorch-ROCm (the VolumeEncoder layer list, tests/common.py), [B,3,128^3] in
             one call against B calls of [1,3,128^3],
  query    - the feature + MLP call with the volumes bound (one icon_query_points_batch against B icon_query_points).
Prints one JSON line.   usage: python tools/time_query_batch_pamir.py [--B 8] [--N 8000] [--reps R]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_pamir as bp  # noqa: E402
from common import volume_encoder_replica  # noqa: E402
from icon_amd.engine import IconQueryEngine, semantic_voxelization, semantic_voxelization_batch  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return round(t0.elapsed_time(t1) / reps, 4)


def main():
    B, n, reps = arg("--B", 8), arg("--N", 8000), arg("--reps", 10)
    dev = torch.device("cuda:0")
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    S = bp.subjects(B)
    vv, tets, code = T(S["verts"]), T(S["tets"]), S["code"]
    torch.manual_seed(0)
    ve = volume_encoder_replica().eval().to(dev)
    planes, calibs = T(bp.planes(B)), T(S["calibs"])
    pts = T(bp.candidate_points(S, n).transpose(0, 2, 1))
    sd = {k: torch.from_numpy(v) for k, v in bp.state_dict().items()}
    with torch.no_grad():
        vol = semantic_voxelization_batch(vv, tets, code, res=bp.VOL_RES, sigma=bp.SIGMA)
        vfeat = ve(vol.contiguous(), intermediate_output=False)[-1]
    batch = IconQueryEngine(prior_type="pamir")
    batch.set_regressor(sd)
    batch.set_volume_features(vfeat)
    singles = []
    for b in range(B):
        e = IconQueryEngine(prior_type="pamir")
        e.set_regressor(sd)
        e.set_volume_features(vfeat[b:b + 1])
        singles.append((e, [planes[b:b + 1]], pts[b:b + 1].contiguous(), calibs[b:b + 1]))
    vols1 = [semantic_voxelization(vv[b:b + 1], tets[None], code, res=bp.VOL_RES, sigma=bp.SIGMA) for b in range(B)]

    def enc(x):
        with torch.no_grad():
            return ve(x, intermediate_output=False)[-1]

    res = {
        "voxelise_batched_ms": timed(lambda: semantic_voxelization_batch(vv, tets, code, res=bp.VOL_RES, sigma=bp.SIGMA), reps),
        "voxelise_loop_ms": timed(lambda: [semantic_voxelization(vv[b:b + 1], tets[None], code, res=bp.VOL_RES, sigma=bp.SIGMA) for b in range(B)], reps),
        "encode_batched_ms": timed(lambda: enc(vol), reps),
        "encode_loop_ms": timed(lambda: [enc(v) for v in vols1], reps),
        "query_batched_ms": timed(lambda: batch.query([planes], pts, calibs), reps),
        "query_loop_ms": timed(lambda: [e.query(f, p, c) for e, f, p, c in singles], reps),
    }
    for k in ("voxelise", "encode", "query"):
        res[f"{k}_speedup"] = round(res[f"{k}_loop_ms"] / res[f"{k}_batched_ms"], 2)
    res["total_batched_ms"] = round(sum(res[f"{k}_batched_ms"] for k in ("voxelise", "encode", "query")), 4)
    res["total_loop_ms"] = round(sum(res[f"{k}_loop_ms"] for k in ("voxelise", "encode", "query")), 4)
    print(json.dumps({"time_query_batch_pamir": dict(B=B, N=n, res=bp.VOL_RES, reps=reps, **res)}))


if __name__ == "__main__":
    main()

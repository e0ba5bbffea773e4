#!/usr/bin/env python3
"""ms per batched query() (one call, B subjects, 2 feature stacks) against a loop of B single-subject calls, meshes and planes
prebuilt (warm caches), for B in {1, 4, 12} x N in {8,000, 100,000} points per subject.  Prints one JSON line.
usage: python tools/time_query_batch.py [--reps R]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_subjects as bs  # noqa: E402
from icon_amd.engine import IconQueryEngine  # noqa: E402


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
    dev = torch.device("cuda:0")
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    sd = {k: torch.from_numpy(v) for k, v in bs.state_dict("full").items()}
    S = bs.subjects(12)
    planes = [T(bs.planes(12, 12, 128, k)) for k in range(2)]
    rows = []
    for B in (1, 4, 12):
        for n in (8000, 100000):
            pts = T(bs.candidate_points({k: v[:B] for k, v in S.items()}, n).transpose(0, 2, 1))
            calibs = T(S["calibs"][:B])
            feats = [p[:B].contiguous() for p in planes]
            batch = IconQueryEngine(prior_type="icon", sdf_clip=0.05)
            batch.set_mesh(*(T(S[k][:B]) for k in ("smpl_verts", "smpl_faces", "smpl_cmap", "smpl_vis")))
            batch.set_regressor(sd)
            singles = []
            for b in range(B):
                e = IconQueryEngine(prior_type="icon", sdf_clip=0.05)
                e.set_mesh(*(T(S[k][b:b + 1]) for k in ("smpl_verts", "smpl_faces", "smpl_cmap", "smpl_vis")))
                e.set_regressor(sd)
                singles.append((e, [f[b:b + 1].contiguous() for f in feats], pts[b:b + 1].contiguous(), calibs[b:b + 1]))

            def run_batch():
                return batch.query(feats, pts, calibs)

            def run_loop():
                return [e.query(f, p, c) for e, f, p, c in singles]

            res = {}
            for name, fn in (("batched_ms", run_batch), ("loop_ms", run_loop)):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(reps):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                res[name] = round(t0.elapsed_time(t1) / reps, 4)
            rows.append(dict(B=B, N=n, stacks=2, **res, speedup=round(res["loop_ms"] / res["batched_ms"], 2)))
            batch.poll_mesh_status(wait=True)
    print(json.dumps({"time_query_batch": rows}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the training rows two ways, in one process on one GPU:

  native    icon_amd.training.point_features_device forward + torch.autograd backward of its rows: ONE native call each way
            (csrc/train_rows.hip), every stack from one search
  composed  the same rule from the existing geometry leaf and torch operators, as icon_amd/composed.py obtains it: per subject
            MeshHandle.sdf_query, then the clip, the batch-global outlier cmap list, F.grid_sample + feat_select's gather per stack,
            torch.cat - and autograd (float32 atomics) for the backward

at the shipped training sizes: B = 4 subjects x N = 8000 points, S = 2 stacks of [4,12,128,128], SMPL-size bodies
(tests/batch_subjects.py), all four smpl_feats.  HIP events around alternating calls after a warm-up, median (min, max) ms.  Also
the whole step without the filter both ways: rows, the regressor module forward and backward in training mode, MSE.  Launches,
copies / memsets and synchronising API calls per call are counted by torch.profiler in a run of their own; extra memory is the
caching allocator's high-water mark over one call.

    python tools/train_rows_timing.py [--reps 30] [--out profiles/train_rows_timing.txt]

``--prior pamir`` (written to profiles/train_rows_pamir_timing.txt): the rows [img | vol] and their gradients into
the planes AND the volumes at configs/train/pamir.yaml's size - B = 8 x N = 8000, S = 2, planes [8,6,128,128], volumes
[8,7,32,32,32] - native (icon_train_pamir_forward, icon_train_rows_backward, icon_train_vol_backward) against the same rule from
torch operators (two F.grid_sample per stack, autograd with float32 atomics), timed and counted the same way.
"""
import argparse
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main_pamir(args):
    import numpy as np
    import torch
    import torch.nn.functional as F
    import batch_pamir as bp
    from icon_amd import _lib, training
    from icon_amd.engine import IconQueryEngine
    from torch.profiler import ProfilerActivity, profile

    _lib.require_device()
    dev = torch.device("cuda:0")
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    B, N, S, C, size, Cv, D = 8, 8000, 2, 6, 128, 7, 32
    Sj = bp.subjects(B)
    eng = IconQueryEngine(prior_type="pamir")
    pts = T(bp.candidate_points(Sj, N).transpose(0, 2, 1))                     # [B,3,N]
    calibs = T(Sj["calibs"])
    torch.manual_seed(0)
    planes = [torch.randn(B, C, size, size, device=dev).requires_grad_(True) for _ in range(S)]
    vols = [torch.randn(B, Cv, D, D, D, device=dev).requires_grad_(True) for _ in range(S)]
    g_rows = [torch.randn(B, C + Cv, N, device=dev) for _ in range(S)]

    def native_rows():
        return training.point_features_device(eng, planes, pts, calibs, vol_feats=vols)[0]

    def composed_rows():
        uv = torch.baddbmm(calibs[:, :3, 3:4], calibs[:, :3, :3], pts).transpose(1, 2)
        return [torch.cat([F.grid_sample(f, uv[:, :, None, :2], align_corners=True)[..., 0],
                           F.grid_sample(v, uv[:, :, None, None, :], align_corners=True)[:, :, :, 0, 0]], 1) for f, v in zip(planes, vols)]

    def fwd_bwd(rows_fn):
        return torch.autograd.grad(rows_fn(), planes + vols, grad_outputs=g_rows)

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"pamir training rows [img | vol] and their gradients into planes and volumes, {torch.cuda.get_device_name(0)}; records of ONE run, not promises")
    say(f"B = {B} subjects x N = {N} points, S = {S} stacks: planes [{B},{C},{size},{size}], volumes [{B},{Cv},{D},{D},{D}]")
    rn, rc = native_rows(), composed_rows()
    gn, gc = fwd_bwd(native_rows), fwd_bwd(composed_rows)
    say(f"agreement: max |rows native - composed| = {max(float((a - b).detach().abs().max()) for a, b in zip(rn, rc)):.3e}, "
        f"max |grad native - composed| = {max(float((a - b).abs().max()) for a, b in zip(gn, gc)):.3e} (largest gradient {max(float(a.abs().max()) for a in gn):.3e})")
    say(f"native gradients equal from call to call, bit for bit: {all(torch.equal(a, b) for a, b in zip(gn, fwd_bwd(native_rows)))}; "
        f"composed: {all(torch.equal(a, b) for a, b in zip(gc, fwd_bwd(composed_rows)))}")
    say()
    say("rows forward + backward (planes and volumes)")
    ways = (("native", lambda: fwd_bwd(native_rows)), ("composed", lambda: fwd_bwd(composed_rows)))
    for _ in range(3):
        for _, f in ways:
            f()
    times = {name: [] for name, _ in ways}
    for _ in range(args.reps):
        for name, f in ways:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record(); e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {}
    for name, ts in times.items():
        ts = sorted(ts)
        med[name] = ts[len(ts) // 2]
        say(f"  {name:9s} {ts[len(ts) // 2]:8.3f} ms median (min {ts[0]:.3f}, max {ts[-1]:.3f}; {len(ts)} calls, HIP events, alternated)")
    say(f"  the bar (native pair not slower than the composed pair in this process): {'met' if med['native'] <= med['composed'] else 'MISSED'}")
    for name, f in ways:
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            f()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        kernels = [e for e in ev if "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        say(f"  {name:9s} {len(kernels)} kernel launches, {len(ev) - len(kernels)} copies / memsets")
        if name == "native":
            for e in sorted(kernels, key=lambda e: -e.device_time)[:6]:
                say(f"            {e.device_time:8.1f} us  {e.name[:90]}")
    out = args.out or os.path.join(ROOT, "profiles", "train_rows_pamir_timing.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--prior", default="icon", choices=("icon", "pamir"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.prior == "pamir":
        return main_pamir(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "train_rows_timing.txt")
    import numpy as np
    import torch
    import torch.nn.functional as F
    import batch_subjects as bs
    from icon_amd import _lib, training
    from icon_amd.composed import tiled_outlier_cmap
    from icon_amd.engine import IconQueryEngine, MeshHandle
    spec = importlib.util.spec_from_file_location("train_step_example", os.path.join(ROOT, "examples", "train_step.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)

    _lib.require_device()
    dev = torch.device("cuda:0")
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    B, N, S, C, size, clip = 4, 8000, 2, 12, 128, 0.05
    Sj = bs.subjects(B)
    keys = ("smpl_verts", "smpl_faces", "smpl_cmap", "smpl_vis")
    eng = IconQueryEngine(prior_type="icon", sdf_clip=clip)
    eng.set_mesh(*(T(Sj[k]) for k in keys))
    handles = [MeshHandle(*(T(Sj[k][b]) for k in keys), validate=False) for b in range(B)]
    pts = T(bs.candidate_points(Sj, N).transpose(0, 2, 1))                     # [B,3,N]
    calibs = T(Sj["calibs"])
    leaves = [T(bs.planes(B, C, size, s)).requires_grad_(True) for s in range(S)]
    g_rows = [torch.randn(B, C // 2 + 7, N, device=dev) for _ in range(S)]
    labels = (torch.rand(B, 1, N, device=dev) > 0.5).float()
    torch.manual_seed(0)
    reg = ex.Regressor((C // 2 + 7, 512, 256, 128, 1), norm="batch", last_op=torch.nn.Sigmoid()).to(dev).train()
    half = C // 2

    def native_rows():
        return training.point_features_device(eng, leaves, pts, calibs)

    def composed_rows():
        xyz = torch.baddbmm(calibs[:, :3, 3:4], calibs[:, :3, :3], pts)
        in_cube = ((xyz > -1.0) & (xyz < 1.0)).all(dim=1, keepdim=True).float()
        with torch.no_grad():
            o = [handles[b].sdf_query(xyz[b].t().contiguous()) for b in range(B)]
            sdf = torch.stack([x["sdf"] for x in o]).reshape(B, N, 1).clone()
            norm, cmap = torch.stack([x["norm"] for x in o]), torch.stack([x["cmap"] for x in o])
            vis = torch.stack([x["vis"] for x in o]).reshape(B, N, 1).float()
            outlier = sdf.abs() >= clip
            sdf[outlier] = torch.sign(sdf[outlier])
            smpl = torch.cat([sdf, tiled_outlier_cmap(cmap, sdf, outlier, False), norm], 2).permute(0, 2, 1)
            idx = ((1.0 - vis.permute(0, 2, 1)) * half + torch.arange(half, device=dev).view(1, half, 1)).long()
        uv = xyz[:, :2].transpose(1, 2).unsqueeze(2)
        rows = [torch.cat([torch.gather(F.grid_sample(f, uv, align_corners=True)[:, :, :, 0], 1, idx), smpl], 1) for f in leaves]
        return rows, in_cube

    def fwd_bwd(rows_fn):
        rows, _ = rows_fn()
        return torch.autograd.grad(rows, leaves, grad_outputs=g_rows)

    def step(rows_fn):
        rows, in_cube = rows_fn()
        err = sum(F.mse_loss(in_cube * reg(r), labels) for r in rows) / S
        return torch.autograd.grad(err, leaves + list(reg.parameters()))

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"training rows (HGPIFuNet.query in train mode up to the regressor), {torch.cuda.get_device_name(0)}; records of ONE run, not promises")
    say(f"B = {B} subjects x N = {N} points, S = {S} stacks [{B},{C},{size},{size}], {Sj['smpl_verts'].shape[1]} vertices / {Sj['smpl_faces'].shape[1]} faces per body, "
        "smpl_feats sdf norm vis cmap")
    rn, rc = native_rows()[0], composed_rows()[0]
    gn, gc = fwd_bwd(native_rows), fwd_bwd(composed_rows)
    say(f"agreement: max |rows native - composed| = {max(float((a - b).detach().abs().max()) for a, b in zip(rn, rc)):.3e}, "
        f"max |grad native - composed| = {max(float((a - b).abs().max()) for a, b in zip(gn, gc)):.3e} (largest gradient {max(float(a.abs().max()) for a in gn):.3e})")
    from torch.profiler import ProfilerActivity, profile

    def sync_events(prof):
        return len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CPU and "synchronize" in e.name.lower()])

    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        torch.cuda.synchronize()
    own = sync_events(prof)                                                    # what the closing synchronize of a profiled call records itself
    for title, fn in (("rows forward + backward", fwd_bwd), ("whole step without the filter (rows, regressor forward + backward, MSE)", step)):
        say()
        say(title)
        ways = (("native", lambda: fn(native_rows)), ("composed", lambda: fn(composed_rows)))
        for _ in range(3):
            for _, f in ways:
                f()
        times = {name: [] for name, _ in ways}
        for _ in range(args.reps):
            for name, f in ways:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); f(); e1.record(); e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        med = {}
        for name, ts in times.items():
            ts = sorted(ts)
            med[name] = ts[len(ts) // 2]
            say(f"  {name:9s} {ts[len(ts) // 2]:8.3f} ms median (min {ts[0]:.3f}, max {ts[-1]:.3f}; {len(ts)} calls, HIP events, alternated)")
        if fn is fwd_bwd:
            say(f"  the bar (native rows, forward plus backward, not slower than composed in this process): {'met' if med['native'] <= med['composed'] else 'MISSED'}")
        for name, f in ways:
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                f()
                torch.cuda.synchronize()
            ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
            kernels = [e for e in ev if "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
            syncs = sync_events(prof) - own
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = f()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            del out
            say(f"  {name:9s} {len(kernels)} kernel launches, {len(ev) - len(kernels)} copies / memsets, {syncs} synchronising API calls inside the call; "
                f"peak extra memory {peak / 2 ** 20:.2f} MiB")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

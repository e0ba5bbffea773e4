#!/usr/bin/env python3
"""Times the evaluator's normal consistency (icon_amd.evaluator) in one process on one GPU: ONE native call,
icon_normal_consistency, on the cleaned 257^3 mesh of the synthetic subject against a perturbed copy of it, 512^2, the four views
of Evaluator.calculate_normal_consist, vertex normals computed by the call.  HIP events around the call after a warm-up, median
(min, max) ms; launches per call counted by torch.profiler in a run of its own.  A record, not a promise: there is no earlier
path to compare it with.

    python tools/time_evaluator.py [--res 257] [--size 512] [--reps 30] [--out profiles/evaluator_timing.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=257)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluator_timing.txt"))
    args = ap.parse_args()
    import torch
    from icon_amd import _lib, synth
    from icon_amd.engine import IconQueryEngine
    from icon_amd.evaluator import normal_consistency_device
    from icon_amd.recon import clean_mesh, export_mesh_device

    _lib.require_device()
    dev = torch.device("cuda:0")
    a = synth.make_assets("body")
    T = lambda x: torch.from_numpy(x).to(dev)
    eng = IconQueryEngine(prior_type="icon", sdf_clip=a.sdf_clip)
    eng.set_mesh(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in a.state_dict.items()})
    occ = eng.eval_slab(T(a.features), args.res, 0, args.res)
    v, f = clean_mesh(*export_mesh_device(occ, 0.5))
    half = (args.res - 1) / 2.0
    verts, faces = ((v.float() - half) / half).contiguous(), f.contiguous()
    g = torch.Generator(device=dev).manual_seed(3)
    other = (verts + 0.002 * torch.randn(verts.shape, generator=g, device=dev)).contiguous()
    call = lambda: normal_consistency_device(verts, faces, other, faces, size=args.size)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    err = call()
    again = call()
    say(f"normal consistency, {torch.cuda.get_device_name(0)}; records of ONE run, not promises")
    say(f"mesh: cleaned {args.res}^3 synthetic subject, {verts.shape[0]} vertices, {faces.shape[0]} faces ({faces.dtype}), against a copy perturbed by "
        f"N(0, 0.002); {args.size}^2, views at 0, 180, 90, 270 degrees, vertex normals computed by the call")
    say(f"per-view error {[float(x) for x in err.cpu()]}; NC {float(err.sum()):.6f}; two calls give equal bytes: {bool(torch.equal(err, again))}")
    for _ in range(3):
        call()
    ts = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts = sorted(ts)
    say(f"native    {ts[len(ts) // 2]:8.3f} ms median (min {ts[0]:.3f}, max {ts[-1]:.3f}; {len(ts)} calls, HIP events)")
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        call()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = [e for e in ev if "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    native = [e for e in kernels if "k_ev_" in e.name or "k_s1_" in e.name]
    say(f"native    {len(kernels)} kernel launches per call ({len(native)} of them the library's), {len(ev) - len(kernels)} copies / memsets")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

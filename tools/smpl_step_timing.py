#!/usr/bin/env python3
"""Times one skinning step of the body-fit loop - forward plus backward of <verts, Gv> + <joints, Gj> into betas and the rotation
matrices at B = 1, V = 6890, J = 24, NB = 10 - two ways, in one process on one GPU:

  native    icon_amd.smpl.smpl_lbs_device over csrc/smpl.hip
  composed  the float64 oracle's statement (tests/smpl_oracle.py: lbs) run in float32 from torch operators on the same device:
            the operator sequence of the reference's lib/smplx lbs(), Python loop over the kinematic chain included

HIP events around alternating steps after a warm-up, median (min) ms; launches per step counted by torch.profiler in a run of its
own; extra memory: the caching allocator's high-water mark over one step plus, for the native path, the scratch its pool holds.

    python tools/smpl_step_timing.py [--reps 50] [--out profiles/smpl_step_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smpl_step_timing.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import smpl_oracle as so
    from icon_amd import _lib
    from icon_amd.smpl import SmplModel, smpl_lbs_device

    _lib.require_device()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fns, reps):
        ms = [[] for _ in fns]
        for _ in range(reps):
            for k, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record(); e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return [(float(np.median(m)), float(np.min(m))) for m in ms]

    def launches(fn):
        from torch.profiler import ProfilerActivity, profile
        fn(); torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
        on_device = [ev for ev in prof.key_averages() if ev.device_type == torch.autograd.DeviceType.CUDA]   # not the runtime calls that enqueue them
        n = sum(ev.count for ev in on_device if "memcpy" not in ev.key.lower() and "memset" not in ev.key.lower())
        other = sum(ev.count for ev in on_device) - n
        if not any("k_smpl_" in ev.key or "aten" in ev.key or "elementwise" in ev.key for ev in on_device):
            raise SystemExit(f"the profiler recorded no kernels: {sorted(ev.key for ev in on_device)[:8]}")
        own = {}                                                           # the skinning's kernels: microseconds on the device per launch
        for ev in on_device:
            if "k_smpl_" in ev.key:
                us = getattr(ev, "self_device_time_total", None) or getattr(ev, "self_cuda_time_total", 0.0)
                own[ev.key[ev.key.index("k_smpl_"):].split("(")[0].split("E")[0]] = (ev.count / 5.0, us / max(ev.count, 1))
        return n / 5.0, other / 5.0, own

    def peak(fn):
        """-> MiB allocated at the high-water mark of one step above what was allocated before it: outputs and temporaries (the
        native path's pooled scratch is not in it)"""
        fn(); torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(); torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20

    name = "body"
    V, J, NB, _ = so.CASES[name]
    T = lambda a: torch.from_numpy(a).to(dev)
    case = {k: T(a) for k, a in so.case(name).items()}
    model = SmplModel(*(case[k] for k in so.BUFFERS))
    betas, rot, gv, gj = (T(a) for a in so.inputs(name, 1))
    betas.requires_grad_(True), rot.requires_grad_(True)

    def native():
        verts, joints = smpl_lbs_device(betas, rot, model)
        return torch.autograd.grad((verts * gv).sum() + (joints * gj).sum(), (betas, rot))

    on_host = dict(case, parents=case["parents"].cpu())                   # the chain's loop reads its parents on the host: no synchronisation per step

    def composed():
        verts, joints = so.lbs(betas, rot, on_host)
        return torch.autograd.grad((verts * gv).sum() + (joints * gj).sum(), (betas, rot))

    nbytes = C.c_int64(0)
    _lib.check(_lib.lib().icon_smpl_bytes(C.c_int64(1), C.c_int64(V), J, NB, model.K, C.byref(nbytes)), "icon_smpl_bytes")
    scratch = nbytes.value / 2.0 ** 20
    say("one skinning step of the body-fit loop: forward + backward of <verts, Gv> + <joints, Gj> into betas and the rotation matrices")
    say(f"device: {torch.cuda.get_device_name(0)}; HIP events, {args.reps} alternating repetitions after 5 warm-up steps; median (min) ms")
    for _ in range(5):
        gn, gc = native(), composed()
    torch.cuda.synchronize()
    db = float((gn[0] - gc[0]).abs().max() / gc[0].abs().max())
    dr = float((gn[1] - gc[1]).abs().max() / gc[1].abs().max())
    say()
    say(f"B = 1, V = {V}, J = {J}, NB = {NB}, K = {model.K}; native against composed: grad betas {db:.1e}, grad rot_mats {dr:.1e} (relative, max norm)")
    (tn, tn_min), (tc, tc_min) = timed([native, composed], args.reps)
    (ln, on, kn), (lc, oc, _) = launches(native), launches(composed)
    pn, pc = peak(native), peak(composed)
    say(f"  native    {tn:8.3f} ({tn_min:.3f}) ms   {ln:6.1f} kernel launches + {on:.1f} copies / fills per step   extra memory {pn + scratch:8.2f} MiB "
        f"({pn:.2f} outputs and temporaries + {scratch:.2f} pooled scratch)")
    say(f"  composed  {tc:8.3f} ({tc_min:.3f}) ms   {lc:6.1f} kernel launches + {oc:.1f} copies / fills per step   extra memory {pc:8.2f} MiB "
        f"(outputs and temporaries)")
    say(f"  -> {lc / ln:.1f} x fewer launches, {tc / tn:.1f} x in time ({'the native step is the faster one' if tn < tc else 'THE NATIVE STEP IS NOT THE FASTER ONE'}); "
        f"{sum(c for c, _ in kn.values()):.1f} of the native launches are the skinning's own, the others the torch operators of the two inner "
        f"products and their backward")
    say("  the skinning's kernels on the device, microseconds per launch (torch.profiler): "
        + ", ".join(f"{k} {us:.1f}" for k, (_, us) in sorted(kn.items())))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the gradient of the normal maps (icon_amd.render.render_normal_device(differentiable=True)) at 512^2:
the SMPL-size body from cameras 0 and 2 - the backward call alone, and forward + L1 loss + backward as a fit-loop iteration runs
them -, the cleaned 257^3 marching-cubes mesh of the dense synthetic volume under both lane mappings of the per-face sweep, and
render_checker's `quads` (two whole-image faces: the deferred big-box list).  HIP events around each call after a warm-up; the
median (min .. max) of the repetitions.  There is no pytorch3d build for this device to compare with: the figures are records.

    python tools/time_render_grad.py [--res 257] [--reps 30] [--out profiles/render_grad_timing.txt]
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
    ap.add_argument("--res", type=int, default=257)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_grad_timing.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from icon_amd import _lib, synth
    from icon_amd.engine import IconQueryEngine
    from icon_amd.recon import clean_mesh, export_mesh_device
    from icon_amd.render import render_normal_device

    _lib.require_device()
    dev = torch.device("cuda:0")
    S = args.size
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def set_lanes(n):
        _lib.check(_lib.lib().icon_debug_set_option(b"rn_lanes", C.c_int(n)), "rn_lanes")

    def timed(fn, setup=None):
        """one event pair per call (setup() runs outside the pair) -> 'median (min .. max) ms'"""
        ms = []
        for k in range(5 + args.reps):
            ctx = setup() if setup else None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(ctx); e1.record(); e1.synchronize()
            if k >= 5:
                ms.append(e0.elapsed_time(e1))
        return f"{np.median(ms):8.3f} ({np.min(ms):.3f} .. {np.max(ms):.3f}) ms"

    def field(n):
        c = (torch.arange(S, device=dev, dtype=torch.float32) + 0.5) / S
        return torch.stack([torch.sin(5.0 * c[None, :] + 3.0 * c[:, None] + k) for k in range(3 * n)]).reshape(n, 3, S, S).contiguous()

    def backward_only(v, f, cams):
        """-> a setup that renders (outside the timed pair) and a function that runs the backward call alone"""
        g = field(len(cams))

        def setup():
            vv = v.detach().clone().requires_grad_(True)
            return vv, render_normal_device(vv, f, cams, S, differentiable=True)

        def run(ctx):
            ctx[1].backward(g)
        return setup, run

    def head(label, v, f, cams):
        img = render_normal_device(v, f, cams, S)
        say()
        say(f"{label}: {v.shape[0]} vertices, {f.shape[0]} faces, {S}^2 x {len(cams)} views; {100 * float((img[:, 0] != 0).float().mean()):.1f} % of the pixels covered")

    a = synth.make_assets("body")
    T = lambda x: torch.from_numpy(x).to(dev)
    say(f"render_normal_device(differentiable=True); device: {torch.cuda.get_device_name(0)}; HIP events, {args.reps} repetitions after 5 warm-up calls; "
        f"median (min .. max) ms")
    bv, bf = T(a.smpl_verts[0]).float().contiguous(), T(a.smpl_faces[0]).long().contiguous()
    head("synthetic SMPL-size body", bv, bf, (0, 2))
    try:
        setup, run = backward_only(bv, bf, (0, 2))
        say(f"  backward call (default mapping)        {timed(run, setup)}")
        target = field(2) * 0.5

        def step(_):
            vv = bv.detach().clone().requires_grad_(True)
            img = render_normal_device(vv, bf, (0, 2), S, differentiable=True)
            (img - target).abs().mean().backward()
        say(f"  forward + L1 loss + backward           {timed(step)}")
        if args.res:
            eng = IconQueryEngine(prior_type="icon", sdf_clip=a.sdf_clip)
            eng.set_mesh(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
            eng.set_regressor({k: torch.from_numpy(v) for k, v in a.state_dict.items()})
            occ = eng.eval_slab(T(a.features), args.res, 0, args.res)
            mv, mf = clean_mesh(*export_mesh_device(occ, 0.5))
            del occ
            half = (args.res - 1) / 2.0
            mv = ((mv.float() - half) / half).contiguous()
            head(f"cleaned marching-cubes mesh {args.res}^3", mv, mf, (0, 1, 2, 3))
            grads = {}
            for lanes, what in ((1, "1 thread per face "), (8, "8 lanes per face  ")):
                set_lanes(lanes)
                setup, run = backward_only(mv, mf, (0, 1, 2, 3))
                say(f"  backward call, {what}      {timed(run, setup)}")
                ctx = setup(); run(ctx); grads[lanes] = ctx[0].grad
            set_lanes(0)
            d = float((grads[1] - grads[8]).abs().max() / grads[8].abs().max())
            say(f"  the two mappings' gradients differ by {d:.2e} of the largest entry (another summation order over a face's pixels)")
        import render_checker
        qv, qf = (T(x) for x in render_checker.quads())
        head("render_checker.quads (two whole-image faces: the deferred list)", qv, qf, (0, 1, 2, 3))
        setup, run = backward_only(qv, qf, (0, 1, 2, 3))
        say(f"  backward call                          {timed(run, setup)}")
    finally:
        set_lanes(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

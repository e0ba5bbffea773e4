#!/usr/bin/env python3
"""Times the turntable video's frames (icon_amd.render.render_turntable_device / Render.get_rendered_frames):
360 frames at 512^2 of the SMPL-size body and of the cleaned 257^3 marching-cubes mesh, four ways -

    (a) ONE render_turntable_device call;
    (b) 90 calls of render_normal_device(cams 0..3): the only way to 360 frames of one mesh and size before the turntable call
        existed - the baseline;
    (c) Render.get_rendered_frames end to end for two meshes and two images (the device side of get_rendered_video);
    (d) the same with every chunk copied to the host, as a video writer needs them.

(a) and (b) alternate in one process after a warm-up, a host clock around work that ends in a device synchronise; (c) and (d)
alternate likewise.  (a) is also timed at other chunk sizes ("tt_chunk").  There is no pytorch3d build for this device to compare
with: the figures are records.

    python tools/time_turntable.py [--reps 10] [--out profiles/turntable_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=257)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "turntable_timing.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from icon_amd import _lib, synth
    from icon_amd.engine import IconQueryEngine
    from icon_amd.recon import clean_mesh, export_mesh_device
    from icon_amd.render import Render, render_normal_device, render_turntable_device

    _lib.require_device()
    dev = torch.device("cuda:0")
    S, angles = args.size, list(range(360))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fns, reps):
        """alternating calls, each ending in a synchronise -> (median, min, max) ms per function"""
        ms = [[] for _ in fns]
        for _ in range(reps):
            for k, fn in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[k].append(1e3 * (time.perf_counter() - t0))
        return [(float(np.median(m)), float(np.min(m)), float(np.max(m))) for m in ms]

    fmt = lambda r: f"{r[0]:9.2f} ms  (min {r[1]:.2f}, max {r[2]:.2f})"

    def set_chunk(n):
        _lib.check(_lib.lib().icon_debug_set_option(b"tt_chunk", C.c_int(n)), "tt_chunk")

    def measure(label, v, f):
        one = lambda: render_turntable_device(v, f, angles, S)

        def ninety():
            for _ in range(90):
                render_normal_device(v, f, (0, 1, 2, 3), S)
        for _ in range(2):
            frames = one()
            ninety()
        torch.cuda.synchronize()
        covered = float((frames != 127).any(3).float().mean())
        say()
        say(f"{label}: {v.shape[0]} vertices, {f.shape[0]} faces, 360 frames at {S}^2; {100 * covered:.1f} % of the pixels covered")
        ra, rb = timed([one, ninety], args.reps)
        say(f"  (a) one render_turntable_device call               {fmt(ra)}")
        say(f"  (b) 90 x render_normal_device(cams 0..3)           {fmt(rb)}")
        say(f"      (a) / (b) = {ra[0] / rb[0]:.2f}")
        try:
            sweep = {k: [] for k in (4, 8, 16, 32)}
            for k in sweep:                                                 # warm-up; the chunk does not change a byte
                set_chunk(k)
                assert torch.equal(one(), frames)
            for _ in range(args.reps):                                      # alternated like the rest
                for k in sweep:
                    set_chunk(k)
                    sweep[k].append(timed([one], 1)[0][0])
            say("  (a) by views per chunk (median ms): " + ", ".join(f"{k}: {np.median(m):.2f}" for k, m in sweep.items()))
        finally:
            set_chunk(0)

    def measure_frames(meshes, images):
        r = Render(size=S, device=dev)
        r.load_meshes([m[0] for m in meshes], [m[1] for m in meshes])

        def on_device():
            for frames in r.get_rendered_frames(images):
                pass

        def to_host():
            for frames in r.get_rendered_frames(images):
                frames.cpu()
        for _ in range(2):
            on_device(); to_host()
        rc, rd = timed([on_device, to_host], args.reps)
        W = next(r.get_rendered_frames(images, angles=[0])).shape[2]
        say()
        say(f"Render.get_rendered_frames: {len(meshes)} meshes ({', '.join(str(m[1].shape[0]) for m in meshes)} faces), {len(images)} images "
            f"{tuple(images[0].shape)}, 360 frames of {S} x {W}, 30 per chunk")
        say(f"  (c) end to end, frames left on the device          {fmt(rc)}")
        say(f"  (d) with every chunk copied to the host            {fmt(rd)}")

    a = synth.make_assets("body")
    T = lambda x: torch.from_numpy(x).to(dev)
    say(f"turntable frames; device: {torch.cuda.get_device_name(0)}; host clock around calls that end in a synchronise, "
        f"{args.reps} alternating repetitions after 2 warm-up rounds; median (min, max)")
    body = (T(a.smpl_verts[0]).float().contiguous(), T(a.smpl_faces[0]).long().contiguous())
    measure("synthetic SMPL-size body", *body)
    eng = IconQueryEngine(prior_type="icon", sdf_clip=a.sdf_clip)
    eng.set_mesh(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in a.state_dict.items()})
    occ = eng.eval_slab(T(a.features), args.res, 0, args.res)
    v, f32 = clean_mesh(*export_mesh_device(occ, 0.5))
    del occ
    half = (args.res - 1) / 2.0
    dense = (((v.float() - half) / half).contiguous(), f32)
    measure(f"cleaned marching-cubes mesh {args.res}^3", *dense)
    rng = np.random.RandomState(0)
    measure_frames([body, dense], [rng.randint(0, 256, (512, 512, 3)).astype(np.uint8) for _ in range(2)])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

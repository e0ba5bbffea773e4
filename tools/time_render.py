#!/usr/bin/env python3
"""Times icon_amd.render.render_normal_device: the SMPL-size body at 512^2 x 2 views with depth, and the cleaned marching-cubes
meshes of the dense synthetic volumes (257^3, 513^3) at 512^2 x 4 views, for both lane mappings of the rasteriser (eight lanes
per face / one thread per face).  HIP events around alternating calls after a warm-up; per-kernel times from a torch.profiler
run of their own.  There is no pytorch3d build for this device to compare with: the figures are records.  query_color_device is
timed in the same session on the same meshes (the two share the S1 normal kernels of csrc/s1_normals_device.h).

    python tools/time_render.py [--res 257 513] [--reps 30] [--out profiles/render_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="*", default=[257, 513])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_timing.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from icon_amd import _lib, synth
    from icon_amd.engine import IconQueryEngine
    from icon_amd.recon import clean_mesh, export_mesh_device, query_color_device
    from icon_amd.render import render_normal_device

    _lib.require_device()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fns, reps):
        """alternating calls, one event pair each -> median / min ms per function"""
        ms = [[] for _ in fns]
        for _ in range(reps):
            for k, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record(); e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return [(float(np.median(m)), float(np.min(m))) for m in ms]

    def set_lanes(n):
        _lib.check(_lib.lib().icon_debug_set_option(b"rn_lanes", C.c_int(n)), "rn_lanes")

    def with_lanes(n, fn):
        def run():
            set_lanes(n)
            return fn()
        return run

    def measure(label, v, f, cams, depth):
        S = args.size
        call = lambda: render_normal_device(v, f, cams, S, return_depth=depth)
        outs = {}
        for lanes in (8, 1):
            set_lanes(lanes)
            for _ in range(5):
                o = call()
            torch.cuda.synchronize()
            outs[lanes] = o[0] if depth else o
        same = bool(torch.equal(outs[8], outs[1]))
        covered = float((outs[8][:, 0] != 0).float().mean())
        say()
        say(f"{label}: {v.shape[0]} vertices, {f.shape[0]} faces, {S}^2 x {len(cams)} views{' with depth' if depth else ''}; "
            f"{100 * covered:.1f} % of the pixels covered; the two mappings give equal bytes: {same}")
        (t8, m8), (t1, m1) = timed([with_lanes(8, call), with_lanes(1, call)], args.reps)
        say(f"  whole call, 8 lanes per face    {t8:8.3f} ({m8:.3f}) ms")
        say(f"  whole call, 1 thread per face   {t1:8.3f} ({m1:.3f}) ms")
        from torch.profiler import ProfilerActivity, profile
        per = {}
        try:
            for lanes in (8, 1):
                set_lanes(lanes)
                call(); torch.cuda.synchronize()
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    for _ in range(10):
                        call()
                    torch.cuda.synchronize()
                for ev in prof.key_averages():
                    t = getattr(ev, "device_time_total", None)
                    if t is None:
                        t = getattr(ev, "cuda_time_total", 0.0)
                    if any(p in ev.key for p in ("k_rn_", "k_s1_", "k_rs_")) and ev.count:   # k_s1_, k_rs_: the shared kernels (s1_normals_device.h, raster_device.h)
                        key = ev.key.replace("(anonymous namespace)::", "").replace("icon::", "").replace("void ", "").split("(")[0]
                        if lanes == 8 or "k_rn_raster" in key:
                            per[key + (f"  [{lanes} lane(s)]" if "k_rn_raster" in key else "")] = t / ev.count
        finally:
            set_lanes(0)
        if not any("k_rn_raster" in k for k in per):
            raise SystemExit(f"the profiler recorded no rasteriser kernels: {sorted(per)}")
        say("  per kernel (torch.profiler, mean of 10 launches, us):")
        for k in sorted(per):
            say(f"    {k:60s} {per[k]:9.1f}")

    a = synth.make_assets("body")
    T = lambda x: torch.from_numpy(x).to(dev)
    say(f"render_normal_device; device: {torch.cuda.get_device_name(0)}; HIP events, {args.reps} alternating repetitions after 5 warm-up calls; median (min) ms")
    measure("synthetic SMPL-size body", T(a.smpl_verts[0]).float().contiguous(), T(a.smpl_faces[0]).long().contiguous(), (0, 2), True)
    if args.res:
        eng = IconQueryEngine(prior_type="icon", sdf_clip=a.sdf_clip)
        eng.set_mesh(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
        eng.set_regressor({k: torch.from_numpy(v) for k, v in a.state_dict.items()})
        image = torch.from_numpy(np.tanh(synth.make_feature_planes(3, 512, 531)[0]).astype(np.float32))[None].to(dev)
    for res in args.res:
        occ = eng.eval_slab(T(a.features), res, 0, res)
        v, f32 = clean_mesh(*export_mesh_device(occ, 0.5))
        del occ
        half = (res - 1) / 2.0
        v = ((v.float() - half) / half).contiguous()
        measure(f"cleaned marching-cubes mesh {res}^3", v, f32, (0, 1, 2, 3), False)
        qc = lambda: query_color_device(v, f32, image)
        for _ in range(5):
            qc()
        torch.cuda.synchronize()
        runs = [timed([qc], args.reps)[0] for _ in range(3)]
        say(f"  query_color_device on the same mesh, three runs of {args.reps}: " + ", ".join(f"{m:.3f} ({mn:.3f})" for m, mn in runs) + " ms")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

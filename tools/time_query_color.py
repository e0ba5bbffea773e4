#!/usr/bin/env python3
"""Times icon_amd.recon.query_color_device on the cleaned marching-cubes meshes of the dense synthetic volumes (257^3, 513^3)
against the only composition of the same result that exists without it, on device tensors: get_visibility (icon_visibility)
+ torch.nn.functional.grid_sample + vertex normals by torch index_add_.  HIP events around alternating calls after a warm-up;
per-kernel times of the rasteriser (one wavefront per face - icon_visibility's mapping - against the default 8 lanes per face) and
of the resolve passes from a torch.profiler run of their own.

    python tools/time_query_color.py [--res 257 513] [--reps 30] [--out profiles/query_color_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[257, 513])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_color_timing.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from icon_amd import _lib, synth
    from icon_amd.engine import IconQueryEngine, get_visibility
    from icon_amd.recon import clean_mesh, export_mesh_device, query_color_device

    _lib.require_device()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    a = synth.make_assets("body")
    T = lambda x: torch.from_numpy(x).to(dev)
    eng = IconQueryEngine(prior_type="icon", sdf_clip=a.sdf_clip)
    eng.set_mesh(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in a.state_dict.items()})
    image = torch.from_numpy(np.tanh(synth.make_feature_planes(3, 512, 531)[0]).astype(np.float32))[None].to(dev)
    flip = torch.tensor([1.0, -1.0], device=dev)

    def composed(v, f64):
        (xy, z) = v.split([2, 1], dim=1)
        vis = get_visibility(xy, z, f64[:, [0, 2, 1]]).flatten()
        colors = (F.grid_sample(image, (xy * flip)[None, :, None, :], align_corners=True)[0, :, :, 0].permute(1, 0) + 1.0) * 0.5 * 255.0
        tri = v[f64]
        fn = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
        n = torch.zeros_like(v)
        for k in range(3):
            n.index_add_(0, f64[:, k], fn)
        n = n / n.norm(dim=1, keepdim=True).clamp_min(1e-6)
        colors[vis == 0.0] = ((n + 1.0) * 0.5 * 255.0)[vis == 0.0]
        return colors, vis

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
        _lib.check(_lib.lib().icon_debug_set_option(b"qc_lanes", C.c_int(n)), "qc_lanes")

    say("query_color on the cleaned marching-cubes mesh of the dense synthetic volume; image 512 x 512; z-buffer 4096^2")
    say(f"device: {torch.cuda.get_device_name(0)}; HIP events, {args.reps} alternating repetitions after 5 warm-up calls; median (min) ms")
    for res in args.res:
        occ = eng.eval_slab(T(a.features), res, 0, res)
        v, f32 = clean_mesh(*export_mesh_device(occ, 0.5))
        del occ
        half = (res - 1) / 2.0
        v = ((v.float() - half) / half).contiguous()
        f64 = f32.long().contiguous()
        native = lambda: query_color_device(v, f32, image, return_vis=True)
        comp = lambda: composed(v, f64)
        for _ in range(5):
            cn, vn = native(); cc_, vc = comp()
        torch.cuda.synchronize()
        same_vis = bool(torch.equal(vn, vc))
        dcol = float((cn - cc_).abs().max())
        say()
        say(f"{res}^3: {v.shape[0]} vertices, {f32.shape[0]} faces, {100 * float(vn.mean()):.1f} % visible; visible set equal to the composition's: {same_vis}; "
            f"max |colour difference| {dcol:.2e} (the composition's normals are atomic float sums)")
        (tn, tn_min), (tc, tc_min) = timed([native, comp], args.reps)
        say(f"  native query_color_device (int32 faces)          {tn:8.3f} ({tn_min:.3f}) ms")
        say(f"  get_visibility + grid_sample + index_add_        {tc:8.3f} ({tc_min:.3f}) ms   -> {tc / tn:.1f} x")
        rows = []
        for lanes in (64, 0):
            set_lanes(lanes)
            for _ in range(3):
                native()
            rows.append((lanes, timed([native], args.reps)[0]))
        set_lanes(0)
        for lanes, (m, mn) in rows:
            say(f"  native, {'64 lanes per face (one wavefront: the old mapping)' if lanes == 64 else ' 8 lanes per face (the default)':52s} {m:8.3f} ({mn:.3f}) ms")
        # per-kernel times: a profiler run of its own (a failure here fails the tool: the file must not look complete without them)
        from torch.profiler import ProfilerActivity, profile
        per = {}
        try:
            for lanes in (64, 0):
                set_lanes(lanes)
                native(); torch.cuda.synchronize()
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    for _ in range(10):
                        native()
                    if lanes == 64:
                        for _ in range(10):
                            get_visibility(v[:, :2], v[:, 2:3], f64[:, [0, 2, 1]])
                    torch.cuda.synchronize()
                for ev in prof.key_averages():
                    t = getattr(ev, "device_time_total", None)
                    if t is None:
                        t = getattr(ev, "cuda_time_total", 0.0)
                    if any(p in ev.key for p in ("k_qc_", "k_s1_", "k_vis_")) and ev.count:     # k_s1_: the shared normal kernels (s1_normals_device.h)
                        key = ev.key.replace("(anonymous namespace)::", "").replace("icon::", "").replace("void ", "").split("(")[0]
                        if lanes == 64 or "k_qc_raster" in key:
                            per[key] = t / ev.count
        finally:
            set_lanes(0)
        if not any("k_qc_raster" in k for k in per) or not any("k_vis_raster" in k for k in per):
            raise SystemExit(f"the profiler recorded no rasteriser kernels: {sorted(per)}")
        say("  per kernel (torch.profiler, mean of 10 launches, us):")
        for k in sorted(per):
            say(f"    {k:60s} {per[k]:9.1f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the training sampler two ways, in one process on one GPU:

  native    icon_amd.sampling.sample_geo_device - ONE native call (csrc/sample_geo.hip), nothing waited for
  composed  the same rule from torch operators on the same device: torch.randint / randn / rand / randperm for the draws, float64
            arithmetic rounded once, MeshHandle.sdf_query for the labels, nonzero for the balancing - what a port without kernels
            would run.  Another generator, so its samples are other samples of the same distribution: the inside shares are printed.

with the shipped settings (N = 8000, sigma_geo = 5.0, zray_type off and on with ray_sample_num = 1) on the cleaned 257^3 mesh of
the synthetic subject scaled to a scan's units (x 100).  HIP events around alternating calls after a warm-up, median (min, max) ms;
the composed call ends in the synchronisations of its own nonzero and of sdf_query, which the events include.  Launches per call
counted by torch.profiler in a run of its own; extra memory: the caching allocator's high-water mark over one call (for the native
call plus the scratch its pool keeps).  The reference's own CPU time (trimesh's contains) is not measured: trimesh is not here.

    python tools/sample_geo_timing.py [--res 257] [--reps 30] [--out profiles/sample_geo_timing.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def composed(torch, scan, A, Ainv, N, sigma, zray, R):
    """the rule from torch operators: A / Ainv float64 [3,4] on the device"""
    dev, nS, nU = scan.device, 4 * N, N // 4
    ids = torch.randint(scan.V, (nS,), device=dev)
    off = torch.randn((nS, 1), dtype=torch.float64, device=dev) * sigma
    surf = scan.verts[ids].double() + scan.vert_normals[ids].double() * off
    proj = lambda p, m: p @ m[:, :3].T + m[:, 3]
    parts = [surf, proj(2.0 * torch.rand((nU, 3), dtype=torch.float64, device=dev) - 1.0, Ainv)]
    if zray:
        cube = proj(surf, A).repeat_interleave(R, 0)
        cube[:, 2] += 0.5 * (0.40 * torch.randn(nS * R, dtype=torch.float64, device=dev))
        parts.append(proj(cube, Ainv))
    pts = torch.cat(parts)
    pts = pts[torch.randperm(pts.shape[0], device=dev)].float()
    inside = scan.handle.sdf_query(pts)["inside"]
    ins, outs = torch.nonzero(inside)[:, 0], torch.nonzero(~inside)[:, 0]
    nin = ins.shape[0]
    if nin > N // 2:
        ins, outs = ins[:N // 2], outs[:N // 2]
    else:
        outs = outs[:N - nin]
    samples = torch.cat([pts[ins], pts[outs]])
    labels = torch.cat([torch.ones(ins.shape[0], device=dev), torch.zeros(outs.shape[0], device=dev)])
    return samples, labels, inside


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=257)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_geo_timing.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from icon_amd import _lib, _native, synth
    from icon_amd.engine import IconQueryEngine
    from icon_amd.recon import clean_mesh, export_mesh_device
    from icon_amd.sampling import ScanMesh, sample_geo_device

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
    scan = ScanMesh((100.0 * (v.float() - half) / half).contiguous(), f.contiguous())
    calib = np.array([[1 / 128, 0, 0, 0.03125], [0, -1 / 128, 0, 0.0625], [0, 0, 1 / 128, -0.015625], [0, 0, 0, 1]])
    A, Ainv = T(calib[:3].copy()), T(np.linalg.inv(calib)[:3].copy())
    N, sigma, R = 8000, 5.0, 1
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"training samples (get_sampling_geo), {torch.cuda.get_device_name(0)}; records of ONE run, not promises")
    say(f"scan: cleaned {args.res}^3 synthetic subject x 100, {scan.V} vertices, {scan.F} faces; N = {N}, sigma_geo = {sigma}, ray_sample_num = {R}")
    say("the reference's own time on a CPU worker (trimesh's contains): not measured - trimesh is not installed here")
    from torch.profiler import ProfilerActivity, profile
    for zray in (False, True):
        seed = [0]

        def native(return_all=False):                                            # a new seed per call, as a loader would pass
            seed[0] += 1
            return sample_geo_device(scan, calib, N, sigma, zray_type=zray, ray_sample_num=R, seed=seed[0], return_all=return_all)

        torch_way = lambda: composed(torch, scan, A, Ainv, N, sigma, zray, R)
        out_n, out_c = native(return_all=True), torch_way()
        n = out_n[3]["all_inside"].shape[0]
        say()
        say(f"zray_type = {zray}: n = {n} samples before balancing; inside share native {float(out_n[3]['all_inside'].float().mean()):.4f}, "
            f"composed {float(out_c[2].float().mean()):.4f}; rows native {out_n[2].tolist()}, composed {int(out_c[1].sum())} + {int((out_c[1] == 0).sum())}")
        for _ in range(3):
            native(); torch_way()
        times = {"native": [], "composed": []}
        for _ in range(args.reps):
            for name, fn in (("native", native), ("composed", torch_way)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record(); e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        med = {}
        for name, ts in times.items():
            ts = sorted(ts)
            med[name] = ts[len(ts) // 2]
            say(f"  {name:9s} {ts[len(ts) // 2]:8.3f} ms median (min {ts[0]:.3f}, max {ts[-1]:.3f}; {len(ts)} calls, HIP events, alternated)")
        say(f"  the bar (native not slower than composed in this process): {'met' if med['native'] <= med['composed'] else 'MISSED'}")
        for name, fn in (("native", native), ("composed", torch_way)):
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                fn()
                torch.cuda.synchronize()
            ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
            kernels = [e for e in ev if "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            pool = sum(b.numel() for b in _native._tls.pool.values()) if name == "native" else 0
            say(f"  {name:9s} {len(kernels)} kernel launches, {len(ev) - len(kernels)} copies / memsets per call; peak extra memory {peak / 2 ** 20:.2f} MiB"
                + (f" + {pool / 2 ** 20:.2f} MiB pooled scratch" if name == "native" else ""))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

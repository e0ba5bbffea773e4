#!/usr/bin/env python3
"""Times garment extraction two ways, in one process on one GPU:

  native    icon_amd.garment.extract_cloth_device - ONE native call (csrc/garment.hip)
  composed  the same rule from torch operators on the same device, in float64, chunked (the dense 70 k x 6,890 float64 distance
            matrix alone would be 3.9 GB) - what a port without kernels would run; its output is compared with the native one

on the cleaned 257^3 mesh of the synthetic subject, the 6,890-vertex synthetic body as the source mesh (parts = height bands, every
other band removed) and three polygons of about 200 vertices.  HIP events around alternating calls after a warm-up, median (min, max)
ms; both calls end in a synchronisation of their own (the counts / the nonzero), which the events include.  Launches per call counted by
torch.profiler in a run of its own; extra memory: the caching allocator's high-water mark over one call (for the native call plus the
scratch its pool keeps).

    python tools/garment_timing.py [--res 257] [--reps 30] [--out profiles/garment_timing.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/garment_timing.py --profile-only      (the three stages, per kernel)
    python tools/garment_timing.py --dump mesh.npz / --reference-cpu mesh.npz    (the inputs; the reference's own function on them, CPU)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def polygons(np):
    """three overlapping polygons of about 200 vertices over the torso, in the model plane"""
    rng = np.random.RandomState(19)
    out = []
    for n, (cx, cy), (rx, ry) in ((200, (0.0, 0.12), (0.24, 0.42)), (211, (-0.1, 0.2), (0.16, 0.3)), (190, (0.12, -0.05), (0.15, 0.25))):
        a = np.sort(rng.uniform(0, 2 * np.pi, n))
        r = rng.uniform(0.85, 1.0, n)
        out.append(np.stack([cx + rx * r * np.cos(a), cy + ry * r * np.sin(a)], 1))
    return out


def composed(torch, verts, faces, polys, src, rem, chunk=4096):
    """rules 2-6 from torch operators, float64, nothing larger than chunk x max(n, Vs) at a time"""
    V = verts.shape[0]
    sel = torch.zeros(V, dtype=torch.bool, device=verts.device)
    xy = verts[:, :2].double()
    for p in polys:
        x0, y0 = p[:, 0][None], p[:, 1][None]
        x1, y1 = torch.roll(p[:, 0], -1)[None], torch.roll(p[:, 1], -1)[None]
        for a in range(0, V, 4 * chunk):
            tx, ty = xy[a:a + 4 * chunk, 0:1], xy[a:a + 4 * chunk, 1:2]
            f0, f1 = y0 >= ty, y1 >= ty
            cross = (f0 != f1) & ((((y1 - ty) * (x0 - x1)) >= ((x1 - tx) * (y0 - y1))) == f1)
            sel[a:a + 4 * chunk] |= (cross.sum(1) & 1).bool()
    ids = torch.nonzero(sel)[:, 0]
    q, s = verts[ids].double(), src.double()
    nn = torch.empty(ids.shape[0], dtype=torch.int64, device=verts.device)
    for a in range(0, ids.shape[0], chunk):
        d = q[a:a + chunk, None, :] - s[None]
        d = d * d
        nn[a:a + chunk] = ((d[..., 0] + d[..., 1]) + d[..., 2]).argmin(1)
    keep_v = torch.zeros(V, dtype=torch.bool, device=verts.device)
    keep_v[ids] = ~rem[nn]
    f = faces.long()
    keep_f = keep_v[f].any(1)
    kept = f[keep_f]
    used = torch.zeros(V, dtype=torch.bool, device=verts.device)
    used[kept.reshape(-1)] = True
    remap = torch.cumsum(used, 0) - 1
    out_ids = torch.nonzero(used)[:, 0]
    return verts[out_ids], remap[kept].int(), out_ids.int()


def reference_cpu(path, reps=3):
    """the reference's own extract_cloth (stand-in trimesh container of tests/test_garment.py) on the dumped inputs, on this CPU"""
    import numpy as np
    import test_garment as tg
    d = np.load(path)
    ref = tg.load_reference()
    assert ref is not None, "the reference tree, matplotlib and scikit-learn are needed"
    polys = [d[f"poly_{k}"] for k in range(3)]
    scale = tg.go.polygons_to_model_plane([np.array([[1.0, 1.0], [0.0, 0.0]])], tg.K_INFER, tg.R_INFER, tg.T_INFER)[0][0]
    seg = dict(coord_normalized=[p / scale for p in polys], type_id=1)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        mesh = ref.extract_cloth(tg._Mesh(d["verts"], d["faces"]), seg, tg.K_INFER, tg.R_INFER, tg.T_INFER, tg._Mesh(d["body"], d["body_faces"]))
        ts.append(1e3 * (time.perf_counter() - t0))
    print(f"reference extract_cloth on this CPU (type_id 1, its own part table, stand-in container): {sorted(ts)[len(ts) // 2]:.0f} ms "
          f"(min {min(ts):.0f}, {reps} runs) -> {len(mesh.vertices)} vertices, {len(mesh.faces)} faces of {len(d['verts'])} / {len(d['faces'])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=257)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "garment_timing.txt"))
    ap.add_argument("--profile-only", action="store_true", help="20 native calls and nothing else (for a kernel trace)")
    ap.add_argument("--dump", default=None, help="write the inputs as npz and stop")
    ap.add_argument("--reference-cpu", default=None, metavar="NPZ", help="time the reference's function on dumped inputs, on the CPU")
    args = ap.parse_args()
    if args.reference_cpu:
        return reference_cpu(args.reference_cpu)
    import numpy as np
    import torch
    from icon_amd import _lib, _native, garment as gm, synth
    from icon_amd.engine import IconQueryEngine
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
    body = T(np.ascontiguousarray(a.smpl_verts[0], dtype=np.float32))
    rem = (((body[:, 1] + 1.0) * 12.0).long().clamp(0, 23) % 2) == 1
    polys = polygons(np)
    polys_d = [T(p) for p in polys]
    if args.dump:
        np.savez(args.dump, verts=verts.cpu().numpy(), faces=faces.cpu().numpy(), body=body.cpu().numpy(), body_faces=a.smpl_faces[0],
                 **{f"poly_{k}": p for k, p in enumerate(polys)})
        return
    native = lambda: gm.extract_cloth_device(verts, faces, polys, body, rem, return_index=True)
    torch_way = lambda: composed(torch, verts, faces, polys_d, body, rem, chunk=2048)
    if args.profile_only:
        for _ in range(20):
            native()
        torch.cuda.synchronize()
        return
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    out_n, out_c = native(), torch_way()
    same = all(x.equal(y) for x, y in zip(out_n, out_c))
    sel = gm.extract_cloth_device(verts, torch.arange(verts.shape[0], device=dev)[:, None].expand(-1, 3).contiguous(), polys, return_index=True)
    say(f"garment extraction, {torch.cuda.get_device_name(0)}; records of ONE run, not promises")
    say(f"mesh: cleaned {args.res}^3 synthetic subject, {verts.shape[0]} vertices, {faces.shape[0]} faces ({faces.dtype}); source: {body.shape[0]} vertices, "
        f"{int(rem.sum())} removed; polygons: {[len(p) for p in polys]} vertices")
    say(f"selected {sel[2].shape[0]} vertices; garment {out_n[0].shape[0]} vertices, {out_n[1].shape[0]} faces; native == composed: {same}")
    for _ in range(3):
        native(); torch_way()
    times = {"native": [], "composed": []}
    for _ in range(args.reps):
        for name, fn in (("native", native), ("composed", torch_way)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    for name, ts in times.items():
        ts = sorted(ts)
        say(f"{name:9s} {ts[len(ts) // 2]:8.3f} ms median (min {ts[0]:.3f}, max {ts[-1]:.3f}; {len(ts)} calls, HIP events, alternated)")
    from torch.profiler import ProfilerActivity, profile
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
        say(f"{name:9s} {len(kernels)} kernel launches, {len(ev) - len(kernels)} copies / memsets per call; peak extra memory {peak / 2 ** 20:.1f} MiB"
            + (f" (outputs at the input sizes included) + {pool / 2 ** 20:.2f} MiB pooled scratch" if name == "native" else " (chunked)"))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

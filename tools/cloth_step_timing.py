#!/usr/bin/env python3
"""Times one iteration of the cloth refinement step without the renderer - forward plus backward of
10 <y, G> + 1e5 stiffness + 1e5 rigid + 1e2 laplacian + edge + nc into LocalAffine's A and b - two ways, in one
process on one GPU:

  native    icon_amd.cloth (local_affine_device + mesh_shape_prior_losses_device over csrc/cloth.hip)
  composed  the float64 oracle's statement (tests/cloth_oracle.py) run in float32 from torch operators on the same device:
            what the reference's loop costs without pytorch3d's own kernels - the only comparison this repository can run

on the clean_mesh output of the synthetic subject's dense volume (257^3: 140,716 faces) and on the synthetic body
surface.  HIP events around alternating iterations after a warm-up, median (min) ms; launches per iteration counted by
torch.profiler in a run of its own; extra memory: the caching allocator's high-water mark over one iteration plus, for the
native path, the scratch its pools hold between iterations.  The first mesh is timed a second time at the end: whatever the
first timing owes to its place in the process shows as the difference.

    python tools/cloth_step_timing.py [--res 257] [--reps 50] [--out profiles/cloth_step_timing.txt]
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloth_step_timing.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import cloth_oracle as co
    from icon_amd import _lib, synth
    from icon_amd.cloth import ClothTopology, local_affine_device, mesh_shape_prior_losses_device
    from icon_amd.engine import IconQueryEngine
    from icon_amd.recon import clean_mesh, export_mesh_device

    _lib.require_device()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def meshes():
        v, f = synth.load_body_mesh()
        yield "body", torch.from_numpy(v.astype(np.float32)).to(dev), torch.from_numpy(f.astype(np.int64)).to(dev)
        a = synth.make_assets("body")
        T = lambda x: torch.from_numpy(x).to(dev)
        eng = IconQueryEngine(prior_type="icon", sdf_clip=a.sdf_clip)
        eng.set_mesh(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
        eng.set_regressor({k: torch.from_numpy(v) for k, v in a.state_dict.items()})
        occ = eng.eval_slab(T(a.features), args.res, 0, args.res)
        v, f32 = clean_mesh(*export_mesh_device(occ, 0.5))
        half = (args.res - 1) / 2.0
        yield f"clean_mesh {args.res}^3", ((v.float() - half) / half).contiguous(), f32.long().contiguous()

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
        if not any("k_la_" in ev.key or "aten" in ev.key or "elementwise" in ev.key for ev in on_device):
            raise SystemExit(f"the profiler recorded no kernels: {sorted(ev.key for ev in on_device)[:8]}")
        return n / 5.0, other / 5.0

    def peak(fn):
        """-> MiB allocated at the high-water mark of one iteration above what was allocated before it: outputs and temporaries.
        The native path's scratch is NOT in it: it is pooled (one buffer per calling thread, device and stream, kept between
        iterations) and allocated long before - pooled_scratch() gives it"""
        fn(); torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(); torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20

    def pooled_scratch(V, E, P):
        """MiB of scratch the native path holds for this mesh: the forward calls run on the calling thread and the backward calls
        on autograd's device thread, and each thread's pool holds ONE buffer of the larger of the two queries"""
        la, mp = C.c_int64(0), C.c_int64(0)
        _lib.check(_lib.lib().icon_local_affine_bytes(C.c_int64(1), C.c_int64(V), C.c_int64(E), C.byref(la)), "icon_local_affine_bytes")
        _lib.check(_lib.lib().icon_mesh_priors_bytes(C.c_int64(V), C.c_int64(E), C.c_int64(P), C.byref(mp)), "icon_mesh_priors_bytes")
        return 2 * max(la.value, mp.value) / 2.0 ** 20

    say("one cloth iteration without the renderer: forward + backward of 10 <y,G> + 1e5 stiffness + 1e5 rigid + 1e2 laplacian + edge + nc")
    say(f"device: {torch.cuda.get_device_name(0)}; HIP events, {args.reps} alternating repetitions after 5 warm-up iterations; median (min) ms")
    say("the remeshed surface of the reference (pymeshlab, 0.5 %) is not available here: its size is unknown; these are the sizes we can build")
    todo = list(meshes())
    todo.append((todo[0][0] + ", timed again after the larger mesh",) + todo[0][1:])
    first = True
    for name, v, f in todo:
        V = v.shape[0]
        topo = ClothTopology(f, num_verts=V)
        gen = torch.Generator(device="cpu").manual_seed(7)
        x = v[None].contiguous()
        A = (torch.eye(3)[None, None] + 0.05 * torch.randn(1, V, 3, 3, generator=gen)).to(dev).requires_grad_(True)
        b = (0.02 * torch.randn(1, V, 3, 1, generator=gen)).to(dev).requires_grad_(True)
        G = torch.randn(1, V, 3, generator=gen).to(dev)
        edges, pairs = topo.edges, topo.pairs

        def native():
            y, s, r = local_affine_device(x, A, b, topo)
            e, n, l = mesh_shape_prior_losses_device(y, topo)
            return torch.autograd.grad(co.W_CLOTH * (y * G).sum() + co.W_STIFF * s + co.W_RIGID * r + co.W_LAP * l + co.W_EDGE * e + co.W_NC * n, (A, b))

        def composed():
            y, s, r = co.local_affine(x, A, b, edges)
            e, n, l = co.priors(y[0], edges, pairs)
            return torch.autograd.grad(co.W_CLOTH * (y * G).sum() + co.W_STIFF * s + co.W_RIGID * r + co.W_LAP * l + co.W_EDGE * e + co.W_NC * n, (A, b))

        scratch = pooled_scratch(V, topo.num_edges, topo.num_pairs)
        if first:                                                          # fresh pools: what one native iteration leaves allocated besides its results
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            gn = native()
            torch.cuda.synchronize()
            held = (torch.cuda.memory_allocated() - before - sum(t.numel() * 4 for t in gn)) / 2.0 ** 20
            say(f"(pooled scratch of the first mesh: {scratch:.2f} MiB by the size queries, {held:.2f} MiB left allocated by the first native iteration)")
            first = False
        for _ in range(5):
            gn, gc = native(), composed()
        torch.cuda.synchronize()
        dA = float((gn[0] - gc[0]).abs().max() / gc[0].abs().max())
        db = float((gn[1] - gc[1]).abs().max() / gc[1].abs().max())
        say()
        say(f"{name}: {V} vertices, {f.shape[0]} faces, {topo.num_edges} edges, {topo.num_pairs} face pairs; native against composed: "
            f"grad A {dA:.1e}, grad b {db:.1e} (relative, max norm)")
        (tn, tn_min), (tc, tc_min) = timed([native, composed], args.reps)
        (ln, on), (lc, oc) = launches(native), launches(composed)
        pn, pc = peak(native), peak(composed)
        say(f"  native    {tn:8.3f} ({tn_min:.3f}) ms   {ln:6.1f} kernel launches + {on:.1f} copies / fills per iteration   extra memory {pn + scratch:8.2f} MiB "
            f"({pn:.2f} outputs and temporaries + {scratch:.2f} pooled scratch)")
        say(f"  composed  {tc:8.3f} ({tc_min:.3f}) ms   {lc:6.1f} kernel launches + {oc:.1f} copies / fills per iteration   extra memory {pc:8.2f} MiB "
            f"(outputs and temporaries)")
        say(f"  -> {lc / ln:.1f} x fewer launches, {tc / tn:.1f} x in time; the native count includes the torch operators of the weighted sum and its "
            f"backward around the seven native launches")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

"""Times the soft silhouette (icon_amd.render.silhouette_device): forward, backward and forward + backward on
the synthetic SMPL-size body at 512^2 x 2 views, forward on a cleaned 257^3 marching-cubes mesh at 512^2 x 2 and x 4 views (with
the time per view), both directions on two quads whose boxes are the whole image, and the body's normal-map render beside them for scale.  HIP events, median of 30 calls
after warm-up.

    python tools/time_silhouette.py [--out profiles/silhouette_timing.txt] [--no-mc]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-mc", action="store_true")
    args = ap.parse_args()
    from icon_amd import synth
    from icon_amd.render import render_normal_device, silhouette_device
    lines = [f"device: {torch.cuda.get_device_name(0)}; HIP events, median (min .. max) of 30 calls after 5 warm-up calls, ms"]
    a = synth.make_assets("body")
    v = torch.from_numpy(a.smpl_verts[0].astype(np.float32)).cuda()
    f = torch.from_numpy(a.smpl_faces[0].astype(np.int64)).cuda()
    S = 512
    tests = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
    sys.path.insert(0, tests)
    from silhouette_oracle import smooth_field
    row = lambda what, t, per=1: lines.append(f"{what:78s} {t[0]:8.3f}  ({t[1]:.3f} .. {t[2]:.3f})" + (f"  {t[0] / per:.3f} per view" if per > 1 else ""))
    lines.append(f"synthetic body, {len(v)} vertices / {len(f)} faces, {S}^2 x 2 views (cameras 0, 2)")
    row("  normal maps with depth (render_normal_device; 4.13's record: 0.116)", median_ms(lambda: render_normal_device(v, f, (0, 2), S, return_depth=True)))
    row("  silhouette forward", median_ms(lambda: silhouette_device(v, f, (0, 2), S)))
    vg = v.clone().requires_grad_(True)
    alpha = silhouette_device(vg, f, (0, 2), S)
    ga = torch.from_numpy(smooth_field(2, S)).to(alpha)
    row("  silhouette backward (the tests' smooth seeded grad_alpha, values in [-1, 1])", median_ms(lambda: torch.autograd.grad(alpha, vg, ga, retain_graph=True)))
    target = (alpha.detach() > 0.5).float().roll(7, dims=2)

    def both():
        vg.grad = None
        (silhouette_device(vg, f, (0, 2), S) - target).abs().sum().backward()
    row("  forward + L1 loss + backward (the fit loop's use)", median_ms(both))
    # the worst case of the eight-lane backward sweep: faces whose grown box is the whole image (render_checker's quads)
    import render_checker
    qv, qf = (torch.from_numpy(x).cuda() for x in render_checker.quads())
    qg = qv.float().clone().requires_grad_(True)
    qa = silhouette_device(qg, qf, (0, 2), S)
    lines.append(f"quads, {len(qv)} vertices / {len(qf)} faces, every box the whole image, {S}^2 x 2 views")
    row("  silhouette forward", median_ms(lambda: silhouette_device(qg.detach(), qf, (0, 2), S)))
    row("  silhouette backward (the same smooth grad_alpha)", median_ms(lambda: torch.autograd.grad(qa, qg, ga, retain_graph=True)))
    if not args.no_mc:
        from icon_amd.recon import clean_mesh, export_mesh_device
        from test_gpu_parity import T, make_engine
        R = 257
        occ = make_engine(a).eval_slab(T(a.features), R, 0, R)
        mv, mf = clean_mesh(*export_mesh_device(occ, 0.5))
        mv = (mv.float() - (R - 1) / 2) / ((R - 1) / 2)
        lines.append(f"cleaned {R}^3 mesh, {len(mv)} vertices / {len(mf)} faces, {S}^2")
        row("  silhouette forward, 2 views (cameras 0, 2)", median_ms(lambda: silhouette_device(mv, mf, (0, 2), S), n=30, warm=2), 2)
        row("  silhouette forward, 4 views", median_ms(lambda: silhouette_device(mv, mf, (0, 1, 2, 3), S), n=30, warm=2), 4)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

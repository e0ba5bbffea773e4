#!/usr/bin/env python
"""End-to-end on the synthetic subject: what apps/ICON.py:test_single does after netG.filter() (lines 729-761) -
reconEngine -> export_mesh -> clean_mesh -> vertices into the [-1,1] cube - through the HIP path, with timings.

    python examples/dense_recon.py [--res 257] [--adaptive] [--color] [--normal-maps] [--turntable DIR] [--garment OUT.obj]
                                     [--out body.obj]

Needs an MI355X (there is no CPU path).  The inputs stand in for what the reference computes upstream of the hot path:
`features` = HGPIFuNet.filter() output, the SMPL tensors = TestDataset.compute_vis_cmap(), the regressor = netG.if_regressor.
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=257)
    ap.add_argument("--adaptive", action="store_true", help="the reference's coarse-to-fine schedule instead of the dense lattice")
    ap.add_argument("--out", default=None, help="write the mesh as Wavefront OBJ")
    ap.add_argument("--color", action="store_true", help="colour the vertices from a synthetic image (query_color, apps/infer.py:531); OBJ lines become v x y z r g b")
    ap.add_argument("--normal-maps", action="store_true", help="render the cleaned mesh from the four cameras of lib/common/render.py (icon_amd.render) "
                    "and write the normal maps as <out stem>_normal_<cam>.ppm")
    ap.add_argument("--turntable", metavar="DIR", default=None, help="render the cleaned mesh from 360 cameras around it (the frames of the "
                    "reference's turntable video; icon_amd.render) and write every 30th frame as DIR/turntable_<angle>.png")
    ap.add_argument("--garment", metavar="OUT.obj", default=None, help="cut a garment out of the cleaned mesh (extract_cloth, apps/infer.py:565-605; "
                    "icon_amd.garment): a fixed torso-shaped polygon, the synthetic body as the SMPL mesh with its parts split by height")
    ap.add_argument("--metrics", action="store_true", help="Chamfer, P2S and normal consistency of the dense lattice's mesh against the coarse-to-fine "
                    "schedule's (icon_amd.evaluator: the three metrics of `python -m apps.train -test`, lib/dataset/Evaluator.py)")
    args = ap.parse_args()
    import torch
    from icon_amd import synth
    from icon_amd.engine import IconQueryEngine, query_func
    from icon_amd.recon import AdaptiveReconEngine, DenseReconEngine, clean_mesh, query_color

    dev = torch.device("cuda:0")
    a = synth.make_assets("body")
    T = lambda x: torch.from_numpy(x).to(dev)
    eng = IconQueryEngine(prior_type="icon", sdf_clip=a.sdf_clip)               # or IconQueryEngine.attach(netG) on a reference network
    eng.set_mesh(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in a.state_dict.items()})
    features = [T(a.features)]
    res = args.res
    levels = [r for r in (33, 65, 129, 257, 513) if r <= res] if res in (65, 129, 257, 513) else [res]
    cls = AdaptiveReconEngine if args.adaptive else DenseReconEngine
    recon = cls(query_func=query_func, b_min=[[-1.0, 1.0, -1.0]], b_max=[[1.0, -1.0, 1.0]], resolutions=levels, align_corners=True,
                balance_value=0.5, faster=True).to(dev)
    opt = SimpleNamespace(num_views=1)

    def sync():
        torch.cuda.synchronize(); return time.perf_counter()
    w = recon(opt=opt, netG=eng, features=features, proj_matrix=None)          # warm-up: BVH build, operand packing, workspaces,
    clean_mesh(*recon.export_mesh(w))                                           # ... and the marching-cubes / clean_mesh scratch
    t0 = sync()
    sdf = recon(opt=opt, netG=eng, features=features, proj_matrix=None)
    t1 = sync()
    verts, faces = recon.export_mesh(sdf)                                       # marching cubes on the GPU, CPU tensors out (as upstream)
    t2 = sync()
    verts, faces = clean_mesh(verts, faces)                                     # largest component (apps/ICON.py:755-756)
    t3 = sync()
    half = (res - 1) / 2.0
    verts = (verts.float() - half) / half                                       # apps/ICON.py:758-759
    colors, color_ms = None, ""
    if args.color:
        import numpy as np
        image = torch.from_numpy(np.tanh(synth.make_feature_planes(3, 512, 531)).astype(np.float32))    # stands in for the input photograph, in [-1,1]
        query_color(verts, faces, image)                                        # warm-up: the call's scratch
        t4 = sync()
        colors = query_color(verts, faces, image)                               # [V,3] 0..255 on the CPU, as upstream
        color_ms = f", query_color {1e3 * (sync() - t4):.2f} ms"
    print(f"{'adaptive' if args.adaptive else 'dense'} {res}^3: volume {1e3 * (t1 - t0):.2f} ms, marching cubes {1e3 * (t2 - t1):.2f} ms, "
          f"clean_mesh {1e3 * (t3 - t2):.2f} ms{color_ms} -> {verts.shape[0]} vertices, {faces.shape[0]} faces, "
          f"bbox {verts.min(0).values.tolist()} .. {verts.max(0).values.tolist()}")
    if args.normal_maps:
        from icon_amd.render import Render
        render = Render(size=512, device=dev)
        render.load_meshes(verts, faces)
        render.get_rgb_image(cam_ids=[0, 1, 2, 3])                               # warm-up: the call's scratch
        render.load_meshes(verts, faces)
        t5 = sync()
        maps = render.get_rgb_image(cam_ids=[0, 1, 2, 3])                        # four [1,3,512,512] tensors in [-1,1], on the device
        print(f"render: four 512^2 normal maps in {1e3 * (sync() - t5):.2f} ms (mesh upload included)")
        stem = os.path.splitext(args.out)[0] if args.out else "dense_recon"
        for cam, m in enumerate(maps):
            rgb = ((m[0].permute(1, 2, 0) + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8).cpu().numpy()
            with open(f"{stem}_normal_{cam}.ppm", "wb") as fh:
                fh.write(b"P6\n512 512\n255\n" + rgb.tobytes())
        print(f"wrote {stem}_normal_0.ppm .. {stem}_normal_3.ppm")
    if args.turntable:
        from PIL import Image
        from icon_amd.render import Render
        render = Render(size=512, device=dev)
        render.load_meshes(verts, faces)
        for _ in render.get_rendered_frames([]):                                # warm-up: the call's scratch
            pass
        t6 = sync()
        chunks = list(render.get_rendered_frames([]))                           # 12 uint8 [30,512,512,3] tensors on the device
        print(f"turntable: 360 frames of 512^2 in {1e3 * (sync() - t6):.2f} ms, left on the device")
        os.makedirs(args.turntable, exist_ok=True)
        for k, frames in enumerate(chunks):                                     # the reference hands the frame to the writer as it is
            Image.fromarray(frames[0].cpu().numpy()).save(os.path.join(args.turntable, f"turntable_{30 * k:03d}.png"))
        print(f"wrote {args.turntable}/turntable_000.png .. turntable_330.png")
    if args.garment:
        import numpy as np
        from icon_amd.garment import Garment, extract_cloth_device
        torso = np.array([[-0.2, 0.5], [0.0, 0.42], [0.2, 0.5], [0.24, 0.1], [0.18, -0.3], [-0.18, -0.3], [-0.24, 0.1]])   # model plane: what
        body = T(a.smpl_verts[0])                                                # polygons_to_model_plane makes of a segmentation
        band = ((body[:, 1] + 1.0) * 4.0).long().clamp(0, 7)                     # eight "parts" by height; the bands 4 and 6 (shoulders, head) go
        remove = (band == 4) | (band == 6)
        v_d, f_d = verts.to(dev), faces.to(dev)
        extract_cloth_device(v_d, f_d, [torso], body, remove)                    # warm-up: the call's scratch
        t7 = sync()
        out = extract_cloth_device(v_d, f_d, [torso], body, remove, return_index=True)
        ms = 1e3 * (sync() - t7)
        if out is None:
            print(f"garment: no face kept ({ms:.2f} ms)")
        else:
            Garment(*(x.cpu().numpy() for x in out)).export(args.garment)
            print(f"garment: {out[0].shape[0]} vertices, {out[1].shape[0]} faces of {verts.shape[0]} / {faces.shape[0]} in {ms:.2f} ms; wrote {args.garment}")
    if args.metrics:
        from icon_amd.evaluator import EvalMesh, Evaluator
        other_cls = DenseReconEngine if args.adaptive else AdaptiveReconEngine
        other = other_cls(query_func=query_func, b_min=[[-1.0, 1.0, -1.0]], b_max=[[1.0, -1.0, 1.0]], resolutions=levels, align_corners=True,
                          balance_value=0.5, faster=True).to(dev)
        ov, of = clean_mesh(*other.export_mesh(other(opt=opt, netG=eng, features=features, proj_matrix=None)))
        ov = (ov.float() - half) / half
        meshes = [EvalMesh(verts.to(dev), faces.to(dev)), EvalMesh(ov.to(dev), of.to(dev))]
        dense, sched = meshes[::-1] if args.adaptive else meshes
        ev = Evaluator(dev)
        ev.set_mesh({}, scale_factor=1.0)
        ev.src_mesh, ev.tgt_mesh = dense, sched                                  # both are in the [-1,1] cube already: no space_transfer
        ev.calculate_normal_consist()                                           # warm-up: the call's scratch
        t8 = sync()
        nc = ev.calculate_normal_consist()                                      # one native call, four 512^2 views of both meshes
        nc_ms = 1e3 * (sync() - t8)
        chamfer, p2s = ev.calculate_chamfer_p2s()
        print(f"metrics, dense ({dense.vertices.shape[0]} vertices) against the schedule's mesh ({sched.vertices.shape[0]}): chamfer {chamfer:.4f}, "
              f"p2s {p2s:.4f}, normal consistency {nc:.6f} ({nc_ms:.2f} ms)")
    if args.out:
        v, f = verts.cpu().numpy(), faces.cpu().numpy() + 1
        with open(args.out, "w") as fh:
            if colors is None:
                fh.writelines(f"v {x:.6f} {y:.6f} {z:.6f}\n" for x, y, z in v)
            else:                                                               # the common "v x y z r g b" extension, colours in 0..1
                fh.writelines(f"v {x:.6f} {y:.6f} {z:.6f} {r:.6f} {g:.6f} {b:.6f}\n" for (x, y, z), (r, g, b) in zip(v, colors.numpy() / 255.0))
            fh.writelines(f"f {i} {j} {k}\n" for i, j, k in f)
        print("wrote", args.out)


if __name__ == "__main__":
    main()

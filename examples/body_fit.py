#!/usr/bin/env python
"""The body-fit loop of apps/infer.py:163-273 on the synthetic subject, with nothing but this package: every step goes from the
optimised parameters through an attached SMPL-style module (icon_amd.smpl: native skinning with gradients), ``* [1, -1, -1]`` and
``Render(normal_grad=True)`` to L1 terms on the normal maps and the silhouette, and steps Adam.

    python examples/body_fit.py [--steps 50] [--size 512]

Needs an MI355X (there is no CPU path).  The body model is synthetic: the synthetic subject as the template, 24 joints on
SMPL's kinematic tree regressed from slices of it, smooth weights on the four nearest joints, small random blend shapes.  The
target maps are rendered from known parameters; the loop starts from perturbed ones.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)


def synthetic_body(verts, num_betas=10, seed=0):
    """an smplx-style module (the six buffers, SMPL's parameters, a joint selector) around the template ``verts [V,3]``"""
    import torch
    V, J = verts.shape[0], len(SMPL_PARENTS)
    gen = torch.Generator().manual_seed(seed)
    order = torch.argsort(verts[:, 1])                                     # slices by height: joint j is the mean of slice j
    J_regressor = torch.zeros(J, V)
    for j, idx in enumerate(torch.tensor_split(order, J)):
        J_regressor[j, idx] = 1.0 / len(idx)
    d2 = torch.cdist(verts, J_regressor @ verts) ** 2
    near = torch.topk(d2, 4, dim=1, largest=False)
    w = torch.softmax(-near.values / 0.01, dim=1)
    lbs_weights = torch.zeros(V, J).scatter_(1, near.indices, w)

    class Body(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.register_buffer("v_template", verts.clone())
            self.register_buffer("shapedirs", 0.01 * torch.randn(V, 3, num_betas, generator=gen))
            self.register_buffer("posedirs", 0.002 * torch.randn(9 * (J - 1), 3 * V, generator=gen))
            self.register_buffer("J_regressor", J_regressor)
            self.register_buffer("parents", torch.tensor(SMPL_PARENTS))
            self.register_buffer("lbs_weights", lbs_weights)
            self.betas = torch.nn.Parameter(torch.zeros(1, num_betas))
            self.global_orient = torch.nn.Parameter(torch.zeros(1, 3))
            self.body_pose = torch.nn.Parameter(torch.zeros(1, 3 * (J - 1)))
            self.joint_mapper = None

        def vertex_joint_selector(self, vertices, joints):
            return joints

        def forward(self, **kwargs):
            raise RuntimeError("this stand-in has no forward of its own: icon_amd.smpl.attach gives it one")

    return Body()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    import torch
    from icon_amd import synth
    from icon_amd.render import Render
    from icon_amd.smpl import attach, batch_rodrigues

    dev = torch.device("cuda:0")
    a = synth.make_assets("body")
    faces = torch.from_numpy(a.smpl_faces[0]).to(dev)
    smpl_model = synthetic_body(torch.from_numpy(a.smpl_verts[0]).float()).to(dev)
    attach(smpl_model)                                                     # on a reference checkout: attach(dataset.smpl_model)
    render = Render(size=args.size, device=dev, normal_grad=True)
    flip = torch.tensor([1.0, -1.0, -1.0], device=dev)
    J = len(SMPL_PARENTS)

    def maps(betas, pose, orient, trans):
        out = smpl_model(betas=betas, body_pose=pose, global_orient=orient, pose2rot=False)
        render.load_meshes((out.vertices + trans) * flip, faces)
        return render.get_rgb_image(), render.get_silhouette_image()

    gen = torch.Generator().manual_seed(1)
    true_betas = (0.5 * torch.randn(1, 10, generator=gen)).to(dev)
    true_rot = batch_rodrigues(0.1 * torch.randn(J, 3, generator=gen)).view(1, J, 3, 3).to(dev)
    true_trans = torch.tensor([[0.01, 0.02, 0.0]], device=dev)
    with torch.no_grad():
        (gt_F, gt_B), (gt_mF, gt_mB) = maps(true_betas, true_rot[:, 1:], true_rot[:, :1], true_trans)
        gt_F, gt_B, gt_mF, gt_mB = (t.clone() for t in (gt_F, gt_B, gt_mF, gt_mB))
    # infer.py hands the rotation matrices themselves to Adam
    eye = torch.eye(3, device=dev)
    optimed_betas = torch.zeros(1, 10, device=dev, requires_grad=True)
    optimed_pose = eye.expand(1, J - 1, 3, 3).clone().requires_grad_(True)
    optimed_orient = eye.expand(1, 1, 3, 3).clone().requires_grad_(True)
    optimed_trans = torch.zeros(1, 3, device=dev, requires_grad=True)
    opt = torch.optim.Adam([optimed_betas, optimed_pose, optimed_orient, optimed_trans], lr=1e-2, amsgrad=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        opt.zero_grad()
        (nF, nB), (mF, mB) = maps(optimed_betas, optimed_pose, optimed_orient, optimed_trans)
        normal = ((nF - gt_F).abs() + (nB - gt_B).abs()).mean()
        silhouette = (torch.cat([mF, mB], dim=-1) - torch.cat([gt_mF, gt_mB], dim=-1)).abs().mean()
        loss = 1e0 * normal + 1e1 * silhouette
        loss.backward()
        opt.step()
        if i % 10 == 0 or i == args.steps - 1:
            print(f"step {i:3d}: normal {normal.item():.5f}  silhouette {silhouette.item():.5f}  total {loss.item():.5f}")
    torch.cuda.synchronize()
    print(f"{args.steps} steps at {args.size}^2 in {1e3 * (time.perf_counter() - t0):.1f} ms; |betas - true| "
          f"{(optimed_betas - true_betas).abs().max().item():.3f}, |trans - true| {(optimed_trans - true_trans).abs().max().item():.4f}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""A training step of the implicit function on the device, with nothing but this package: synthetic subjects, samples and labels
from ``sample_geo_device``, a one-convolution stand-in for the hourglass filter (so that the feature planes need a gradient),
``icon_amd.training.attach`` as the network's ``query``, MSE against the labels and Adam - the shape of ``ICON.training_step``
(apps/ICON.py:178-236): ``netG.train()``, ``netG(in_tensor_dict)`` = filter -> query -> get_error, backward, step.

    python examples/train_step.py [--steps 40] [--batch 2] [--points 2000] [--prior icon|pifu]

Needs an MI355X (there is no CPU path).  ``StandInNet`` follows HGPIFuNet's interface as far as the step uses it; its regressor
is lib/net/MLP.py restated (Conv1d stack, norm per ``norm``, LeakyReLU, the input re-concatenated before ``res_layers``)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

ALL_FEATS = ("sdf", "norm", "vis", "cmap")


class Regressor(nn.Module):
    """lib/net/MLP.py:8-72: ``filters`` / ``norms`` ModuleLists with the reference's state_dict keys; norm 'batch', 'group',
    'instance', 'weight' or None; last_op a module or None"""

    def __init__(self, dims=(13, 512, 256, 128, 1), res_layers=(2, 3, 4), norm="batch", last_op=None):
        super().__init__()
        self.filters, self.norms = nn.ModuleList(), nn.ModuleList()
        self.res_layers, self.norm, self.last_op = list(res_layers), norm, last_op
        for l in range(len(dims) - 1):
            conv = nn.Conv1d(dims[l] + (dims[0] if l in self.res_layers else 0), dims[l + 1], 1)
            self.filters.append(nn.utils.weight_norm(conv) if norm == "weight" else conv)
            if l != len(dims) - 2:
                if norm == "batch":
                    self.norms.append(nn.BatchNorm1d(dims[l + 1]))
                elif norm == "group":
                    self.norms.append(nn.GroupNorm(32, dims[l + 1]))
                elif norm == "instance":
                    self.norms.append(nn.InstanceNorm1d(dims[l + 1]))

    def forward(self, feature):
        y, x = feature, feature
        for i, f in enumerate(self.filters):
            y = f(y if i not in self.res_layers else torch.cat([y, x], 1))
            if i != len(self.filters) - 1:
                y = F.leaky_relu(self.norms[i](y) if len(self.norms) else y, 0.01)
        return self.last_op(y) if self.last_op is not None else y


class StandInNet(nn.Module):
    """HGPIFuNet as far as a training step uses it: ``filter`` (one 3x3 convolution giving ``num_stack`` stacks of ``channels``
    planes; ``use_filter=False``: the input maps themselves, one stack), ``query`` (replaced by ``icon_amd.training.attach``),
    ``get_error`` and ``forward`` (lib/net/HGPIFuNet.py:369-410)"""

    def __init__(self, prior_type="icon", smpl_feats=ALL_FEATS, channels=12, num_stack=2, use_filter=True, sdf_clip=0.05,
                 norm="batch", in_channels=6):
        super().__init__()
        self.prior_type, self.smpl_feats, self.sdf_clip = prior_type, list(smpl_feats), sdf_clip
        self.use_filter, self.num_stack, self.channels = use_filter, (num_stack if use_filter else 1), (channels if use_filter else in_channels)
        self.F_filter = nn.Conv2d(in_channels, channels * num_stack, 3, padding=1) if use_filter else None
        if prior_type == "icon":
            img = self.channels // 2 if "vis" in smpl_feats else self.channels
            c0 = img + 1 + (3 if "cmap" in smpl_feats else 0) + (3 if "norm" in smpl_feats else 0)
        else:
            c0 = self.channels + 1
        self.if_regressor = Regressor((c0, 512, 256, 128, 1), norm=norm, last_op=nn.Sigmoid())
        self.error_term = nn.MSELoss()
        self.smpl_feat_dict = None

    def filter(self, in_tensor_dict):
        x = in_tensor_dict["image"]
        if self.prior_type == "icon":
            self.smpl_feat_dict = {k: in_tensor_dict[k] for k in ("smpl_verts", "smpl_faces", "smpl_vis", "smpl_cmap")}
        if not self.use_filter:
            return [x]
        stacks = list(torch.tanh(self.F_filter(x)).split(self.channels, dim=1))
        return stacks if self.training else stacks[-1:]

    def query(self, features, points, calibs, transforms=None, regressor=None):
        raise RuntimeError("StandInNet has no query of its own: icon_amd.training.attach gives it one")

    def get_error(self, preds_if_list, labels):
        return sum(self.error_term(p, labels) for p in preds_if_list) / len(preds_if_list)

    def forward(self, in_tensor_dict):
        in_feat = self.filter(in_tensor_dict)
        preds = self.query(in_feat, in_tensor_dict["sample"], in_tensor_dict["calib"], regressor=self.if_regressor)
        return preds[-1], self.get_error(preds, in_tensor_dict["label"])


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def make_batch(B, N, device, seed=0, size=128, in_channels=6):
    """B synthetic subjects (the synthetic body moved, scaled and re-lit per subject, its own calibration), N samples each with
    labels from ``sample_geo_device`` (the body is its own scan here), smooth random input maps -> the step's ``in_tensor_dict``"""
    from icon_amd import synth
    from icon_amd.sampling import ScanMesh, sample_geo_device
    v0, f = synth.load_body_mesh()
    v0 = v0.astype(np.float64)
    c = 0.5 * (v0.min(0) + v0.max(0))
    rng = np.random.RandomState(seed + 4242)
    d = {k: [] for k in ("smpl_verts", "smpl_faces", "smpl_vis", "smpl_cmap", "calib", "sample", "label", "image")}
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    for b in range(B):
        ay, s, t = rng.uniform(-0.6, 0.6), rng.uniform(0.85, 1.05), rng.uniform(-0.06, 0.06, 3)
        v = (((v0 - c) @ _rot(1, ay).T) * s + c + t).astype(np.float32)
        vis, cmap = synth.make_vis_cmap(v, f)
        K = np.eye(4)
        K[:3, :3] = rng.uniform(0.9, 1.1) * _rot(2, rng.uniform(-0.15, 0.15))
        K[:3, 3] = rng.uniform(-0.03, 0.03, 3)
        # the body the query searches lives in the projected space (HGPIFuNet.query projects the points, not the body); the scan the
        # samples are drawn around is the same surface in world space, and calib takes it into the image cube
        Kinv = np.linalg.inv(K)
        scan = ScanMesh(T((v.astype(np.float64) @ Kinv[:3, :3].T + Kinv[:3, 3]).astype(np.float32)), T(f))
        samples, labels, _ = sample_geo_device(scan, K, N, 0.05, seed=seed * 1000 + b)
        d["smpl_verts"].append(T(v)); d["smpl_faces"].append(T(f)); d["smpl_vis"].append(T(vis)); d["smpl_cmap"].append(T(cmap))
        d["calib"].append(T(K.astype(np.float32))); d["sample"].append(samples.t().contiguous()); d["label"].append(labels[None])
        d["image"].append(T(synth.make_feature_planes(in_channels, size, synth.SEED + 97 * b + seed)[0]))
    return {k: torch.stack(v) for k, v in d.items()}


def train_step(netG, optimizer, batch):
    """ICON.training_step without the logging (apps/ICON.py:178-236) -> the error (a device scalar: nothing is read back)"""
    netG.train()
    optimizer.zero_grad(set_to_none=True)
    _, error = netG(batch)
    error.backward()
    optimizer.step()
    return error.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--prior", default="icon", choices=("icon", "pifu"))
    ap.add_argument("--lr", type=float, default=1e-3)
    args = ap.parse_args()
    from icon_amd import _lib, training
    _lib.require_device()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    netG = StandInNet(prior_type=args.prior).to(dev)
    training.attach(netG)
    opt = torch.optim.Adam(netG.parameters(), lr=args.lr)
    batch = make_batch(args.batch, args.points, dev)
    print(f"{args.prior}: B = {args.batch}, N = {args.points}, inside {float(batch['label'].mean()):.3f}")
    errors = [train_step(netG, opt, batch) for _ in range(args.steps)]
    for k, e in enumerate(torch.stack(errors).tolist()):
        print(f"step {k:3d}  error {e:.6f}")
    netG.eval()
    with torch.no_grad():
        pred, _ = netG(batch)
    acc = float(((pred > 0.5).float() == batch["label"]).float().mean())
    print(f"eval-mode query() after training: accuracy {acc:.3f}")


if __name__ == "__main__":
    main()

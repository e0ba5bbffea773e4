#!/usr/bin/env python
"""A training step of the implicit function on the device, with nothing but this package: synthetic subjects, samples and labels
from ``sample_geo_device``, a one-convolution stand-in for the hourglass filter (so that the feature planes need a gradient),
``icon_amd.training.attach`` as the network's ``query``, MSE against the labels and Adam - the shape of ``ICON.training_step``
(apps/ICON.py:178-236): ``netG.train()``, ``netG(in_tensor_dict)`` = filter -> query -> get_error, backward, step.

    python examples/train_step.py [--steps 40] [--batch 2] [--points 2000] [--prior icon|pifu|pamir]

Needs an MI355X (there is no CPU path).  ``StandInNet`` follows HGPIFuNet's interface as far as the step uses it; its regressor
is lib/net/MLP.py restated (Conv1d stack, norm per ``norm``, LeakyReLU, the input re-concatenated before ``res_layers``).
``PamirStandInNet`` adds what the pamir prior's step uses: the voxel tensors in ``smpl_feat_dict``, a small volume encoder ``ve`` whose
parameters the optimizer owns, and the ``voxelization`` attributes the semantic voxeliser reads."""
import argparse
import os
import sys
from types import SimpleNamespace

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


class SmallVolumeEncoder(nn.Module):
    """A volume encoder of VolumeEncoder's call contract (``ve(vol, intermediate_output)`` -> one [B,Cv,res/4,res/4,res/4] volume per
    stack, or the last one alone): two stride-2 Conv3d + BatchNorm3d + ReLU, then per stack a residual Conv3d + BatchNorm3d block.
    Every parameter takes part in the output of the last stack."""

    def __init__(self, num_in=3, num_out=7, num_stack=2, width=8):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv3d(num_in, width, 3, stride=2, padding=1), nn.BatchNorm3d(width)
        self.conv2, self.bn2 = nn.Conv3d(width, num_out, 3, stride=2, padding=1), nn.BatchNorm3d(num_out)
        self.res = nn.ModuleList(nn.Sequential(nn.Conv3d(num_out, num_out, 3, padding=1), nn.BatchNorm3d(num_out)) for _ in range(num_stack))

    def forward(self, x, intermediate_output=True):
        out = F.relu(self.bn2(self.conv2(F.relu(self.bn1(self.conv1(x))))))
        outs = []
        for block in self.res:
            out = out + torch.tanh(block(out))
            outs.append(out)
        return outs if intermediate_output else outs[-1:]


class PamirStandInNet(StandInNet):
    """StandInNet for ``prior_type='pamir'`` (configs/train/pamir.yaml: hourglass_dim 6, voxel_dim 7, num_stack 2): ``filter`` also
    binds the four voxel tensors, ``ve`` is a SmallVolumeEncoder, ``voxelization`` carries what the semantic voxeliser reads (the
    surface vertices' code, the volume's resolution, sigma) and the regressor takes ``[img | vol]`` = channels + vol_channels."""

    def __init__(self, vertex_code, channels=6, vol_channels=7, num_stack=2, volume_res=128, sigma=0.05, norm="batch", in_channels=6):
        super().__init__(prior_type="pamir", smpl_feats=(), channels=channels, num_stack=num_stack, norm=norm, in_channels=in_channels)
        self.if_regressor = Regressor((channels + vol_channels, 512, 256, 128, 1), norm=norm, last_op=nn.Sigmoid())
        self.ve = SmallVolumeEncoder(3, vol_channels, num_stack)
        self.voxelization = SimpleNamespace(smpl_vertex_code=np.asarray(vertex_code, np.float32), volume_res=volume_res, sigma=sigma)

    def filter(self, in_tensor_dict):
        self.smpl_feat_dict = {k: in_tensor_dict[k] for k in ("voxel_verts", "voxel_faces", "pad_v_num", "pad_f_num")}
        return super().filter(in_tensor_dict)


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def make_batch(B, N, device, seed=0, size=128, in_channels=6, prior="icon"):
    """B synthetic subjects (the synthetic body moved, scaled and re-lit per subject, its own calibration), N samples each with
    labels from ``sample_geo_device`` (the body is its own scan here), smooth random input maps -> the step's ``in_tensor_dict``.
    ``prior='pamir'``: also the tetrahedralised body of every subject (``synth.make_tetra_body``) padded as a batch delivers it -
    ``voxel_verts`` / ``voxel_faces`` with pad counts that differ across subjects - and ``vertex_code``, the surface code table"""
    from icon_amd import synth
    from icon_amd.sampling import ScanMesh, sample_geo_device
    v0, f = synth.load_body_mesh()
    v0 = v0.astype(np.float64)
    c = 0.5 * (v0.min(0) + v0.max(0))
    rng = np.random.RandomState(seed + 4242)
    d = {k: [] for k in ("smpl_verts", "smpl_faces", "smpl_vis", "smpl_cmap", "calib", "sample", "label", "image")}
    tetra = []
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
        if prior == "pamir":
            tetra.append(synth.make_tetra_body(v, f, cmap))
    out = {k: torch.stack(v) for k, v in d.items()}
    if prior == "pamir":
        # subject b carries pad counts of its own; the reference strips every subject with subject 0's (lib/net/HGPIFuNet.py:316-319)
        pad_v, pad_f = [5 + 2 * (b % 3) for b in range(B)], [9 - 3 * (b % 3) for b in range(B)]
        vv = np.stack([np.concatenate([t[0], np.zeros((pad_v[0], 3), np.float32)]) for t in tetra]).astype(np.float32)
        tets = np.concatenate([tetra[0][1], np.zeros((pad_f[0], 4), np.int64)])
        out.update(voxel_verts=T(vv), voxel_faces=T(np.repeat(tets[None], B, 0)), pad_v_num=T(np.asarray(pad_v, np.int64)),
                   pad_f_num=T(np.asarray(pad_f, np.int64)), vertex_code=T(tetra[0][2]))
    return out


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
    ap.add_argument("--prior", default="icon", choices=("icon", "pifu", "pamir"))
    ap.add_argument("--lr", type=float, default=1e-3)
    args = ap.parse_args()
    from icon_amd import _lib, training
    _lib.require_device()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    batch = make_batch(args.batch, args.points, dev, prior=args.prior)
    if args.prior == "pamir":
        netG = PamirStandInNet(batch["vertex_code"].cpu().numpy()).to(dev)
        training.attach(netG, voxelizer="hip")
    else:
        netG = StandInNet(prior_type=args.prior).to(dev)
        training.attach(netG)
    opt = torch.optim.Adam(netG.parameters(), lr=args.lr)
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

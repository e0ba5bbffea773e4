"""The training step's ``query()``: ``HGPIFuNet.query`` with the network in TRAIN mode (``lib/net/HGPIFuNet.py:268-367``, reached from
``ICON.training_step``, ``apps/ICON.py:178-236``, through ``netG.forward``) for the ``icon`` and ``pifu`` priors.

What is native is everything in front of the regressor (csrc/train_rows.hip): ``point_feat`` of EVERY feature stack
from one search (``icon_train_rows_forward``) and the gradient of those rows into the feature planes, without floating-point
atomics (``icon_train_rows_backward``).  The regressor stays the module's own PyTorch layers: train-mode BatchNorm reduces over all
B * N points between every pair of layers, updates its running statistics, and its parameters are the optimizer's leaves.

There is no gradient for the points, the calibrations, the SMPL tensors, the sdf / cmap / norm / z channels or ``in_cube``: the
reference detaches or never differentiates them.  ``attach(netG)`` installs a ``query`` that takes this path while the regressor
in use is in training mode and ``IconQueryEngine.query`` - untouched - otherwise.
"""
from __future__ import annotations

import ctypes as C
import sys
from typing import Sequence

import numpy as np
import torch

from . import _lib
from ._lib import IconAmdError, check
from ._native import scratch_for, stream

_WHAT = "point_features_device"


def _native_forward(eng, stacks, pts, calib12):
    """(rows [S,B,Cin,N], in_cube [B,1,N], taps [B*N,4] int32) of contiguous float32 device tensors: one native call"""
    S = len(stacks)
    B, Cc, H, W = (int(x) for x in stacks[0].shape)
    N = int(pts.shape[1])
    icon = eng.prior_type == "icon"
    feats = tuple(eng.smpl_feats) if icon else ()
    csel = Cc // 2 if "vis" in feats else Cc
    cin = csel + 1 + (3 if "cmap" in feats else 0) + (3 if "norm" in feats else 0)
    dev = pts.device
    mb = eng._mesh_batch_handle(B) if icon else None
    rows = torch.empty((S, B, cin, N), dtype=torch.float32, device=dev)
    in_cube = torch.empty((B, 1, N), dtype=torch.float32, device=dev)
    taps = torch.empty((B * N, 4), dtype=torch.int32, device=dev)
    ptrs = (C.c_void_p * S)(*[t.data_ptr() for t in stacks])
    shapes = (C.c_int32 * (4 * S))(*[int(x) for t in stacks for x in t.shape])
    check(_lib.lib().icon_train_rows_forward(
        mb.h if mb is not None else C.c_void_p(0), C.c_int(_lib.PRIOR[eng.prior_type]), C.c_float(np.float32(eng.sdf_clip)),
        C.c_int(_lib.CMAP[eng.cmap_mode]), C.c_int(int("vis" in feats)), C.c_int(int("cmap" in feats)), C.c_int(int("norm" in feats)),
        ptrs, shapes, C.c_int(S), _lib.ptr(calib12), _lib.ptr(pts), C.c_int64(N), _lib.ptr(rows), _lib.ptr(in_cube), _lib.ptr(taps),
        C.c_int(_lib.SEARCH[eng.search]), eng._work().h, stream()), "icon_train_rows_forward")
    return rows, in_cube, taps


def _native_backward(grad_rows, taps, shape, n_select: int, mask: int, out=None):
    """grad_planes [S,B,C,H,W]: the stacks whose bit of ``mask`` is set are written, element by element (``out``: into this tensor)"""
    S, B, Cc, H, W = shape
    cin, N = int(grad_rows.shape[2]), int(grad_rows.shape[3])
    dev = grad_rows.device
    L = _lib.lib()
    scratch = scratch_for(dev, "icon_train_rows_bytes", C.c_int(B), C.c_int64(N), C.c_int(S), C.c_int(Cc), C.c_int(H), C.c_int(W))   # autograd's thread has its own
    grad_planes = torch.empty((S, B, Cc, H, W), dtype=torch.float32, device=dev) if out is None else out
    check(L.icon_train_rows_backward(_lib.ptr(grad_rows), _lib.ptr(taps), C.c_int(S), C.c_uint32(mask), C.c_int(B), C.c_int(cin),
                                     C.c_int(Cc), C.c_int(H), C.c_int(W), C.c_int(n_select), C.c_int64(N), _lib.ptr(grad_planes),
                                     _lib.ptr(scratch), C.c_int64(scratch.numel()), stream()), "icon_train_rows_backward")
    return grad_planes


class _TrainRowsFn(torch.autograd.Function):
    """(engine, pts [B,N,3], calib12 [B,12], *stacks [B,C,H,W]) -> rows [S,B,Cin,N], in_cube [B,1,N]"""

    @staticmethod
    def forward(ctx, eng, pts, calib12, *stacks):
        with torch.cuda.device(pts.device):
            rows, in_cube, taps = _native_forward(eng, stacks, pts, calib12)
        ctx.save_for_backward(taps)
        ctx.shape = (len(stacks),) + tuple(int(x) for x in stacks[0].shape)
        ctx.n_select = 2 if (eng.prior_type == "icon" and "vis" in eng.smpl_feats) else 1
        ctx.mark_non_differentiable(in_cube)
        return rows, in_cube

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rows, _g_in_cube):
        S = ctx.shape[0]
        needs = ctx.needs_input_grad[3:]
        mask = sum(1 << s for s in range(S) if needs[s])
        if mask == 0 or g_rows is None:                              # use_filter False: the stacks are the input normal maps
            return (None,) * (3 + S)
        (taps,) = ctx.saved_tensors
        with torch.cuda.device(g_rows.device):
            gp = _native_backward(g_rows.to(torch.float32).contiguous(), taps, ctx.shape, ctx.n_select, mask)
        return (None, None, None) + tuple(gp[s] if needs[s] else None for s in range(S))


def _check_call(eng, features, points, calibs, transforms=None) -> None:
    if eng.prior_type == "pamir":
        raise IconAmdError(f"{_WHAT}: prior_type 'pamir' is not trained here - the gradient into the volume encoder's planes is not "
                           "implemented (icon and pifu are)")
    if transforms is not None:
        raise IconAmdError(f"{_WHAT}: transforms is not supported - the reference's own orthogonal() raises for any `transforms` "
                           "(lib/net/geometry.py:57-60)")
    if getattr(points, "requires_grad", False):
        raise IconAmdError(f"{_WHAT}: points.requires_grad is set - there is no gradient for the points (the reference's training never asks for one)")
    if getattr(calibs, "requires_grad", False):
        raise IconAmdError(f"{_WHAT}: calibs.requires_grad is set - there is no gradient for the calibrations")
    if not isinstance(features, (list, tuple)) or len(features) == 0:
        raise IconAmdError(f"{_WHAT}: features must be a non-empty list of [B,C,H,W] tensors")
    for name, t in (("points", points), ("calibs", calibs)) + tuple((f"features[{s}]", f) for s, f in enumerate(features)):
        if not torch.is_tensor(t):
            raise IconAmdError(f"{_WHAT}: {name} must be a tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise IconAmdError(f"{_WHAT}: {name} is a CPU tensor; icon_amd has no CPU path - move it to the HIP device")
    if points.dim() != 3 or points.shape[1] != 3 or points.shape[0] < 1 or points.shape[2] < 1:
        raise IconAmdError(f"{_WHAT}: points must be [B,3,N] with N >= 1, got {tuple(points.shape)}")
    B, n = int(points.shape[0]), int(points.shape[2])
    if calibs.dim() != 3 or int(calibs.shape[0]) != B or tuple(calibs.shape[1:]) not in ((4, 4), (3, 4)):
        raise IconAmdError(f"{_WHAT}: calibs {tuple(calibs.shape)} must be [{B},4,4] or [{B},3,4]")
    shape0 = tuple(features[0].shape)
    for s, f in enumerate(features):
        if f.dim() != 4 or int(f.shape[0]) != B:
            raise IconAmdError(f"{_WHAT}: feature stack {s} {tuple(f.shape)} must be [{B},C,H,W]")
        if tuple(f.shape) != shape0:
            raise IconAmdError(f"{_WHAT}: feature stacks differ in shape ({shape0} and {tuple(f.shape)}): one call covers stacks of one shape")
    if B * n >= 2 ** 31:
        raise IconAmdError(f"{_WHAT}: B * N = {B * n}: a call holds fewer than 2^31 points")
    if eng.search == "brute":
        raise IconAmdError(f"{_WHAT}: search='brute' (validation path) is evaluated at batch size 1 only")
    if eng.tie_rule is not None:
        raise IconAmdError(f"{_WHAT}: tie_rule (diagnostics) is evaluated at batch size 1 only")


def point_features_device(engine, features: Sequence[torch.Tensor], points: torch.Tensor, calibs: torch.Tensor, transforms=None):
    """``point_feat`` of ``HGPIFuNet.query`` (:329-359) for every stack of ``features`` (list of [B,C,H,W], one shape) at ``points``
    [B,3,N] under ``calibs`` [B,4,4] -> ``(rows_list, in_cube)``: S views [B,Cin,N] of one tensor, channels ``[img | sdf | cmap |
    norm]`` (icon, per ``engine.smpl_feats``) or ``[img | z]`` (pifu), and ``in_cube`` [B,1,N] (:274-275).  Differentiable in the
    feature stacks only; a stack that does not need a gradient costs the backward nothing, and when none does no backward call is
    made.  One native call each way on the current stream, nothing read back; equal bytes from run to run."""
    _check_call(engine, features, points, calibs, transforms)
    with torch.cuda.device(points.device):
        calib12 = calibs[:, :3, :4].detach().to(points.device, torch.float32).reshape(calibs.shape[0], 12).contiguous()
        pts = points.detach().transpose(1, 2).to(torch.float32).contiguous()
        stacks = [f.to(torch.float32).contiguous() for f in features]
        rows, in_cube = _TrainRowsFn.apply(engine, pts, calib12, *stacks)
    return [rows[s] for s in range(len(stacks))], in_cube


class TrainQuery:
    """The dispatcher ``attach`` installs as ``netG.query`` (the reference's signature)."""

    def __init__(self, netG, engine):
        self.netG, self.engine = netG, engine

    def __call__(self, features, points, calibs, transforms=None, regressor=None):
        eng = self.engine
        reg = eng._bound_regressor(regressor)
        if not (isinstance(reg, torch.nn.Module) and reg.training):
            return eng.query(features, points, calibs, transforms=transforms, regressor=regressor)
        mod = sys.modules.get(type(self.netG).__module__)
        if mod is not None and getattr(mod, "maskout", False):
            raise IconAmdError(f"{_WHAT}: {type(self.netG).__module__}.maskout is set; the training path evaluates the shipped maskout = False path only")
        rows_list, in_cube = point_features_device(eng, features, points, calibs, transforms)
        # the reference's own operators behind point_feat (:361-365), one entry per stack in order
        return [in_cube * reg(rows) for rows in rows_list]


def attach(netG, **kw):
    """Replace ``netG.query`` by a dispatcher: while the regressor in use is in training mode, ``[in_cube * regressor(rows_s) for s in
    stacks]`` over the native rows (so ``netG.forward`` and ``get_error`` run unchanged); in eval mode ``IconQueryEngine.query``,
    untouched.  Works whether ``netG`` is in train or eval mode now: the engine checks the regressor when an eval-mode call first
    needs its folded weights.  ``kw``: ``IconQueryEngine``'s.  Returns the dispatcher (``.engine``: the engine)."""
    from .engine import IconQueryEngine
    eng = IconQueryEngine.attach(netG, **kw)          # refuses maskout; binds netG; checks no regressor yet
    q = TrainQuery(netG, eng)
    netG.query = q
    return q

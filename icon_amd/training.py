"""The training step's ``query()``: ``HGPIFuNet.query`` with the network in TRAIN mode (``lib/net/HGPIFuNet.py:268-367``, reached from
``ICON.training_step``, ``apps/ICON.py:178-236``, through ``netG.forward``) for the ``icon``, ``pifu`` and ``pamir`` priors.

What is native is everything in front of the regressor (csrc/train_rows.hip): ``point_feat`` of EVERY feature stack
from one search (``icon_train_rows_forward``) and the gradient of those rows into the feature planes, without floating-point
atomics (``icon_train_rows_backward``).  The regressor stays the module's own PyTorch layers: train-mode BatchNorm reduces over all
B * N points between every pair of layers, updates its running statistics, and its parameters are the optimizer's leaves.

The pamir prior: the rows are ``[img | vol]`` - the bilinear tap of the planes and the trilinear tap of the volume
that ``netG.ve`` (train mode, its parameters the optimizer's) gave for the same stack (``icon_train_pamir_forward``) - and the volume
encoder is reached by the gradient of those rows into the volumes (``icon_train_vol_backward``): a gather in a fixed order, where
torch's own 5-D ``grid_sample`` scatters with floating-point atomics.

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


def _native_pamir_forward(stacks, vols, pts, calib12):
    """(rows [S,B,C+Cv,N], in_cube [B,1,N], taps [B*N,4] int32): two launches, no workspace"""
    S = len(stacks)
    B, Cc = int(stacks[0].shape[0]), int(stacks[0].shape[1])
    Cv, N, dev = int(vols[0].shape[1]), int(pts.shape[1]), pts.device
    rows = torch.empty((S, B, Cc + Cv, N), dtype=torch.float32, device=dev)
    in_cube = torch.empty((B, 1, N), dtype=torch.float32, device=dev)
    taps = torch.empty((B * N, 4), dtype=torch.int32, device=dev)
    ptrs = (C.c_void_p * S)(*[t.data_ptr() for t in stacks])
    shapes = (C.c_int32 * (4 * S))(*[int(x) for t in stacks for x in t.shape])
    vptrs = (C.c_void_p * S)(*[t.data_ptr() for t in vols])
    vshapes = (C.c_int32 * (5 * S))(*[int(x) for t in vols for x in t.shape])
    check(_lib.lib().icon_train_pamir_forward(ptrs, shapes, vptrs, vshapes, C.c_int(S), _lib.ptr(calib12), _lib.ptr(pts), C.c_int64(N),
                                              _lib.ptr(rows), _lib.ptr(in_cube), _lib.ptr(taps), stream()), "icon_train_pamir_forward")
    return rows, in_cube, taps


def _native_vol_backward(grad_rows, taps, shape, n_planes: int, mask: int, out=None):
    """grad_vols [S,B,Cv,D,H,W]: the stacks whose bit of ``mask`` is set are written, element by element (``out``: into this tensor);
    ``n_planes``: the image channels in front of the volume channels of the rows"""
    S, B, Cv, D, H, W = shape
    cin, N = int(grad_rows.shape[2]), int(grad_rows.shape[3])
    dev = grad_rows.device
    scratch = scratch_for(dev, "icon_train_vol_bytes", C.c_int(B), C.c_int64(N), C.c_int(S), C.c_int(Cv), C.c_int(D), C.c_int(H), C.c_int(W))
    grad_vols = torch.empty(shape, dtype=torch.float32, device=dev) if out is None else out
    check(_lib.lib().icon_train_vol_backward(_lib.ptr(grad_rows), _lib.ptr(taps), C.c_int(S), C.c_uint32(mask), C.c_int(B), C.c_int(cin),
                                             C.c_int(n_planes), C.c_int(Cv), C.c_int(D), C.c_int(H), C.c_int(W), C.c_int64(N),
                                             _lib.ptr(grad_vols), _lib.ptr(scratch), C.c_int64(scratch.numel()), stream()),
          "icon_train_vol_backward")
    return grad_vols


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


class _TrainPamirFn(torch.autograd.Function):
    """(pts [B,N,3], calib12 [B,12], S, *stacks [B,C,H,W], *vols [B,Cv,D,H,W]) -> rows [S,B,C+Cv,N], in_cube [B,1,N]"""

    @staticmethod
    def forward(ctx, pts, calib12, S, *tensors):
        stacks, vols = tensors[:S], tensors[S:]
        with torch.cuda.device(pts.device):
            rows, in_cube, taps = _native_pamir_forward(stacks, vols, pts, calib12)
        ctx.save_for_backward(taps)
        ctx.S = S
        ctx.plane_shape = (S,) + tuple(int(x) for x in stacks[0].shape)
        ctx.vol_shape = (S,) + tuple(int(x) for x in vols[0].shape)
        ctx.mark_non_differentiable(in_cube)
        return rows, in_cube

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rows, _g_in_cube):
        S = ctx.S
        needs_p, needs_v = ctx.needs_input_grad[3:3 + S], ctx.needs_input_grad[3 + S:]
        mask_p = sum(1 << s for s in range(S) if needs_p[s])
        mask_v = sum(1 << s for s in range(S) if needs_v[s])
        if (mask_p == 0 and mask_v == 0) or g_rows is None:
            return (None,) * (3 + 2 * S)
        (taps,) = ctx.saved_tensors
        gp = gv = None
        with torch.cuda.device(g_rows.device):
            g = g_rows.to(torch.float32).contiguous()
            if mask_p:                                               # the planes' own backward: the rows hold C + Cv channels, one half
                gp = _native_backward(g, taps, ctx.plane_shape, 1, mask_p)
            if mask_v:
                gv = _native_vol_backward(g, taps, ctx.vol_shape, ctx.plane_shape[2], mask_v)
        return (None, None, None) + tuple(gp[s] if needs_p[s] else None for s in range(S)) + tuple(gv[s] if needs_v[s] else None for s in range(S))


def _check_call(eng, features, points, calibs, transforms=None, vol_feats=None) -> None:
    if eng.prior_type == "pamir" and vol_feats is None:
        raise IconAmdError(f"{_WHAT}: prior_type 'pamir' is not trained here without vol_feats (the volume encoder's output per feature "
                           "stack, [B,Cv,D,H,W] each)")
    if eng.prior_type != "pamir" and vol_feats is not None:
        raise IconAmdError(f"{_WHAT}: vol_feats belong to prior_type 'pamir', not to {eng.prior_type!r}")
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
    if vol_feats is not None:
        if not isinstance(vol_feats, (list, tuple)) or len(vol_feats) != len(features):
            n_vol = len(vol_feats) if isinstance(vol_feats, (list, tuple)) else type(vol_feats).__name__
            raise IconAmdError(f"{_WHAT}: vol_feats holds {n_vol} volumes for {len(features)} feature stacks: one [B,Cv,D,H,W] volume per "
                               "stack (the reference's zip would drop the surplus silently)")
        for s, v in enumerate(vol_feats):
            if not torch.is_tensor(v):
                raise IconAmdError(f"{_WHAT}: vol_feats[{s}] must be a tensor, got {type(v).__name__}")
            if not v.is_cuda:
                raise IconAmdError(f"{_WHAT}: vol_feats[{s}] is a CPU tensor; icon_amd has no CPU path - move it to the HIP device")
            if v.dim() != 5 or int(v.shape[0]) != B:
                raise IconAmdError(f"{_WHAT}: vol_feats[{s}] {tuple(v.shape)} must be [{B},Cv,D,H,W]: the points' batch size")
            if tuple(v.shape) != tuple(vol_feats[0].shape):
                raise IconAmdError(f"{_WHAT}: vol_feats differ in shape ({tuple(vol_feats[0].shape)} and {tuple(v.shape)}): one call covers "
                                   "volumes of one shape")


def point_features_device(engine, features: Sequence[torch.Tensor], points: torch.Tensor, calibs: torch.Tensor, transforms=None,
                          vol_feats: Sequence[torch.Tensor] = None):
    """``point_feat`` of ``HGPIFuNet.query`` (:329-359) for every stack of ``features`` (list of [B,C,H,W], one shape) at ``points``
    [B,3,N] under ``calibs`` [B,4,4] -> ``(rows_list, in_cube)``: S views [B,Cin,N] of one tensor, channels ``[img | sdf | cmap |
    norm]`` (icon, per ``engine.smpl_feats``) or ``[img | z]`` (pifu), and ``in_cube`` [B,1,N] (:274-275).  Differentiable in the
    feature stacks only; a stack that does not need a gradient costs the backward nothing, and when none does no backward call is
    made.  One native call each way on the current stream, nothing read back; equal bytes from run to run.

    ``prior_type == 'pamir'``: ``vol_feats`` is the list of ``netG.ve``'s volumes, one [B,Cv,D,H,W] device tensor per feature stack
    and all of one shape (another count is refused: the reference's ``zip`` would drop stacks); the rows are [B,C+Cv,N], ``[img |
    vol]`` (:348-359), differentiable in the stacks and in the volumes.  The backward calls the planes' gather only when a stack
    needs a gradient and the volumes' gather (``icon_train_vol_backward``, no floating-point atomics) only when a volume does."""
    _check_call(engine, features, points, calibs, transforms, vol_feats)
    with torch.cuda.device(points.device):
        calib12 = calibs[:, :3, :4].detach().to(points.device, torch.float32).reshape(calibs.shape[0], 12).contiguous()
        pts = points.detach().transpose(1, 2).to(torch.float32).contiguous()
        stacks = [f.to(torch.float32).contiguous() for f in features]
        if vol_feats is not None:
            vols = [v.to(torch.float32).contiguous() for v in vol_feats]
            rows, in_cube = _TrainPamirFn.apply(pts, calib12, len(stacks), *stacks, *vols)
        else:
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
        # train-mode BatchNorm writes its running statistics in place WITHOUT raising their version counter, which is what the engine's
        # cache of the folded eval-mode regressor is keyed on: an eval call after this one folds anew
        eng._mlp_key = None
        if eng.prior_type == "pamir":
            rows_list, in_cube = point_features_device(eng, features, points, calibs, transforms, vol_feats=self._pamir_vol_feats(points))
        else:
            rows_list, in_cube = point_features_device(eng, features, points, calibs, transforms)
        # the reference's own operators behind point_feat (:361-365), one entry per stack in order
        return [in_cube * reg(rows) for rows in rows_list]


    def _pamir_vol_feats(self, points):
        """``self.ve(vol, intermediate_output=True)`` of lib/net/HGPIFuNet.py:314-325 in training mode: the semantic volume from the
        code the eval path uses (``engine._semantic_volume``: padding stripped with subject 0's counts, subject 0's tetrahedra, the
        engine's ``voxelizer=``) without a gradient - the reference's VoxelizationFunction defines none -, then the volume encoder
        with autograd, once per call and never cached: its parameters change every step.  The engine's eval-mode volume caches
        are keyed on the voxel tensors alone, so a training call drops them: the next eval call encodes with the current weights.
        Reading ``pad_v_num[0]`` / ``pad_f_num[0]`` from device tensors waits for the device, as the eval path's read does: "nothing
        waited for" holds for the native calls only."""
        netG, eng = self.netG, self.engine
        if not hasattr(netG, "ve") or not hasattr(netG, "voxelization"):
            raise IconAmdError(f"{_WHAT}: prior_type 'pamir' is not trained here: netG has no `ve` / `voxelization`")
        eng._vol_key = eng._volb_key = None
        with torch.no_grad():
            vol = eng._semantic_volume(int(points.shape[0]))
        return netG.ve(vol, intermediate_output=True)


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

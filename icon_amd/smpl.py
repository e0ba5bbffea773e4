"""SMPL linear blend skinning on the device: what ``dataset.smpl_model(betas=..., body_pose=..., global_orient=...,
pose2rot=False)`` computes per step of the body-fit loop (``apps/infer.py:163-273``, ``optim_body`` in ``apps/ICON.py``),
without the vendored ``lib/smplx``.

Replaces ``lbs()`` (``lib/smplx/lbs.py:152-252``) by a ``torch.autograd.Function`` over two native calls, ``icon_smpl_forward``
and ``icon_smpl_backward`` (csrc/smpl.hip; the rule is DESIGN.md 4.17, pinned to the reference's own ``lbs`` through
tests/smpl_oracle.py), and ``SMPL.forward`` (``lib/smplx/body_models.py:314-398``) by ``attach(module)``.  What the native calls
read of a model is built ONCE per model by ``SmplModel``, from torch operators on whatever device the buffers live on; the
native calls need a HIP device and there is no CPU path for them.

Not built: the SMPL-H / SMPL-X forwards (hand poses, jaw and eye poses, expression blend shapes, landmarks), MANO, FLAME and
pixie's own body model - ``attach`` takes modules whose forward is ``SMPL.forward``'s (shape, body pose, global orientation,
translation) and nothing else.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import IconAmdError, check
from ._native import need_device, scratch_for, stream

MAX_JOINTS, MAX_BETAS = 64, 512                                            # include/icon_amd.h: the limits of icon_smpl_*
BUFFERS = ("v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights")
FIELDS = ("vertices", "joints", "full_pose", "global_orient", "transl", "betas", "body_pose")


class _Tables(C.Structure):                                               # include/icon_amd.h: icon_smpl_tables
    _fields_ = [(n, C.c_void_p) for n in ("v_template", "shapedirs", "posedirs", "J_template", "J_shapedirs", "parents", "skin_idx",
                                          "skin_w")] + [("V", C.c_int64), ("J", C.c_int32), ("NB", C.c_int32), ("K", C.c_int32), ("P", C.c_int32)]


class SmplModel:
    """The tables the native skinning reads of one body model, built once (plumbing: torch operators, one synchronisation).

    ``SmplModel(v_template [V,3], shapedirs [V,3,NB], posedirs [9(J-1),3V], J_regressor [J,V], parents [J], lbs_weights [V,J])``:
    the buffers of an ``smplx``-style module, on any device (``from_module`` reads them off one).  Raises ``IconAmdError`` unless
    every shape agrees, every value is finite, ``parents[0] == -1`` and ``0 <= parents[j] < j`` for ``j >= 1`` (the chain is
    walked in index order), ``J <= 64`` and ``NB <= 512`` - so that no kernel can index outside a table.

    * ``v_template [3,V]``, ``shapedirs [NB,3,V]``, ``posedirs [9(J-1),3,V]``: float32, component-major (vertex last).
    * ``J_template [J,3] = J_regressor v_template``, ``J_shapedirs [J,3,NB] = J_regressor shapedirs``: formed in float64, rounded
      once - the joints are linear in betas.
    * ``skin_idx [V,K]`` int32, ``skin_w [V,K]`` float32: the non-zero weights of each vertex, joints ascending, rows padded with
      ``(0, 0.0)``; ``K`` the largest count of any row (4 for SMPL; ``J`` for dense weights), at least 1.
    * ``parents [J]`` int32.

    ``to(device)`` gives a copy."""

    _FIELDS = ("v_template", "shapedirs", "posedirs", "J_template", "J_shapedirs", "parents", "skin_idx", "skin_w")

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights):
        named = dict(zip(BUFFERS, (v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights)))
        for name, t in named.items():
            if not torch.is_tensor(t):
                raise IconAmdError(f"SmplModel: {name} must be a tensor, got {type(t).__name__}")
            if (name == "parents") == (t.dtype.is_floating_point or t.dtype == torch.bool):
                raise IconAmdError(f"SmplModel: {name} must be {'an integer' if name == 'parents' else 'a floating-point'} tensor, got {t.dtype}")
        dev = v_template.device
        if any(t.device != dev for t in named.values()):
            raise IconAmdError("SmplModel: the six buffers must live on one device")
        if v_template.dim() != 2 or v_template.shape[1] != 3 or v_template.shape[0] < 1 or J_regressor.dim() != 2 or J_regressor.shape[0] < 1:
            raise IconAmdError(f"SmplModel: v_template must be [V,3] and J_regressor [J,V], got {tuple(v_template.shape)} and {tuple(J_regressor.shape)}")
        V, J = int(v_template.shape[0]), int(J_regressor.shape[0])
        if shapedirs.dim() != 3:
            raise IconAmdError(f"SmplModel: shapedirs must be [V,3,NB], got {tuple(shapedirs.shape)}")
        NB, P = int(shapedirs.shape[2]), 9 * (J - 1)
        want = dict(shapedirs=(V, 3, NB), posedirs=(P, 3 * V), J_regressor=(J, V), parents=(J,), lbs_weights=(V, J))
        for name, shape in want.items():
            if tuple(named[name].shape) != shape:
                raise IconAmdError(f"SmplModel: {name} must be {list(shape)} for V = {V}, J = {J}, NB = {NB}, got {list(named[name].shape)}")
        if J > MAX_JOINTS or NB > MAX_BETAS:
            raise IconAmdError(f"SmplModel: J = {J}, NB = {NB}: the kernels are built for J <= {MAX_JOINTS} and NB <= {MAX_BETAS}")
        vt, sd, pd, Jr, w = (named[n].detach() for n in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights"))
        par = parents.detach().to(torch.int64)
        nz = w != 0
        order_ok = (par[0] == -1) & ((par[1:] >= 0) & (par[1:] < torch.arange(1, J, device=dev))).all()
        finite = torch.stack([torch.isfinite(t).all() for t in (vt, sd, pd, Jr, w)]).all()
        count = nz.sum(1).max()
        ok_order, ok_finite, K = (int(x) for x in torch.stack([order_ok.long(), finite.long(), count.long()]).tolist())   # the one synchronisation
        if not ok_order:
            raise IconAmdError("SmplModel: parents must hold -1 for the root and 0 <= parents[j] < j for every other joint")
        if not ok_finite:
            raise IconAmdError("SmplModel: a buffer holds a value that is not finite")
        self.V, self.J, self.NB, self.P, self.K = V, J, NB, P, max(K, 1)
        f32 = torch.float32
        self.v_template = vt.to(f32).t().contiguous()
        self.shapedirs = sd.to(f32).permute(2, 1, 0).contiguous()
        self.posedirs = pd.to(f32).reshape(P, V, 3).permute(0, 2, 1).contiguous()
        Jr64 = Jr.to(torch.float64)
        self.J_template = (Jr64 @ vt.to(torch.float64)).to(f32).contiguous()
        self.J_shapedirs = torch.einsum("jv,vcl->jcl", Jr64, sd.to(torch.float64)).to(f32).contiguous()
        self.parents = par.to(torch.int32).contiguous()
        # the non-zero columns of each row first, in ascending order (a stable sort of "is zero"), cut at K
        cols = torch.argsort((~nz).to(torch.int8), dim=1, stable=True)[:, :self.K]
        keep = torch.gather(nz, 1, cols)
        self.skin_idx = torch.where(keep, cols, torch.zeros_like(cols)).to(torch.int32).contiguous()
        self.skin_w = torch.where(keep, torch.gather(w.to(f32), 1, cols), torch.zeros((), dtype=f32, device=dev)).contiguous()
        self._struct = None

    @classmethod
    def from_module(cls, module) -> "SmplModel":
        """from the six buffers of an ``smplx``-style module (``SMPL``, ``SMPLLayer``)"""
        missing = [n for n in BUFFERS if not torch.is_tensor(getattr(module, n, None))]
        if missing:
            raise IconAmdError(f"SmplModel.from_module: {type(module).__name__} has no tensor {missing}")
        return cls(*(getattr(module, n) for n in BUFFERS))

    @property
    def device(self) -> torch.device:
        return self.v_template.device

    def to(self, device) -> "SmplModel":
        out = object.__new__(SmplModel)
        out.V, out.J, out.NB, out.P, out.K = self.V, self.J, self.NB, self.P, self.K
        for name in self._FIELDS:
            t = getattr(self, name).to(device)
            setattr(out, name, t.clone() if t is getattr(self, name) else t)
        out._struct = None
        return out

    def lbs_weights(self) -> torch.Tensor:
        """the dense ``[V,J]`` weights the sparse rows were cut from"""
        w = torch.zeros(self.V, self.J, dtype=torch.float32, device=self.device)
        return w.scatter_add_(1, self.skin_idx.long(), self.skin_w)

    def _tables(self) -> _Tables:
        if self._struct is None:
            self._struct = _Tables(*(getattr(self, n).data_ptr() for n in self._FIELDS), self.V, self.J, self.NB, self.K, self.P)
        return self._struct


class _SmplLbsFn(torch.autograd.Function):
    """(betas [B,NB], rot_mats [B,J,3,3]) float32, contiguous, on the model's device -> verts [B,V,3], joints [B,J,3]"""

    @staticmethod
    def forward(ctx, betas, rot, model):
        ctx.set_materialize_grads(False)                                   # an output nobody uses: a null pointer, not a tensor of zeros
        B = rot.shape[0]
        with torch.cuda.device(rot.device):
            verts = torch.empty((B, model.V, 3), dtype=torch.float32, device=rot.device)
            joints = torch.empty((B, model.J, 3), dtype=torch.float32, device=rot.device)
            A = torch.empty((B, model.J, 3, 4), dtype=torch.float32, device=rot.device)   # this call's own: a second forward must not overwrite it
            check(_lib.lib().icon_smpl_forward(C.byref(model._tables()), _lib.ptr(betas), _lib.ptr(rot), C.c_int64(B), _lib.ptr(verts),
                                               _lib.ptr(joints), _lib.ptr(A), stream()), "icon_smpl_forward")
        ctx.save_for_backward(betas, rot, A)
        ctx.model = model
        return verts, joints

    @staticmethod
    def backward(ctx, g_verts, g_joints):
        betas, rot, A = ctx.saved_tensors
        model = ctx.model
        if g_verts is None and g_joints is None:
            return None, None, None
        B = rot.shape[0]
        g_verts, g_joints = (None if g is None else g.to(torch.float32).contiguous() for g in (g_verts, g_joints))
        L = _lib.lib()
        with torch.cuda.device(rot.device):
            scratch = scratch_for(rot.device, "icon_smpl_bytes", C.c_int64(B), C.c_int64(model.V), C.c_int(model.J), C.c_int(model.NB),
                                  C.c_int(model.K))                            # this thread's and this stream's: autograd has its own
            g_betas, g_rot = torch.empty_like(betas), torch.empty_like(rot)
            check(L.icon_smpl_backward(C.byref(model._tables()), _lib.ptr(betas), _lib.ptr(rot), C.c_int64(B), _lib.ptr(A), _lib.ptr(g_verts),
                                       _lib.ptr(g_joints), _lib.ptr(g_betas), _lib.ptr(g_rot), _lib.ptr(scratch), C.c_int64(scratch.numel()),
                                       stream()), "icon_smpl_backward")
        return g_betas, g_rot, None


def smpl_lbs_device(betas: torch.Tensor, rot_mats: torch.Tensor, model: SmplModel):
    """``betas [B,NB]``, ``rot_mats [B,J,3,3]`` (float32) and ``model`` on one HIP device -> ``(verts [B,V,3], joints [B,J,3])``:
    ``lbs(betas, rot_mats, ..., pose2rot=False)`` of lib/smplx/lbs.py, differentiable in both inputs.  The matrices need not be
    orthonormal.  Each direction is one native call of two launches on the current stream: nothing read back, no
    floating-point atomics - equal bytes from run to run.  Non-contiguous inputs are made contiguous; an
    output nobody uses costs its gradient nothing."""
    what = "smpl_lbs_device"
    if not isinstance(model, SmplModel):
        raise IconAmdError(f"{what}: model must be a SmplModel")
    for name, t in (("betas", betas), ("rot_mats", rot_mats)):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise IconAmdError(f"{what}: {name} must be a float32 tensor, got {t.dtype if torch.is_tensor(t) else type(t).__name__}")
    if rot_mats.dim() != 4 or tuple(rot_mats.shape[1:]) != (model.J, 3, 3) or rot_mats.shape[0] < 1:
        raise IconAmdError(f"{what}: rot_mats must be [B,{model.J},3,3] (J = {model.J} joints), got {tuple(rot_mats.shape)}")
    B = rot_mats.shape[0]
    if tuple(betas.shape) != (B, model.NB):
        raise IconAmdError(f"{what}: betas must be [{B},{model.NB}] (NB = {model.NB} shape coefficients), got {tuple(betas.shape)}")
    need_device(what)
    if not (betas.is_cuda and rot_mats.is_cuda and betas.device == rot_mats.device) or model.device != rot_mats.device:
        raise IconAmdError(f"{what}: betas, rot_mats and the model must live on one HIP device (SmplModel.to(device) moves it)")
    return _SmplLbsFn.apply(betas.contiguous(), rot_mats.contiguous(), model)


def batch_rodrigues(rot_vecs: torch.Tensor) -> torch.Tensor:
    """axis-angle ``[N,3]`` -> matrices ``[N,3,3]`` as lib/smplx/lbs.py:299-333 states it:  angle = |r + 1e-8|,  k = r / angle,
    R = I + sin(angle) [k]x + (1 - cos(angle)) [k]x^2"""
    angle = torch.norm(rot_vecs + 1e-8, dim=1, keepdim=True)
    k = rot_vecs / angle
    zeros = torch.zeros_like(angle)
    kx, ky, kz = k[:, 0:1], k[:, 1:2], k[:, 2:3]
    Kx = torch.cat([zeros, -kz, ky, kz, zeros, -kx, -ky, kx, zeros], dim=1).view(-1, 3, 3)
    eye = torch.eye(3, dtype=rot_vecs.dtype, device=rot_vecs.device).unsqueeze(0)
    return eye + torch.sin(angle).unsqueeze(1) * Kx + (1 - torch.cos(angle).unsqueeze(1)) * torch.bmm(Kx, Kx)


class SmplOutput:
    """the fields of the reference's ``SMPLOutput``, readable as attributes and by ``[...]``"""

    def __init__(self, **fields):
        for name in FIELDS:
            setattr(self, name, fields.get(name))

    def __getitem__(self, key):
        return getattr(self, key)

    def get(self, key, default=None):
        return getattr(self, key, default)

    def keys(self):
        return iter(FIELDS)

    def __iter__(self):
        return self.keys()


def _forward(module, betas=None, body_pose=None, global_orient=None, transl=None, return_verts=True, return_full_pose=False,
             pose2rot=True, **kwargs):
    """``SMPL.forward`` (lib/smplx/body_models.py:314-398) around the native skinning"""
    global_orient = global_orient if global_orient is not None else module.global_orient
    body_pose = body_pose if body_pose is not None else module.body_pose
    betas = betas if betas is not None else module.betas
    apply_trans = transl is not None or hasattr(module, "transl")
    if transl is None and hasattr(module, "transl"):
        transl = module.transl
    full_pose = torch.cat([global_orient, body_pose], dim=1)
    B = max(betas.shape[0], global_orient.shape[0], body_pose.shape[0])
    if betas.shape[0] != B:
        betas = betas.expand(int(B / betas.shape[0]), -1)
    model = module.icon_amd_smpl
    if model.device != full_pose.device:                                  # the module moved after attach: its tables follow, once
        model = module.icon_amd_smpl = model.to(full_pose.device)
    # axis-angles: the reference's formula in float64, rounded once like everything else of the rule (a handful of small operators)
    rot = batch_rodrigues(full_pose.reshape(-1, 3).double()).to(full_pose.dtype) if pose2rot else full_pose
    vertices, joints = smpl_lbs_device(betas, rot.reshape(B, -1, 3, 3), model)
    joints = module.vertex_joint_selector(vertices, joints)
    if getattr(module, "joint_mapper", None) is not None:
        joints = module.joint_mapper(joints)
    if apply_trans:
        joints = joints + transl.unsqueeze(dim=1)
        vertices = vertices + transl.unsqueeze(dim=1)
    return SmplOutput(vertices=vertices if return_verts else None, joints=joints, betas=betas, global_orient=global_orient,
                      body_pose=body_pose, full_pose=full_pose if return_full_pose else None)


def attach(module) -> SmplModel:
    """Replace the forward of an ``smplx``-style ``SMPL`` module by the HIP path; everything else on the module is untouched.
    Afterwards ``module(betas=..., body_pose=..., global_orient=..., transl=None, pose2rot=..., return_verts=...,
    return_full_pose=...)`` returns an object with the reference's fields (``vertices, joints, full_pose, global_orient, transl,
    betas, body_pose``; ``transl`` stays None there, as in the reference): defaults from the module's own parameters, ``betas``
    expanded to the batch, ``joints`` through the module's ``vertex_joint_selector`` and ``joint_mapper``, ``transl`` added to both
    outputs.  ``pose2rot=True`` converts axis-angle by ``batch_rodrigues`` (torch operators, in float64, rounded once; the native
    call always takes matrices), ``pose2rot=False`` takes ``[B,J-1,3,3]`` / ``[B,1,3,3]`` as apps/infer.py passes them.  The SMPL-H / SMPL-X hand,
    face and expression forwards and pixie's model are not built.  ``detach(module)`` undoes it."""
    if hasattr(module, "icon_amd_smpl"):
        raise IconAmdError("attach: this module is attached already")
    model = SmplModel.from_module(module)
    module.icon_amd_smpl = model
    module.forward = lambda *args, **kwargs: _forward(module, *args, **kwargs)
    return model


def detach(module) -> None:
    """give ``module`` its own forward back"""
    if not hasattr(module, "icon_amd_smpl"):
        raise IconAmdError("detach: this module is not attached")
    del module.forward
    del module.icon_amd_smpl

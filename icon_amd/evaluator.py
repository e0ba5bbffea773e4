"""The reference's ``Evaluator`` on the device: normal consistency, the evaluator's own normal maps, ``calc_acc``.

Replaces ``lib.dataset.Evaluator.Evaluator`` (an OpenGL renderer - lib/renderer/gl/normal_render.py, data/normal.vs/.fs - plus
trimesh and rtree) for ``ICON.test_step`` (apps/ICON.py:519-645), i.e. ``python -m apps.train -test``: the third metric of the
paper's table (``calculate_normal_consist``, :639) and the ``T_normal_F`` / ``T_normal_B`` inputs of ``netG.filter`` in the test
step (``render_normal``, :556).  Every image comes from ONE native call, ``icon_normal_consistency`` (csrc/evaluator.hip); the
rule is DESIGN.md 4.20, stated in csrc/raster_gl_device.h.  It is NOT the pytorch3d rule of ``icon_amd.render`` (4.13): coverage
at the pixel centres with a shared-edge tie rule, near / far clipping, background (1, 1, 1, 0), trimesh's angle-weighted vertex
normals, the normal normalised per fragment.  PARITY UNPINNED like 4.13: neither OpenGL nor trimesh is installed where this was
written; the rasteriser follows the OpenGL specification, the vertex normals are trimesh's restated from memory
(tools/parity_real_packages.py compares both with the real packages where they exist).  There is no CPU path.

Differences that are documented rather than hidden: a face with a clip coordinate beyond 64 in x or y is not drawn (OpenGL
would clip it); a real depth buffer quantises z to 24 bits, this one compares float32; ``trimesh.Trimesh`` merges coincident
vertices when it is constructed, nothing here does; ``calculate_chamfer_p2s`` samples as ``icon_amd.metrics`` documents.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Sequence

import numpy as np
import torch

from . import _lib
from ._lib import IconAmdError, check
from ._native import constants, faces_arg, scratch_for, stream
from .render import _check_mesh, _check_size

MAX_VIEWS = 32


def euler_to_rot_mat(r_x: float, r_y: float, r_z: float) -> np.ndarray:
    """float64 ``[3,3]``: the rotation about x, then y, then z (``Rz Ry Rx``) - what ``NormalRender.euler_to_rot_mat`` returns"""
    cx, sx, cy, sy, cz, sz = math.cos(r_x), math.sin(r_x), math.cos(r_y), math.sin(r_y), math.cos(r_z), math.sin(r_z)
    rot_x = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    rot_y = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    rot_z = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    return rot_z @ (rot_y @ rot_x)


def view_matrices(degs, scale_factor: float = 1.0, offset: float = 0.0) -> np.ndarray:
    """azimuths in degrees -> float32 ``[K,3,4]``: the model matrix of ``Evaluator._render_normal`` for each, formed in float64 -
    ``euler_to_rot_mat(0, deg / 180 * pi, 0)``, ``offset`` in row 1 of the last column - with the ``scale_factor`` the reference
    multiplies the vertices by folded into the 3 x 3 part, and rounded ONCE.  The only place that turns angles into what
    ``icon_normal_consistency`` projects with; needs no device."""
    d = np.asarray(list(degs) if not isinstance(degs, np.ndarray) else degs, dtype=np.float64).reshape(-1)
    if not np.isfinite(d).all() or not math.isfinite(float(scale_factor)) or not math.isfinite(float(offset)):
        raise IconAmdError("evaluator: angles, scale_factor and offset must be finite")
    out = np.zeros((len(d), 3, 4), np.float64)
    for k, deg in enumerate(d):
        out[k, :, :3] = euler_to_rot_mat(0, deg / 180.0 * np.pi, 0) * float(scale_factor)
        out[k, 1, 3] = float(offset)
    return out.astype(np.float32)


def _check_views(degs, mats, muls, scale_factor, offset):
    """-> float32 contiguous ``mats [K,3,4]``, ``muls [K,3]`` on the host"""
    if mats is None:
        if degs is None:
            raise IconAmdError("evaluator: give the views as degs or as mats")
        mats = view_matrices(degs, scale_factor, offset)
    mats = np.ascontiguousarray(np.asarray(mats, dtype=np.float32))
    if mats.ndim != 3 or mats.shape[1:] != (3, 4):
        raise IconAmdError(f"evaluator: mats must be [K,3,4], got {mats.shape}")
    K = mats.shape[0]
    if not 1 <= K <= MAX_VIEWS:
        raise IconAmdError(f"evaluator: 1..{MAX_VIEWS} views per call, got {K}")
    muls = np.ones((K, 3), np.float32) if muls is None else np.asarray(muls, dtype=np.float32)
    if muls.ndim == 1 and muls.shape == (3,):
        muls = np.broadcast_to(muls, (K, 3))
    muls = np.array(muls, dtype=np.float32, order="C")                       # a copy: a broadcast view is read-only
    if muls.shape != (K, 3):
        raise IconAmdError(f"evaluator: muls must be [K,3] or [3], got {muls.shape}")
    return mats, muls


def _check_normals(verts, normals):
    if normals is None:
        return None
    if not torch.is_tensor(normals) or normals.shape != verts.shape or not normals.dtype.is_floating_point:
        raise IconAmdError(f"evaluator: normals must be a floating-point tensor of the vertices' shape {tuple(verts.shape)}")
    if not normals.is_cuda or normals.device != verts.device:
        raise IconAmdError("evaluator: normals must live on the vertices' device")
    return normals.detach().to(torch.float32).contiguous()


def normal_consistency_device(verts_a, faces_a, verts_b=None, faces_b=None, degs=(0, 180, 90, 270), size: int = 512, *,
                              normals_a=None, normals_b=None, scale_factor: float = 1.0, offset: float = 0.0, mats=None, muls=None,
                              return_images: bool = False, return_faces: bool = False, return_normals: bool = False):
    """``verts_* [V,3]`` (float), ``faces_* [F,3]`` (int32 or int64, read in place), all on one HIP device; the views as azimuths
    ``degs`` (``view_matrices``) or as ``mats [K,3,4]``, ``K <= 32``; ``muls [K,3]`` or ``[3]`` multiplies the camera normals
    (default 1); ``normals_*``: vertex normals ``[V,3]``, or None for the angle-weighted ones of DESIGN.md 4.20.

    -> ``err [K]`` float64 on the device: per view the mean over the ``size^2`` pixels of the squared RGB difference of the two
    meshes' normal maps (``Evaluator._get_reproj_normal_error``); then ``rgba_a, rgba_b [K,size,size,4]`` float32 with
    ``return_images``, ``pix_a, pix_b [K,size,size]`` int32 (winning face, -1: background) with ``return_faces`` and the vertex
    normals used, ``[V,3]`` float32 each, with ``return_normals``.  Without mesh b (both None) nothing is compared: the result is
    ``rgba_a`` (then ``pix_a`` with ``return_faces``, the normals with ``return_normals``).

    ONE native call enqueued on the current stream, launches only: nothing is allocated by it, nothing read back, the stream is
    not waited for - so a face that names a vertex that does not exist cannot raise here; it is skipped.  Equal bytes from run
    to run.  Not differentiable.  Bad input raises ``IconAmdError`` before anything is launched."""
    size = _check_size(size)
    single = verts_b is None and faces_b is None
    if not single and (verts_b is None or faces_b is None):
        raise IconAmdError("evaluator: mesh b needs both verts and faces")
    if single and normals_b is not None:
        raise IconAmdError("evaluator: normals_b without mesh b")
    mats, muls = _check_views(degs, mats, muls, scale_factor, offset)
    fa = _check_mesh("normal_consistency_device", verts_a, faces_a, need_float=True)
    fb = None if single else _check_mesh("normal_consistency_device", verts_b, faces_b, need_float=True)
    if not single and verts_b.device != verts_a.device:
        raise IconAmdError("normal_consistency_device: both meshes must live on one HIP device")
    na, nb = _check_normals(verts_a, normals_a), (None if single else _check_normals(verts_b, normals_b))
    va = verts_a.detach().to(torch.float32).contiguous()
    vb = None if single else verts_b.detach().to(torch.float32).contiguous()
    dev, K = va.device, mats.shape[0]
    L = _lib.lib()
    with torch.cuda.device(dev):
        d_mats, d_muls = constants(dev, mats, muls)
        Vb, Fb = (0, 0) if single else (vb.shape[0], fb.shape[0])
        scratch = scratch_for(dev, "icon_normal_consistency_bytes", C.c_int64(va.shape[0]), C.c_int64(fa.shape[0]), C.c_int64(Vb), C.c_int64(Fb),
                              C.c_int(size), C.c_int(K))
        images = return_images or single
        err = None if single else torch.empty(K, dtype=torch.float64, device=dev)
        rgba_a = torch.empty((K, size, size, 4), dtype=torch.float32, device=dev) if images else None
        rgba_b = torch.empty((K, size, size, 4), dtype=torch.float32, device=dev) if images and not single else None
        pix_a = torch.empty((K, size, size), dtype=torch.int32, device=dev) if return_faces else None
        pix_b = torch.empty((K, size, size), dtype=torch.int32, device=dev) if return_faces and not single else None
        out_a = torch.empty_like(va) if return_normals and na is None else None
        out_b = torch.empty_like(vb) if return_normals and not single and nb is None else None
        i64 = lambda f: C.c_int(0) if f is None else faces_arg(f)[1]
        check(L.icon_normal_consistency(_lib.ptr(va), C.c_int64(va.shape[0]), _lib.ptr(fa), C.c_int64(fa.shape[0]), i64(fa), _lib.ptr(na),
                                        _lib.ptr(vb), C.c_int64(Vb), _lib.ptr(fb), C.c_int64(Fb), i64(fb), _lib.ptr(nb),
                                        _lib.ptr(d_mats), _lib.ptr(d_muls), C.c_int(K), C.c_int(size), _lib.ptr(err),
                                        _lib.ptr(rgba_a), _lib.ptr(rgba_b), _lib.ptr(pix_a), _lib.ptr(pix_b), _lib.ptr(out_a), _lib.ptr(out_b),
                                        _lib.ptr(scratch), C.c_int64(scratch.numel()), stream()), "icon_normal_consistency")
    nrm_a, nrm_b = (na if na is not None else out_a), (nb if nb is not None else out_b)
    if single:
        out = (rgba_a,) + ((pix_a,) if return_faces else ()) + ((nrm_a,) if return_normals else ())
        return out if len(out) > 1 else rgba_a
    out = (err,) + ((rgba_a, rgba_b) if return_images else ()) + ((pix_a, pix_b) if return_faces else ()) + ((nrm_a, nrm_b) if return_normals else ())
    return out if len(out) > 1 else err


class EvalMesh:
    """what the reference keeps as ``trimesh.Trimesh``: ``vertices [V,3]`` and ``faces [F,3]`` (tensors), nothing merged"""

    def __init__(self, vertices, faces):
        self.vertices, self.faces = vertices, faces


class Evaluator:
    """Drop-in for ``lib.dataset.Evaluator.Evaluator`` with the data on the device::

        ev = Evaluator(torch.device("cuda:0"))
        ev.set_mesh({"verts_pr": ..., "faces_pr": ..., "verts_gt": ..., "faces_gt": ..., "recon_size": 256, "calib": ...})
        ev.space_transfer()
        chamfer, p2s = ev.calculate_chamfer_p2s()
        nc = ev.calculate_normal_consist()

    The method and attribute names are the reference's.  ``init_gl`` does nothing: there is no OpenGL context to create."""

    _normal_render = "icon_normal_consistency"       # not None: the callers' `if evaluator._normal_render is None: init_gl()` passes

    @staticmethod
    def init_gl():
        return None

    def __init__(self, device, size: int = 512):
        from .render import Render
        self.device = torch.device(device)
        self.size = _check_size(size)
        self.render = Render(size=512, device=self.device) if self.device.type == "cuda" else None     # (it refuses a host device)
        self.error_term = torch.nn.MSELoss()
        self.offset = 0.0
        self.scale_factor = None

    def _tensor(self, x):
        return x.detach().to(self.device) if torch.is_tensor(x) else torch.as_tensor(np.asarray(x)).to(self.device)

    def set_mesh(self, result_dict, scale_factor=1.0, offset=0.0):
        """every entry becomes an attribute; tensors are detached and stay on (or move to) the evaluator's device, arrays become
        tensors there.  The caller's dictionary is left as it is."""
        for k, v in result_dict.items():
            setattr(self, k, self._tensor(v) if torch.is_tensor(v) or isinstance(v, np.ndarray) else v)
        self.scale_factor = scale_factor
        self.offset = offset

    def space_transfer(self):
        """``verts_pr`` from voxel units to the [-1,1] cube, ``verts_gt`` through ``calib`` with y turned over; then ``src_mesh``
        (the prediction) and ``tgt_mesh`` (the ground truth)"""
        half = self.recon_size / 2.0
        self.verts_pr = (self.verts_pr - half) / half
        calib = self.calib.to(self.verts_gt.dtype)
        gt = torch.mm(calib[:3, :3], self.verts_gt.T).T + calib[:3, 3]
        self.verts_gt = gt * torch.tensor([1.0, -1.0, 1.0], dtype=gt.dtype, device=gt.device)
        self.tgt_mesh = EvalMesh(self.verts_gt, self.faces_gt)
        self.src_mesh = EvalMesh(self.verts_pr, self.faces_pr)

    # ---- the normal maps -------------------------------------------------------------------------------------------------
    def _mesh_tensors(self, mesh):
        return self._tensor(mesh.vertices), self._tensor(mesh.faces)

    def _render_views(self, mesh, degs, norms=None, muls=None):
        """-> ``[K,S,S,4]`` float32 on the device: the mesh from every azimuth of ``degs``, one native call"""
        v, f = self._mesh_tensors(mesh)
        return normal_consistency_device(v, f, degs=degs, size=self.size, normals_a=None if norms is None else self._tensor(norms),
                                         scale_factor=self.scale_factor, offset=self.offset, muls=muls)

    def _render_normal(self, mesh, deg, norms=None):
        """-> ``[S,S,4]`` float32 on the device (the reference returns the same array on the host)"""
        return self._render_views(mesh, [deg], norms)[0]

    def render_mesh_list(self, mesh_lst):
        """-> host array ``[len(mesh_lst) S, 4 S, 4]``: a row per mesh, its maps from 0, 90, 180 and 270 degrees side by side"""
        self.offset = 0.0
        self.scale_factor = 1.0
        rows = [torch.cat(list(self._render_views(mesh, np.arange(0, 360, 90))), dim=1) for mesh in mesh_lst]
        return torch.cat(rows, dim=0).cpu().numpy()

    def _get_reproj_normal_errors(self, degs, return_images):
        src_v, src_f = self._mesh_tensors(self.src_mesh)
        tgt_v, tgt_f = self._mesh_tensors(self.tgt_mesh)
        return normal_consistency_device(src_v, src_f, tgt_v, tgt_f, degs=degs, size=self.size, scale_factor=self.scale_factor,
                                         offset=self.offset, return_images=return_images)

    def render_normal(self, verts, faces):
        """``verts [1,V,3]``, ``faces [1,F,3]`` -> ``{"T_normal_F", "T_normal_B"}``, each ``[1,3,S,S]`` in [-1,1] on the device: the
        mesh mirrored by (1,-1,1) from the front, and mirrored by (1,-1,-1) with its normals multiplied by (-1,-1,1) - the back
        seen through the front; both masked by the FRONT map's alpha"""
        v, f = self._tensor(verts)[0], self._tensor(faces)[0]
        self.scale_factor = 1.0
        sign = lambda *s: torch.tensor(s, dtype=v.dtype, device=v.device)
        normal_F = self._render_normal(EvalMesh(v * sign(1.0, -1.0, 1.0), f), 0)
        normal_B = self._render_views(EvalMesh(v * sign(1.0, -1.0, -1.0), f), [0], muls=[-1.0, -1.0, 1.0])[0]
        mask = normal_F[:, :, 3:4]
        to_planes = lambda img: (2.0 * (img - 0.5) * mask).permute(2, 0, 1)[:3].float().unsqueeze(0).to(self.device)
        return {"T_normal_F": to_planes(normal_F), "T_normal_B": to_planes(normal_B)}

    def calculate_normal_consist(self, frontal=True, back=True, left=True, right=True, save_demo_img=None, return_demo=False):
        """the sum over the chosen sides (0, 180, 90, 270 degrees, in that order) of the mean squared RGB difference between the
        prediction's and the ground truth's normal maps, as a Python float - one native call, then ONE read-back.  With
        ``return_demo`` the host array ``[2 S, sides S, 4]`` instead: per side the prediction's map above the ground truth's;
        ``save_demo_img`` writes it with PIL."""
        degs = [d for d, on in ((0, frontal), (180, back), (90, left), (270, right)) if on]
        if not degs:
            if return_demo or save_demo_img is not None:
                raise IconAmdError("calculate_normal_consist: no side chosen, nothing to show")
            return 0
        demo = return_demo or save_demo_img is not None
        out = self._get_reproj_normal_errors(degs, demo)
        err = out[0] if demo else out
        if demo:
            res_array = torch.cat([torch.cat([s, t], dim=0) for s, t in zip(out[1], out[2])], dim=1).cpu().numpy()
            if save_demo_img is not None:
                from PIL import Image
                Image.fromarray((res_array * 255).astype(np.uint8)).save(save_demo_img)
            if return_demo:
                return res_array
        total = 0.0
        for e in err.cpu().tolist():                                         # the reference adds the sides in this order
            total += e
        return total

    # ---- the other metrics -------------------------------------------------------------------------------------------------
    def calculate_chamfer_p2s(self, sampled_points=1000):
        """-> (chamfer, p2s), x100: ``icon_amd.metrics.chamfer_p2s`` on ``src_mesh`` / ``tgt_mesh`` with ``sampled_points`` samples
        per mesh - its docstring has the difference to the reference's sampling (area-weighted with a fixed seed, where the
        reference draws ``sample_surface_even`` points)"""
        from .metrics import chamfer_p2s
        return chamfer_p2s(self.src_mesh.vertices, self.src_mesh.faces, self.tgt_mesh.vertices, self.tgt_mesh.faces, n=int(sampled_points))

    def calc_acc(self, output, target, thres=0.5, use_sdf=False):
        """-> accuracy, IoU, precision, recall of ``output`` against ``target`` at ``thres`` (tensors, any device)"""
        with torch.no_grad():
            output = output.masked_fill(output < thres, 0.0).masked_fill(output > thres, 1.0)
            if use_sdf:
                target = target.masked_fill(target < thres, 0.0).masked_fill(target > thres, 1.0)
            acc = output.eq(target).float().mean()
            pred, gt = output > thres, target > thres
            one = torch.tensor(1.0).to(output.device)
            union, true_pos = max((pred | gt).sum().float(), one), max((pred & gt).sum().float(), one)
            vol_pred, vol_gt = max(pred.sum().float(), one), max(gt.sum().float(), one)
            return acc, true_pos / union, true_pos / vol_pred, true_pos / vol_gt

    def export_mesh(self, dir, name):
        """``<dir>/<name>_gt_pr.obj``: the ground truth in red and the prediction in green, one after the other"""
        path = os.path.join(dir, f"{name}_gt_pr.obj")
        with open(path, "w") as fh:
            base = 1
            for mesh, colour in ((self.tgt_mesh, "1 0 0"), (self.src_mesh, "0 1 0")):
                v, f = mesh.vertices.detach().cpu().numpy(), mesh.faces.detach().cpu().numpy()
                fh.writelines(f"v {x:.8g} {y:.8g} {z:.8g} {colour}\n" for x, y, z in v)
                fh.writelines(f"f {a + base} {b + base} {c + base}\n" for a, b, c in f)
                base += len(v)
        return path

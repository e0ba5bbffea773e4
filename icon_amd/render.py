"""Normal maps and depth maps of a mesh from ICON's four orthographic cameras - the forward renderer.

Replaces ``lib.common.render.Render.load_meshes`` / ``get_rgb_image`` / ``get_depth_map`` (a pytorch3d ``MeshRasterizer`` plus
``cleanShader``; call sites lib/dataset/TestDataset.py:289-299, apps/ICON.py:387-392, apps/infer.py:423/448/482) by ONE native
call, ``icon_render_normal`` (csrc/render_normal.hip; the rule is DESIGN.md 4.13).  No pytorch3d involved; there is no CPU path.

``Render.get_silhouette_image`` (the soft silhouette of the SMPL fit loop, apps/infer.py:205) is ``silhouette_device``: a
``torch.autograd.Function`` over ``icon_silhouette_forward`` / ``icon_silhouette_backward`` (csrc/silhouette.hip; DESIGN.md 4.14,
parity unpinned like 4.13) - differentiable with respect to the vertices.  The normal maps are differentiable on request
(``render_normal_device(differentiable=True)``, ``Render(normal_grad=True)``: ``icon_render_normal_backward``,
csrc/render_normal_bwd.hip); depth maps and ``pix_to_face`` are not.

The turntable video (``Render.get_rendered_video``, apps/infer.py:547-563) is ``render_turntable_device``: ONE native call,
``icon_render_turntable`` (csrc/turntable.hip; DESIGN.md 4.18, parity unpinned like 4.13), renders a mesh from a camera at every
requested azimuth and writes the frames' bytes on the device; ``Render.get_rendered_frames`` lays the panels of every loaded
mesh and the input images side by side.  Not differentiable.  Point clouds are not covered.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _lib
from ._lib import IconAmdError, check
from ._native import constants, faces_arg, need_device as _need_device, scratch_for, stream


def _check_cams(cam_ids) -> list:
    cams = [int(c) for c in cam_ids]
    if not 1 <= len(cams) <= 4 or any(c < 0 or c > 3 for c in cams):
        raise IconAmdError(f"render: cam_ids must be 1..4 values in 0..3, got {list(cam_ids)}")
    return cams


def _check_size(size) -> int:
    if int(size) != size or not 8 <= int(size) <= 2048:
        raise IconAmdError(f"render: size must be an integer in 8..2048, got {size}")
    return int(size)


def _check_mesh(what: str, verts, faces, need_float: bool) -> torch.Tensor:
    """the argument checks of ``render_normal_device`` and ``silhouette_device`` (``what``); -> the faces as the native calls read
    them: detached, int32 or int64, contiguous"""
    if not torch.is_tensor(verts) or verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] == 0:
        raise IconAmdError(f"render: verts must be a [V,3] tensor, got {tuple(getattr(verts, 'shape', ()))}")
    if need_float and not verts.dtype.is_floating_point:
        raise IconAmdError(f"render: verts must be a floating-point tensor, got {verts.dtype}")
    if not torch.is_tensor(faces) or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
        raise IconAmdError(f"render: faces must be a [F,3] tensor, got {tuple(getattr(faces, 'shape', ()))}")
    if faces.dtype.is_floating_point or faces.dtype == torch.bool:
        raise IconAmdError(f"render: faces must be an integer tensor, got {faces.dtype}")
    _need_device(what)
    if not (verts.is_cuda and faces.is_cuda) or verts.device != faces.device:
        raise IconAmdError(f"{what}: verts and faces must live on one HIP device (Render.load_meshes moves host data)")
    return faces_arg(faces)[0]


def turntable_cos_sin(angles) -> np.ndarray:
    """azimuths in degrees (any finite floats: negative ones and those >= 360 included) -> float32 ``[n,2]``: the pairs
    ``(cos, sin)`` of ``pi / 180 * angle`` evaluated in float64 and rounded - exactly ``(1,0)``, ``(0,1)``, ``(-1,0)``, ``(0,-1)``
    at the whole multiples of 90, where the turntable camera is one of the four fixed ones.  The only place that
    turns angles into what ``icon_render_turntable`` projects with; needs no device."""
    a = np.asarray(list(angles) if not isinstance(angles, np.ndarray) else angles, dtype=np.float64).reshape(-1)
    if not np.isfinite(a).all():
        raise IconAmdError("render: turntable angles must be finite")
    theta = np.pi / 180 * a
    pairs = np.stack([np.cos(theta), np.sin(theta)], 1).astype(np.float32)
    quarter = a / 90.0
    whole = quarter == np.round(quarter)
    pairs[whole] = np.array([(1, 0), (0, 1), (-1, 0), (0, -1)], np.float32)[np.mod(quarter[whole], 4).astype(np.int64)]
    return pairs


def _mesh_args(v, f, cams, size):
    """the leading arguments every native call of this module takes: the mesh, the cameras, the image size"""
    return (_lib.ptr(v), C.c_int64(v.shape[0]), _lib.ptr(f), C.c_int64(f.shape[0]), C.c_int(1 if f.dtype == torch.int64 else 0),
            (C.c_int * len(cams))(*cams), C.c_int(len(cams)), C.c_int(size))


def _rn_forward(v, f, cams, size, return_depth, return_faces):
    """the native forward call on a float32, contiguous ``v`` and an int32 / int64, contiguous ``f``"""
    dev, n = v.device, len(cams)
    L = _lib.lib()
    with torch.cuda.device(dev):
        scratch = scratch_for(dev, "icon_render_bytes", C.c_int64(v.shape[0]), C.c_int64(f.shape[0]), C.c_int(size), C.c_int(n))
        images = torch.empty((n, 3, size, size), dtype=torch.float32, device=dev)
        depth = torch.empty((n, size, size), dtype=torch.float32, device=dev) if return_depth else None
        pix = torch.empty((n, size, size), dtype=torch.int32, device=dev) if return_faces else None
        check(L.icon_render_normal(*_mesh_args(v, f, cams, size), _lib.ptr(images), _lib.ptr(depth), _lib.ptr(pix),
                                   _lib.ptr(scratch), C.c_int64(scratch.numel()), stream()), "icon_render_normal")
    return images, depth, pix


class _RenderNormal(torch.autograd.Function):
    """verts (float32, contiguous, on the device) -> images, depth, pix_to_face; only ``images`` is differentiable, and only in
    ``verts``.  The forward is the unchanged native call with ``return_faces``; the backward is ONE native call,
    ``icon_render_normal_backward`` (csrc/render_normal_bwd.hip)"""

    @staticmethod
    def forward(ctx, v, f, cams, size):
        images, depth, pix = _rn_forward(v, f, cams, size, True, True)
        ctx.save_for_backward(v, f, pix)
        ctx.cams, ctx.size = cams, size
        ctx.mark_non_differentiable(depth, pix)
        return images, depth, pix

    @staticmethod
    def backward(ctx, grad_images, _grad_depth, _grad_pix):
        v, f, pix = ctx.saved_tensors
        cams, size = ctx.cams, ctx.size
        g = grad_images.to(torch.float32).contiguous()
        L = _lib.lib()
        with torch.cuda.device(v.device):
            scratch = scratch_for(v.device, "icon_render_normal_backward_bytes", C.c_int64(v.shape[0]), C.c_int64(f.shape[0]), C.c_int(size),
                                  C.c_int(len(cams)))                          # this thread's and this stream's: autograd has its own
            grad_verts = torch.empty_like(v)
            check(L.icon_render_normal_backward(*_mesh_args(v, f, cams, size), _lib.ptr(pix), _lib.ptr(g), _lib.ptr(grad_verts),
                                                _lib.ptr(scratch), C.c_int64(scratch.numel()), stream()), "icon_render_normal_backward")
        return grad_verts, None, None, None


def render_normal_device(verts: torch.Tensor, faces: torch.Tensor, cam_ids: Sequence[int] = (0, 2), size: int = 512,
                         return_depth: bool = False, return_faces: bool = False, differentiable: bool = False):
    """``verts [V,3]`` (float), ``faces [F,3]`` (int32 or int64, read in place), both on one HIP device ->
    ``images [n,3,size,size]`` float32 in [-1,1] there, view k from camera ``cam_ids[k]`` (0: from +z, 1: from +x, 2: from -z,
    3: from -x; +y is up, the [-1,1] cube fills the image; background 0), then ``depth [n,size,size]`` (view depth, background
    -1) with ``return_depth`` and ``pix_to_face [n,size,size]`` int32 (background -1) with ``return_faces``.  With exactly two
    views the planes of camera 2 are mirrored left-right, as the reference's ``get_rgb_image`` does.  ONE native call enqueued
    on the current stream: nothing is allocated by it, nothing read back, the stream is not waited for - so a face that names a
    vertex that does not exist cannot raise here; it is skipped.  The scratch is cached per (thread, device, stream).

    ``differentiable=False`` (the default) renders from a detached copy: nothing returned requires grad.  With ``True`` the
    same forward call runs inside a ``torch.autograd.Function``: ``images`` is differentiable with respect to ``verts`` (which
    must be floating-point; the gradient flows back through the float32 cast), its backward is one native call
    (``icon_render_normal_backward``; the rule is DESIGN.md 4.15: the winner per pixel and the clamp pattern carry no
    gradient; no floating-point atomics - equal bytes from run to run).  ``depth`` and ``pix_to_face`` stay non-differentiable."""
    cams, size = _check_cams(cam_ids), _check_size(size)
    f = _check_mesh("render_normal_device", verts, faces, need_float=differentiable)
    if differentiable:
        v = verts.to(torch.float32).contiguous()                             # differentiable: the gradient flows back through the cast
        images, depth, pix = _RenderNormal.apply(v, f, tuple(cams), size)
    else:
        v = verts.detach().to(torch.float32).contiguous()
        images, depth, pix = _rn_forward(v, f, cams, size, return_depth, return_faces)
    out = (images,) + ((depth,) if return_depth else ()) + ((pix,) if return_faces else ())
    return out if len(out) > 1 else images


def render_turntable_device(verts: torch.Tensor, faces: torch.Tensor, angles, size: int = 512, out: torch.Tensor = None, x0: int = 0,
                            return_images: bool = False, return_depth: bool = False, return_faces: bool = False):
    """``verts [V,3]`` (float), ``faces [F,3]`` (int32 or int64, read in place), both on one HIP device; ``angles``: 1..1024
    azimuths in degrees (``turntable_cos_sin``) -> the frames of the turntable video, uint8 ``[n,size,size,3]`` there: frame k
    is the normal map seen from ``(100 cos a_k, 0, 100 sin a_k)`` as bytes ``(t * 255)`` truncated, channels x, y, z, background
    127 (the reference's ``(renderer(mesh)[0, :, :, :3] * 255.0).astype(np.uint8)``).  With ``out=`` - a
    contiguous uint8 ``[n,size,W,3]`` canvas on the same device - the frames go into columns ``x0 .. x0 + size - 1`` of it, no
    other byte of it is touched, and ``out`` is returned.  Then ``images [n,3,size,size]`` with ``return_images``, ``depth`` with
    ``return_depth`` and ``pix_to_face`` with ``return_faces``, formatted as ``render_normal_device``'s; no view is mirrored.
    ONE native call on the current stream, whatever n: the vertex normals are computed once, the views are rasterised in
    chunks inside the call (the scratch, cached per (thread, device, stream) like ``render_normal_device``'s, does not grow
    with n).  Nothing is allocated by it, nothing read back, the stream is not waited for; equal bytes from run to run.  Not
    differentiable: it renders from a detached copy."""
    size = _check_size(size)
    pairs = turntable_cos_sin(angles)
    n = len(pairs)
    if not 1 <= n <= 1024:
        raise IconAmdError(f"render: a turntable call takes 1..1024 angles, got {n}")
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.uint8:
            raise IconAmdError(f"render: out must be a uint8 tensor, got {getattr(out, 'dtype', type(out))}")
        if out.dim() != 4 or out.shape[0] != n or out.shape[1] != size or out.shape[3] != 3 or not out.is_contiguous():
            raise IconAmdError(f"render: out must be a contiguous [{n},{size},W,3] canvas, got {tuple(out.shape)}")
        if int(x0) != x0 or not 0 <= int(x0) <= out.shape[2] - size:
            raise IconAmdError(f"render: the panel x0 .. x0 + {size} - 1 must lie inside the canvas' width {out.shape[2]}, got x0 = {x0}")
    elif x0 != 0:
        raise IconAmdError(f"render: x0 needs a canvas (out=), got x0 = {x0}")
    f = _check_mesh("render_turntable_device", verts, faces, need_float=False)
    v = verts.detach().to(torch.float32).contiguous()
    dev = v.device
    if out is not None and out.device != dev:
        raise IconAmdError("render_turntable_device: out must live on the device of the mesh")
    L = _lib.lib()
    with torch.cuda.device(dev):
        scratch = scratch_for(dev, "icon_render_turntable_bytes", C.c_int64(v.shape[0]), C.c_int64(f.shape[0]), C.c_int(size), C.c_int(n))
        cos_sin, = constants(dev, pairs)                                     # the video asks for the same chunks of angles for every mesh
        frames = out if out is not None else torch.empty((n, size, size, 3), dtype=torch.uint8, device=dev)
        images = torch.empty((n, 3, size, size), dtype=torch.float32, device=dev) if return_images else None
        depth = torch.empty((n, size, size), dtype=torch.float32, device=dev) if return_depth else None
        pix = torch.empty((n, size, size), dtype=torch.int32, device=dev) if return_faces else None
        check(L.icon_render_turntable(_lib.ptr(v), C.c_int64(v.shape[0]), _lib.ptr(f), C.c_int64(f.shape[0]), C.c_int(1 if f.dtype == torch.int64 else 0),
                                      _lib.ptr(cos_sin), C.c_int(n), C.c_int(size), _lib.ptr(frames), C.c_int64(frames.shape[2]), C.c_int64(int(x0)),
                                      _lib.ptr(images), _lib.ptr(depth), _lib.ptr(pix), _lib.ptr(scratch), C.c_int64(scratch.numel()), stream()),
              "icon_render_turntable")
    res = (frames,) + tuple(t for t in (images, depth, pix) if t is not None)
    return res if len(res) > 1 else frames


def _sil_scratch(v, f, cams, size):
    return scratch_for(v.device, "icon_silhouette_bytes", C.c_int64(v.shape[0]), C.c_int64(f.shape[0]), C.c_int(size), C.c_int(len(cams)))


class _Silhouette(torch.autograd.Function):
    """verts (float32, contiguous, on the device) -> alpha; the other arguments are not differentiable"""

    @staticmethod
    def forward(ctx, v, f, cams, size):
        with torch.cuda.device(v.device):
            scratch = _sil_scratch(v, f, cams, size)
            alpha = torch.empty((len(cams), size, size), dtype=torch.float32, device=v.device)
            check(_lib.lib().icon_silhouette_forward(*_mesh_args(v, f, cams, size), _lib.ptr(alpha), _lib.ptr(scratch),
                                                     C.c_int64(scratch.numel()), stream()), "icon_silhouette_forward")
        ctx.save_for_backward(v, f, alpha)
        ctx.cams, ctx.size = cams, size
        return alpha

    @staticmethod
    def backward(ctx, grad_alpha):
        v, f, alpha = ctx.saved_tensors
        cams, size = ctx.cams, ctx.size
        g = grad_alpha.to(torch.float32).contiguous()
        with torch.cuda.device(v.device):
            scratch = _sil_scratch(v, f, cams, size)                          # this thread's and this stream's: autograd has its own
            grad_verts = torch.empty_like(v)
            check(_lib.lib().icon_silhouette_backward(*_mesh_args(v, f, cams, size), _lib.ptr(alpha), _lib.ptr(g), _lib.ptr(grad_verts),
                                                      _lib.ptr(scratch), C.c_int64(scratch.numel()), stream()), "icon_silhouette_backward")
        return grad_verts, None, None, None


def silhouette_device(verts: torch.Tensor, faces: torch.Tensor, cam_ids: Sequence[int] = (0, 2), size: int = 512) -> torch.Tensor:
    """``verts [V,3]`` (float), ``faces [F,3]`` (int32 or int64, read in place), both on one HIP device -> the soft silhouette
    ``alpha [n,size,size]`` float32 in [0,1] there (background 0), view k from camera ``cam_ids[k]`` (the cameras and the
    left-right mirror of camera 2 in a two-view call are ``render_normal_device``'s).  Differentiable with respect to ``verts``
    (``torch.autograd.Function``: the forward saves ``alpha``, the backward is one native call returning ``grad_verts``; candidate
    set and back-face culling carry no gradient).  Every candidate of a pixel enters the product - pytorch3d keeps the 50 nearest
    (DESIGN.md 4.14).  Each direction is ONE native call on the current stream: nothing allocated by it, nothing read back, no
    floating-point atomics - equal bytes from run to run.  A face that names a missing vertex is skipped."""
    cams, size = _check_cams(cam_ids), _check_size(size)
    f = _check_mesh("silhouette_device", verts, faces, need_float=True)
    v = verts.to(torch.float32).contiguous()                                 # differentiable: the gradient flows back through the cast
    return _Silhouette.apply(v, f, tuple(cams), size)


def _mirror_cam2(cam_ids, cams) -> bool:
    """do ``get_rgb_image`` / ``get_silhouette_image`` have to mirror camera 2 themselves?  The native call mirrors it when IT
    renders exactly two views; the reference decides by ``len(cam_ids)`` (duplicates included)"""
    return (len(cam_ids) == 2) != (len(cams) == 2) and 2 in cams


class Render:
    """Drop-in for ``lib.common.render.Render``'s normal maps, depth maps, soft silhouettes and turntable video::

        render = Render(size=512, device=torch.device("cuda:0"))
        render.load_meshes(verts, faces)
        T_normal_F, T_normal_B = render.get_rgb_image()          # [1,3,S,S] each, in [-1,1]
        depth_F, depth_B = render.get_depth_map(cam_ids=[0, 2])   # [S,S] each
        sil_F, sil_B = render.get_silhouette_image()             # [1,S,S] each, differentiable in verts
        render.load_meshes([verts_pr, verts], [faces_pr, faces])
        render.get_rendered_video([image, normal_F], "turntable.mp4")   # or: for frames in render.get_rendered_frames([...])

    The maps of one set of cameras are rendered once per ``load_meshes`` (one native call gives images and depths); the
    tensors handed out are views of that result.  ``Render(size, device, normal_grad=True)`` makes ``get_rgb_image``
    differentiable in the vertices as well (see there)."""

    def __init__(self, size: int = 512, device=None, normal_grad: bool = False):
        """``normal_grad=True`` makes ``get_rgb_image`` differentiable in the vertices ``load_meshes`` was given (the normal-map
        terms of the fit loop and the cloth loop, apps/infer.py:200-217 / :448-456); by default it is not, as before."""
        self.size = _check_size(size)
        self.normal_grad = bool(normal_grad)
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        if self.device.type != "cuda":
            raise IconAmdError(f"Render: device must be a HIP device, got {self.device} (there is no CPU fallback)")
        self.meshes = None
        self._live = None
        self._cache = {}

    def _device(self) -> torch.device:
        _need_device("Render")
        return self.device if self.device.index is not None else torch.device("cuda", torch.cuda.current_device())

    def load_meshes(self, verts, faces) -> None:
        """``verts [V,3]`` / ``faces [F,3]``: tensors or arrays, on the host or the device (a leading batch axis of 1 is dropped).
        Lists are taken element by element, as the reference does; element 0 is what the get_* calls render.  The normal and
        depth maps are rendered from detached copies, as before; when element 0's vertices are a floating-point device tensor
        that requires grad, a reference to that tensor is kept next to them for ``get_silhouette_image`` - and, with
        ``normal_grad=True``, ``get_rgb_image`` - to back-propagate into."""
        dev = self._device()
        if not isinstance(verts, (list, tuple)):
            verts, faces = [verts], [faces]
        v0 = verts[0] if len(verts) else None
        self._live = None
        if torch.is_tensor(v0) and v0.is_cuda and v0.dtype.is_floating_point and v0.requires_grad:
            self._live = v0[0] if v0.dim() == 3 and v0.shape[0] == 1 else v0
        meshes = []
        for v, f in zip(verts, faces):
            v = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v)
            f = torch.as_tensor(np.asarray(f) if not torch.is_tensor(f) else f)
            if v.dim() == 3 and v.shape[0] == 1:
                v = v[0]
            if f.dim() == 3 and f.shape[0] == 1:
                f = f[0]
            if f.dtype.is_floating_point or f.dtype == torch.bool:
                raise IconAmdError(f"render: faces must be an integer tensor, got {f.dtype}")
            meshes.append((v.detach().to(dev, torch.float32), f.detach().to(dev) if f.dtype in (torch.int32, torch.int64) else f.detach().to(dev, torch.int64)))
        self.meshes = meshes
        self._cache = {}

    def _render(self, cams: tuple):
        _need_device("Render")
        if not self.meshes:
            raise IconAmdError("Render: load_meshes has not been called")
        if cams not in self._cache:
            v, f = self.meshes[0]
            self._cache[cams] = render_normal_device(v, f, cams, self.size, return_depth=True)
        return self._cache[cams]

    def get_rgb_image(self, cam_ids=[0, 2]):
        """-> one ``[1,3,S,S]`` tensor per requested camera, in ascending camera order (the reference walks its camera list and
        keeps the requested ones); camera 2 is mirrored left-right when ``len(cam_ids) == 2``.  By default not differentiable:
        rendered once per ``load_meshes`` from the detached copy of the mesh, whatever ``load_meshes`` was given.  A
        ``Render(normal_grad=True)`` renders from the live tensor instead - a fresh differentiable call every time, never the
        cached images - when ``load_meshes`` kept one (a floating-point device tensor that requires grad) and grad mode is on;
        under ``torch.no_grad()`` or after a detached ``load_meshes`` it takes the cached path like the default."""
        _check_cams(cam_ids)
        cams = tuple(c for c in range(4) if c in [int(x) for x in cam_ids])
        if self.normal_grad and self._live is not None and torch.is_grad_enabled():
            _need_device("Render")
            v, f = self.meshes[0]
            images, depth = render_normal_device(self._live.to(v.device), f, cams, self.size, return_depth=True, differentiable=True)
            if cams not in self._cache:                                      # the same bytes as the detached render: get_depth_map needs no second call
                self._cache[cams] = (images.detach(), depth)
        else:
            images, _ = self._render(cams)
        out = [images[k:k + 1] for k in range(len(cams))]
        if _mirror_cam2(cam_ids, cams):                                    # duplicates in cam_ids: the native call decided by its own count
            k = cams.index(2)
            out[k] = torch.flip(out[k], dims=[3])
        return out

    def get_depth_map(self, cam_ids=[0, 2]):
        """-> one ``[S,S]`` tensor per entry of ``cam_ids``, in that order; camera 2 is ALWAYS mirrored left-right (the
        reference's get_depth_map does not look at the number of views).  Not differentiable, like ``get_rgb_image``."""
        cams = tuple(_check_cams(cam_ids))
        _, depth = self._render(cams)
        out = [depth[k] for k in range(len(cams))]
        if len(cams) != 2:
            out = [torch.fliplr(d) if c == 2 else d for c, d in zip(cams, out)]
        return out

    def get_silhouette_image(self, cam_ids=[0, 2]):
        """-> one ``[1,S,S]`` soft silhouette per requested camera, in ascending camera order; camera 2 is mirrored left-right
        (``dims=[2]``) when ``len(cam_ids) == 2`` - the reference's signature and mirroring.  Differentiable: when ``load_meshes``
        was given a floating-point device tensor that requires grad, ``backward()`` reaches it (``silhouette_device``)."""
        _check_cams(cam_ids)
        cams = tuple(c for c in range(4) if c in [int(x) for x in cam_ids])
        _need_device("Render")
        if not self.meshes:
            raise IconAmdError("Render: load_meshes has not been called")
        v, f = self.meshes[0]
        if self._live is not None:
            v = self._live.to(v.device)
        alpha = silhouette_device(v, f, cams, self.size)
        out = [alpha[k:k + 1] for k in range(len(cams))]
        if _mirror_cam2(cam_ids, cams):
            k = cams.index(2)
            out[k] = torch.flip(out[k], dims=[2])
        return out

    def get_rendered_frames(self, images, angles=range(360), chunk: int = 30):
        """the frames of the turntable video, ``chunk`` at a time: a generator of uint8 DEVICE tensors ``[k,S,W,3]``.  Every frame is
        ``[images resized ..., one panel per loaded mesh ...]`` side by side, in the reference's order, with
        ``W = S * len(meshes) + new_w * len(images)``.  ``images``: host uint8 ``[H,W,3]`` arrays, all resized ONCE to the shape
        the first one gives, as the reference resizes them per frame (``Image.fromarray(img).resize((new_w, S))``,
        ``new_shape = around(S / H * (H, W))``, then the channels reversed), uploaded once and broadcast into each chunk's
        canvas; every mesh's panel is one ``render_turntable_device`` call per chunk, written in place.  Nothing is copied to
        the host."""
        _need_device("Render")
        if not self.meshes:
            raise IconAmdError("Render: load_meshes has not been called")
        angles = [float(a) for a in angles]
        chunk = int(chunk)
        if not 1 <= chunk <= 1024:
            raise IconAmdError(f"render: chunk must be 1..1024 frames, got {chunk}")
        S, dev = self.size, self._device()
        panels = []
        if len(images):
            from PIL import Image
            old = np.array(np.asarray(images[0]).shape[:2])
            new_w = int(np.around((S / old[0]) * old)[1])
            for img in images:
                img = np.asarray(img)
                if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
                    raise IconAmdError(f"render: images must be uint8 [H,W,3] arrays, got {img.dtype} {img.shape}")
                small = np.array(Image.fromarray(img).resize((new_w, S))).astype(np.uint8)[:, :, [2, 1, 0]]
                panels.append(torch.from_numpy(np.ascontiguousarray(small)).to(dev))
        left = sum(p.shape[1] for p in panels)
        W = left + S * len(self.meshes)
        for a0 in range(0, len(angles), chunk):
            part = angles[a0:a0 + chunk]
            canvas = torch.empty((len(part), S, W, 3), dtype=torch.uint8, device=dev)
            x = 0
            for p in panels:
                canvas[:, :, x:x + p.shape[1]] = p
                x += p.shape[1]
            for k, (v, f) in enumerate(self.meshes):
                render_turntable_device(v, f, part, S, out=canvas, x0=left + k * S)
            yield canvas

    def get_rendered_video(self, images, save_path):
        """the reference's signature: 360 frames, one per whole degree, written to ``save_path`` with ``cv2.VideoWriter`` (``mp4v``,
        30 fps, frame size ``(W, S)``) - each chunk of ``get_rendered_frames`` is copied to the host once.  Without ``cv2`` it raises;
        ``get_rendered_frames`` gives the same frames to any other writer.  ``cv2`` is not installed where this was developed: the
        tests put a recording stub in its place, the real writer is UNVERIFIED.  Unlike the reference, the call leaves the four
        cameras of ``get_rgb_image`` alone."""
        try:
            import cv2
        except ImportError as e:
            raise IconAmdError("Render.get_rendered_video needs cv2 (opencv-python) for the video file; "
                               "Render.get_rendered_frames yields the same frames on the device for any other writer") from e
        video = None
        try:
            for frames in self.get_rendered_frames(images):
                if video is None:
                    video = cv2.VideoWriter(save_path, cv2.VideoWriter_fourcc(*"mp4v"), 30, (frames.shape[2], self.size))
                for frame in frames.cpu().numpy():
                    video.write(frame)
        finally:
            if video is not None:
                video.release()

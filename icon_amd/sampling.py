"""Training samples on the device: what ``PIFuDataset.get_sampling_geo`` (``lib/dataset/PIFuDataset.py:483-607``, called per
item at :226-229) draws around a scan and labels by ``trimesh``'s ``contains`` on a CPU worker - here one stream-ordered native
call (csrc/sample_geo.hip: ``icon_sample_geo``) against a scan that stays resident as a ``MeshHandle``.

The rule is DESIGN.md 4.21: surface samples along the vertex normals, uniform samples of the image cube, z-ray samples, a keyed
shuffle, the inside test of the scan, the balancing truncation.  Every draw is a pure function of (seed, stream, index) -
Philox4x32-10 - so a call is reproducible from its seed alone; tests/sampling_oracle.py restates the rule in numpy and
tests/test_sampling.py pins it to a recorded run of the reference.

Unpinned: the labels.  The reference asks trimesh's ray-parity ``contains``; this library asks its own inside test (the rule of
kaolin's ``check_sign`` as DESIGN.md 2 defines it).  The two agree except for points within rounding of the surface.  ``is_sdf=True``
is refused: no shipped config sets ``sdf: True``.  Everything per sample needs a HIP device and there is no CPU path for it.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import IconAmdError, check
from ._native import scratch_for, stream
from .garment import _check_device, _check_points


class ScanMesh:
    """A training scan on the device, built once per scan: ``verts [V,3]`` floating point, ``faces [F,3]`` integer (device
    tensors), ``vert_normals [V,3]`` or None - the handle's own vertex normals (the shared S1 pipeline) then.  Owns the
    ``MeshHandle`` (``.handle``: BVH and ray bins, for the labels and for ``sdf_query``), ``.verts`` and ``.vert_normals``."""

    def __init__(self, verts: torch.Tensor, faces: torch.Tensor, vert_normals: Optional[torch.Tensor] = None):
        from .engine import MeshHandle
        what = "ScanMesh"
        _check_points(verts, "verts", what)
        if not torch.is_tensor(faces) or faces.dtype.is_floating_point or faces.dtype == torch.bool or faces.dim() != 2 or faces.shape[1] != 3:
            raise IconAmdError(f"{what}: faces must be an integer tensor [F,3], got "
                               f"{(faces.dtype, list(faces.shape)) if torch.is_tensor(faces) else type(faces).__name__}")
        if vert_normals is not None:
            _check_points(vert_normals, "vert_normals", what)
            if vert_normals.shape[0] != verts.shape[0]:
                raise IconAmdError(f"{what}: vert_normals must be [{verts.shape[0]},3], got {list(vert_normals.shape)}")
        if verts.shape[0] == 0 or faces.shape[0] == 0:
            raise IconAmdError(f"{what}: the scan is empty ({verts.shape[0]} vertices, {faces.shape[0]} faces)")
        dev = _check_device(what, verts=verts, faces=faces, vert_normals=vert_normals)
        self.device = dev
        self.verts = verts.detach().to(torch.float32).contiguous()
        self.faces = faces.detach().contiguous()
        V = self.verts.shape[0]
        with torch.cuda.device(dev):
            self.handle = MeshHandle(self.verts, self.faces, torch.zeros((V, 3), device=dev), torch.zeros(V, device=dev))
            self.vert_normals = (self.handle.vertex_normals() if vert_normals is None
                                 else vert_normals.detach().to(torch.float32).contiguous())
        self.V, self.F = V, int(faces.shape[0])


def _calib_pair(calib, what: str):
    """``calib`` [4,4] or [3,4] (tensor or array; a device tensor is copied to the host, which waits for it) -> the float64 rows
    [12] of the affine and of its inverse, inverted once in float64"""
    m = calib.detach().cpu().numpy() if torch.is_tensor(calib) else np.asarray(calib)
    if m.dtype.kind not in "fiu" or m.shape not in ((4, 4), (3, 4)):
        raise IconAmdError(f"{what}: calib must be a [4,4] or [3,4] matrix of numbers, got {m.dtype} {list(m.shape)}")
    full = np.eye(4, dtype=np.float64)
    full[:3] = m[:3].astype(np.float64)
    if not np.isfinite(full).all():
        raise IconAmdError(f"{what}: calib has an entry that is not finite")
    try:
        inv = np.linalg.inv(full)
    except np.linalg.LinAlgError:
        raise IconAmdError(f"{what}: calib is singular") from None
    if not np.isfinite(inv).all():
        raise IconAmdError(f"{what}: calib is singular")
    return np.ascontiguousarray(full[:3].reshape(12)), np.ascontiguousarray(inv[:3].reshape(12))


def sample_count(num_sample_geo: int, zray: bool, ray_sample_num: int) -> int:
    """n of DESIGN.md 4.21: the slots of the shuffled list, 4 N surface + N // 4 space + (z-ray: 4 N R)"""
    N = int(num_sample_geo)
    return 4 * N + N // 4 + (4 * N * int(ray_sample_num) if zray else 0)


def sample_geo_device(scan: ScanMesh, calib, num_sample_geo: int, sigma_geo: float, *, zray_type: bool = False,
                      ray_sample_num: int = 1, is_valid: bool = False, seed: int, return_all: bool = False):
    """``get_sampling_geo`` as ONE native call on the current stream -> ``(samples [N,3] f32, labels [N] f32, counts int32 [2])``
    on the scan's device: ``counts = (inside rows, outside rows)``; rows past their sum (only when the outside samples run
    short) are zero with label 0.  ``calib``: the item's [4,4] (or [3,4]) calibration, host data as the loader holds it.  The
    z-ray samples are drawn when ``zray_type and not is_valid``.  ``seed``: any integer, taken modulo 2^64 - equal seeds give
    equal bytes.  ``return_all``: a fourth value, dict(all_samples [n,3] f32, all_inside [n] bool, source [n] int32 - the
    source index ``perm(i)`` of slot i -, vertex [n] int32 - the vertex drawn for it, -1 for a space sample): the shuffled list
    before balancing.  Nothing is waited for; the scratch is cached per (thread, device, stream)."""
    what = "sample_geo_device"
    if not isinstance(scan, ScanMesh):
        raise IconAmdError(f"{what}: scan must be a ScanMesh, got {type(scan).__name__}")
    N, R = int(num_sample_geo), int(ray_sample_num)
    if N < 1 or N >= 2 ** 24:
        raise IconAmdError(f"{what}: num_sample_geo must be 1 .. 2^24 - 1, got {N}")
    if R < 1 or R > 64:
        raise IconAmdError(f"{what}: ray_sample_num must be 1 .. 64, got {R}")
    sigma = float(sigma_geo)
    if not np.isfinite(sigma):
        raise IconAmdError(f"{what}: sigma_geo is not finite")
    zray = bool(zray_type) and not bool(is_valid)
    n = sample_count(N, zray, R)
    if n >= 2 ** 31:
        raise IconAmdError(f"{what}: {n} samples before balancing; the call takes fewer than 2^31")
    cal, cal_inv = _calib_pair(calib, what)
    dev = scan.device
    L = _lib.lib()
    with torch.cuda.device(dev):
        scratch = scratch_for(dev, "icon_sample_geo_bytes", C.c_int64(n))
        samples = torch.empty((N, 3), dtype=torch.float32, device=dev)
        labels = torch.empty(N, dtype=torch.float32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        extra = None
        if return_all:
            extra = dict(all_samples=torch.empty((n, 3), dtype=torch.float32, device=dev),
                         all_inside=torch.empty(n, dtype=torch.uint8, device=dev),
                         source=torch.empty(n, dtype=torch.int32, device=dev), vertex=torch.empty(n, dtype=torch.int32, device=dev))
        opt = [_lib.ptr(extra[k]) if extra else C.c_void_p(0) for k in ("all_samples", "all_inside", "source", "vertex")]
        check(L.icon_sample_geo(scan.handle.h, _lib.ptr(scan.verts), _lib.ptr(scan.vert_normals),
                                cal.ctypes.data_as(C.POINTER(C.c_double)), cal_inv.ctypes.data_as(C.POINTER(C.c_double)),
                                C.c_int64(N), C.c_double(sigma), C.c_int(int(zray)), C.c_int(R), C.c_uint64(int(seed) % 2 ** 64),
                                _lib.ptr(samples), _lib.ptr(labels), _lib.ptr(counts), *opt,
                                _lib.ptr(scratch), C.c_int64(scratch.numel()), stream()), "icon_sample_geo")
    if extra:
        extra["all_inside"] = extra["all_inside"].bool()
        return samples, labels, counts, extra
    return samples, labels, counts


class GeoSampler:
    """The reference's entry point: ``opt`` carries ``num_sample_geo``, ``sigma_geo``, ``zray_type`` and ``ray_sample_num`` (its
    ``cfg.dataset``; attributes or keys).  ``get_sampling_geo(data_dict, is_valid, is_sdf, seed=...)`` takes ``data_dict['mesh']`` -
    a ``ScanMesh`` - and ``data_dict['calib']`` and returns ``{'samples_geo' [M,3], 'labels_geo' [M]}`` on the device, sliced to
    the rows the call filled (M = num_sample_geo unless the outside samples ran short): one synchronisation, for the counts."""

    def __init__(self, opt):
        get = (lambda k, d=None: opt.get(k, d)) if isinstance(opt, dict) else (lambda k, d=None: getattr(opt, k, d))
        self.num_sample_geo, self.sigma_geo = get("num_sample_geo"), get("sigma_geo")
        if self.num_sample_geo is None or self.sigma_geo is None:
            raise IconAmdError("GeoSampler: opt needs num_sample_geo and sigma_geo")
        self.zray_type, self.ray_sample_num = bool(get("zray_type", False)), int(get("ray_sample_num", 1) or 1)

    def get_sampling_geo(self, data_dict, is_valid: bool = False, is_sdf: bool = False, *, seed: int):
        if is_sdf:
            raise IconAmdError("get_sampling_geo: is_sdf=True (HoppeMesh.query) is not supported - no shipped config sets sdf: True")
        if not isinstance(data_dict, dict) or "mesh" not in data_dict or "calib" not in data_dict:
            raise IconAmdError("get_sampling_geo: data_dict needs 'mesh' (a ScanMesh) and 'calib'")
        samples, labels, counts = sample_geo_device(data_dict["mesh"], data_dict["calib"], self.num_sample_geo, self.sigma_geo,
                                                    zray_type=self.zray_type, ray_sample_num=self.ray_sample_num, is_valid=is_valid,
                                                    seed=seed)
        m = int(counts.sum())
        return {"samples_geo": samples[:m], "labels_geo": labels[:m]}


def smpl_signs_device(smpl_mesh, samples: torch.Tensor, calib) -> torch.Tensor:
    """``pts_signs`` of ``load_smpl`` (``PIFuDataset.py:414-420``): ``2 * (inside - 0.5)`` of ``samples [M,3]`` projected by ``calib``
    (float32, as the reference's ``projection(...).float()`` of float32 samples) against the SMPL ``MeshHandle`` -> f32 ``[M]``"""
    from .engine import MeshHandle
    what = "smpl_signs_device"
    if not isinstance(smpl_mesh, MeshHandle):
        raise IconAmdError(f"{what}: smpl_mesh must be a MeshHandle, got {type(smpl_mesh).__name__}")
    _check_points(samples, "samples", what)
    dev = _check_device(what, samples=samples)
    m = calib.detach().cpu().numpy() if torch.is_tensor(calib) else np.asarray(calib)
    if m.dtype.kind not in "fiu" or m.shape not in ((4, 4), (3, 4)):
        raise IconAmdError(f"{what}: calib must be a [4,4] or [3,4] matrix of numbers, got {m.dtype} {list(m.shape)}")
    cal = torch.from_numpy(np.ascontiguousarray(m[:3], dtype=np.float32)).to(dev, non_blocking=True)
    with torch.cuda.device(dev):
        pts = samples.detach().to(torch.float32) @ cal[:, :3].T + cal[:, 3]
        inside = smpl_mesh.sdf_query(pts)["inside"]
    return 2.0 * (inside.to(torch.float32) - 0.5)

"""Garment extraction on the device: what ``extract_cloth`` (``lib/common/cloth_extraction.py:75-170``, the last block of
``apps/infer.py``, lines 565-605) cuts out of the reconstruction for a DeepFashion2 segmentation - without matplotlib, sklearn
and trimesh.

The rule is DESIGN.md 4.19: a vertex is *selected* when its (x, y) lies inside any of the garment's polygons (the crossings test
of ``matplotlib.path.Path.contains_points``), it is *kept* unless its nearest SMPL vertex (``KNeighborsClassifier(n_neighbors=1)``:
the lowest index of the smallest float64 squared distance) carries a body part the garment type excludes, a face is kept when any
corner is, and the kept faces come out in order over the vertices they name, renumbered.  Every decision is an exact float64
comparison on the float32 coordinates, so the native calls (csrc/garment.hip: ``icon_extract_cloth``, ``icon_nearest_vertex``) are
held to EQUALITY with tests/garment_oracle.py, which tests/test_garment.py pins to matplotlib, sklearn and the reference function.

The polygon projection, the part table and the garment-type lists are host plumbing (numpy, the reference's arithmetic restated);
everything per vertex and per face needs a HIP device and there is no CPU path for it.  The library ships no copy of the
reference's ``smpl_vert_segmentation.json``: the caller reads it and passes the dict.

Unpinned: ``trimesh.Trimesh(vertices, faces)`` with its default ``process=True`` would also merge coincident vertices; nothing is
merged here (the meshes of this pipeline have none).  Coordinates given in float64 are rounded to float32 first.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import IconAmdError, check
from ._native import faces_arg, need_device, scratch_for, stream

# csrc/garment.hip: kPolyTile, kSrcTile, kSrcSplit - the sizes at which the kernels take another path (tests pick shapes around them)
POLY_TILE, SRC_TILE, SRC_SPLIT = 256, 512, 128
# csrc/compact_device.h: kCompactRound * kCompactBlock - the vertices or faces above which the scan of the block counts carries a
# total into another round
SCAN_ROUND = 8192 * 256

# lib/common/cloth_extraction.py:117-133 ('rightHand' is listed twice there)
_BASE_PARTS = ["rightHand", "leftToeBase", "leftFoot", "rightFoot", "head", "leftHandIndex1", "rightHandIndex1", "rightToeBase",
               "leftHand", "rightHand"]
_SHORT_SLEEVES, _NO_SLEEVES, _SHORTS = (1, 3, 10), (5, 6, 12, 13, 8, 9), (7,)


# ---- host plumbing -----------------------------------------------------------------------------------------------------------

def part_labels(vert_segmentation: dict, n_verts: int):
    """``smpl_to_recon_labels``' ``y[val] = key`` in dict order (cloth_extraction.py:55-60) -> ``(names, labels int32 [n_verts])``,
    ``labels[v]`` the index into ``names`` (the dict's keys in order) of the LAST part that lists vertex ``v`` - 500 of SMPL's
    vertices are listed under two parts.  Raises ``IconAmdError`` if an index is out of range or a vertex is in no part."""
    if not isinstance(vert_segmentation, dict) or not vert_segmentation:
        raise IconAmdError(f"part_labels: vert_segmentation must be a non-empty dict of part name -> vertex indices, got {type(vert_segmentation).__name__}")
    n_verts = int(n_verts)
    names = [str(k) for k in vert_segmentation.keys()]
    labels = np.full(n_verts, -1, dtype=np.int32)
    for k, (name, val) in enumerate(vert_segmentation.items()):
        idx = np.asarray(val)
        if idx.size == 0:
            continue
        if idx.ndim != 1 or idx.dtype.kind not in "iu":
            raise IconAmdError(f"part_labels: part {name!r} must list integer vertex indices, got an array of {idx.dtype} with shape {list(idx.shape)}")
        if int(idx.min()) < 0 or int(idx.max()) >= n_verts:
            raise IconAmdError(f"part_labels: part {name!r} names vertex {int(idx.max()) if int(idx.max()) >= n_verts else int(idx.min())}, "
                               f"the mesh has {n_verts}")
        labels[idx] = k
    if (labels < 0).any():
        raise IconAmdError(f"part_labels: {int((labels < 0).sum())} vertices are in no part (the first: {int(np.argmax(labels < 0))})")
    return names, labels


def parts_to_remove(type_id) -> list:
    """the body parts ``extract_cloth`` removes for a DeepFashion2 category (cloth_extraction.py:117-133): hands, feet and head
    always; the forearms for short sleeves (1, 3, 10); forearms and arms for sleeveless tops and lower-body clothes (5, 6, 8, 9,
    12, 13); those and the lower legs for shorts (7)."""
    parts = list(_BASE_PARTS)
    if type_id in _SHORT_SLEEVES:
        parts += ["leftForeArm", "rightForeArm"]
    elif type_id in _NO_SLEEVES:
        parts += ["leftForeArm", "rightForeArm", "leftArm", "rightArm"]
    elif type_id in _SHORTS:
        parts += ["leftLeg", "rightLeg", "leftForeArm", "rightForeArm", "leftArm", "rightArm"]
    return parts


def polygons_to_model_plane(coord_normalized, K, R, t) -> list:
    """rule 1 (what cloth_extraction.py:89-108 computes): the segmentation's polygons, normalised image coordinates ``[n,2]`` each,
    taken back through the pseudo-inverse of the 3x4 projection ``K[:3,:3] [R | t]`` -> float64 ``[n,2]`` each.  The same numpy
    operations in the reference's order - ``np.linalg.pinv`` of the float64 product, one 4x3 by 3x1 ``matmul`` per vertex, a division by
    the fourth component - so the coordinates are the reference's to the bit (tests/test_garment.py).  Raises ``IconAmdError`` for a
    polygon that is not ``[n,2]`` or a coordinate that is not finite."""
    K, R, t = np.asarray(K, dtype=np.float64), np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)
    if K.ndim != 2 or K.shape[0] < 3 or K.shape[1] < 3 or R.shape != (3, 3) or t.size != 3:
        raise IconAmdError(f"polygons_to_model_plane: K must be at least [3,3], R [3,3] and t 3 values, got {list(K.shape)}, {list(R.shape)}, {list(t.shape)}")
    back = np.linalg.pinv(np.matmul(K[:3, :3], np.concatenate([R, t.reshape(3, 1)], axis=1)))       # [4,3]: image (x, y, 1) -> homogeneous model point
    out = []
    for k, polygon in enumerate(coord_normalized):
        polygon = np.asarray(polygon, dtype=np.float64)
        if polygon.ndim != 2 or polygon.shape[1] != 2:
            raise IconAmdError(f"polygons_to_model_plane: polygon {k} must be [n,2], got {list(polygon.shape)}")
        image = np.concatenate([polygon, np.ones((polygon.shape[0], 1))], axis=1)
        model = np.matmul(back, image[:, :, None])[:, :, 0]                        # a product per vertex, as the reference forms it
        xy = np.ascontiguousarray(model[:, :2] / model[:, 3:4])
        if not np.isfinite(xy).all():
            raise IconAmdError(f"polygons_to_model_plane: polygon {k} has a coordinate that is not finite in the model plane")
        out.append(xy)
    return out


def _pack_polygons(polygons, what: str):
    """list of [n,2] -> (xy float64 [total,2], off int32 [P+1]) on the host; refuses shapes and non-finite coordinates"""
    if isinstance(polygons, (np.ndarray, torch.Tensor)) and polygons.ndim == 2:
        polygons = [polygons]
    xs, off = [], [0]
    for k, p in enumerate(polygons):
        p = p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)
        if p.dtype.kind not in "fiu":
            raise IconAmdError(f"{what}: polygon {k} must hold numbers, got {p.dtype}")
        p = p.astype(np.float64, copy=False)
        if p.ndim != 2 or p.shape[1] != 2:
            raise IconAmdError(f"{what}: polygon {k} must be [n,2], got {list(p.shape)}")
        if not np.isfinite(p).all():
            raise IconAmdError(f"{what}: polygon {k} has a coordinate that is not finite")
        xs.append(p)
        off.append(off[-1] + p.shape[0])
    if off[-1] >= 2 ** 31:
        raise IconAmdError(f"{what}: {off[-1]} polygon vertices; the call takes fewer than 2^31")
    xy = np.ascontiguousarray(np.concatenate(xs, 0) if xs else np.zeros((0, 2)), dtype=np.float64)
    return xy, np.asarray(off, dtype=np.int32)


# ---- the device side ---------------------------------------------------------------------------------------------------------

def _check_points(t, name: str, what: str):
    if not torch.is_tensor(t):
        raise IconAmdError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if not t.dtype.is_floating_point:
        raise IconAmdError(f"{what}: {name} must be a floating-point tensor, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise IconAmdError(f"{what}: {name} must be [N,3], got {list(t.shape)}")


def _check_device(what: str, **tensors):
    need_device(what)
    devs = {n: t.device for n, t in tensors.items() if t is not None}
    first = next(iter(devs.values()))
    if any(not t.is_cuda for t in tensors.values() if t is not None) or any(d != first for d in devs.values()):
        raise IconAmdError(f"{what}: {', '.join(devs)} must live on one HIP device, got {', '.join(str(d) for d in devs.values())}")
    return first


def nearest_vertex_device(verts: torch.Tensor, src_verts: torch.Tensor, only: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``verts [V,3]``, ``src_verts [Vs,3]`` on one HIP device -> int32 ``[V]`` there: for each vertex the LOWEST index of the
    source vertex at the smallest float64 squared distance (rule 3; numpy's ``((q - s)**2).sum(-1).argmin()``).  ``only``: bool or
    uint8 ``[V]``; a vertex whose entry is 0 is skipped and gets -1.  One native launch (icon_nearest_vertex) on the current
    stream: nothing is allocated by it, nothing waited for."""
    what = "nearest_vertex_device"
    _check_points(verts, "verts", what)
    _check_points(src_verts, "src_verts", what)
    if src_verts.shape[0] == 0:
        raise IconAmdError(f"{what}: src_verts is empty")
    if only is not None:
        if not torch.is_tensor(only) or only.dtype not in (torch.bool, torch.uint8):
            raise IconAmdError(f"{what}: only must be a bool or uint8 tensor, got {only.dtype if torch.is_tensor(only) else type(only).__name__}")
        if only.dim() != 1 or only.shape[0] != verts.shape[0]:
            raise IconAmdError(f"{what}: only must be [{verts.shape[0]}], got {list(only.shape)}")
    dev = _check_device(what, verts=verts, src_verts=src_verts, only=only)
    v = verts.detach().to(torch.float32).contiguous()
    s = src_verts.detach().to(torch.float32).contiguous()
    o = None if only is None else only.detach().to(torch.uint8).contiguous()
    out = torch.empty(v.shape[0], dtype=torch.int32, device=dev)
    if v.shape[0] == 0:
        return out
    with torch.cuda.device(dev):
        check(_lib.lib().icon_nearest_vertex(_lib.ptr(v), C.c_int64(v.shape[0]), _lib.ptr(s), C.c_int64(s.shape[0]), _lib.ptr(o),
                                             _lib.ptr(out), stream()), "icon_nearest_vertex")
    return out


def transfer_labels_device(verts: torch.Tensor, src_verts: torch.Tensor, src_labels: torch.Tensor) -> torch.Tensor:
    """the classifier of ``smpl_to_recon_labels`` (cloth_extraction.py:62-65): ``src_labels [Vs]`` (any dtype) copied onto
    ``verts`` from each vertex's nearest source vertex -> ``[V]`` of that dtype, on the device: a gather of the native index."""
    if not torch.is_tensor(src_labels) or src_labels.dim() != 1 or not torch.is_tensor(src_verts) or src_labels.shape[0] != src_verts.shape[0]:
        raise IconAmdError(f"transfer_labels_device: src_labels must be a tensor [Vs] with one label per source vertex, got "
                           f"{list(src_labels.shape) if torch.is_tensor(src_labels) else type(src_labels).__name__}")
    nn = nearest_vertex_device(verts, src_verts)
    return src_labels.to(nn.device)[nn.long()]


def extract_cloth_device(verts: torch.Tensor, faces: torch.Tensor, polygons: Sequence, src_verts: Optional[torch.Tensor] = None,
                         src_remove: Optional[torch.Tensor] = None, return_index: bool = False):
    """rules 2 to 6 of DESIGN.md 4.19 as ONE native call (icon_extract_cloth) on the current stream, device tensors in and out.

    ``verts [V,3]`` floating point, ``faces [F,3]`` int32 or int64 (read in place; other integer types are widened) on one HIP
    device; ``polygons``: a list of ``[n,2]`` arrays in the model's xy plane (``polygons_to_model_plane``), taken in float64 on the
    host; ``src_verts [Vs,3]`` with ``src_remove [Vs]`` (bool / uint8: the source vertices whose nearest reconstruction vertices
    are dropped), or neither.  -> ``(verts' [V',3] float32, faces' [F',3] int32)`` - with ``return_index`` also ``vert_ids [V']``
    int32, the input index of every output vertex - or ``None`` when no face is kept.  A face that names a vertex that does
    not exist is never kept.  The call waits for the stream once, for the two counts; its scratch is cached per (thread, device,
    stream)."""
    what = "extract_cloth_device"
    _check_points(verts, "verts", what)
    if not torch.is_tensor(faces) or faces.dtype.is_floating_point or faces.dtype == torch.bool:
        raise IconAmdError(f"{what}: faces must be an integer tensor, got {faces.dtype if torch.is_tensor(faces) else type(faces).__name__}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise IconAmdError(f"{what}: faces must be [F,3], got {list(faces.shape)}")
    if src_remove is not None and src_verts is None:
        raise IconAmdError(f"{what}: src_remove given without src_verts")
    if src_verts is not None:
        _check_points(src_verts, "src_verts", what)
        if src_remove is None:
            raise IconAmdError(f"{what}: src_verts given without src_remove (the source vertices to drop)")
        if not torch.is_tensor(src_remove) or src_remove.dtype not in (torch.bool, torch.uint8):
            raise IconAmdError(f"{what}: src_remove must be a bool or uint8 tensor, got {src_remove.dtype if torch.is_tensor(src_remove) else type(src_remove).__name__}")
        if src_remove.dim() != 1 or src_remove.shape[0] != src_verts.shape[0] or src_verts.shape[0] == 0:
            raise IconAmdError(f"{what}: src_remove must be [Vs] for src_verts [Vs,3] with Vs > 0, got {list(src_remove.shape)} and {list(src_verts.shape)}")
    xy, off = _pack_polygons(polygons, what)
    dev = _check_device(what, verts=verts, faces=faces, src_verts=src_verts, src_remove=src_remove)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if V == 0 or F == 0:
        return None
    v = verts.detach().to(torch.float32).contiguous()
    f, f_i64 = faces_arg(faces)
    s = None if src_verts is None else src_verts.detach().to(torch.float32).contiguous()
    r = None if src_remove is None else src_remove.detach().to(torch.uint8).contiguous()
    L = _lib.lib()
    with torch.cuda.device(dev):
        d_xy = torch.from_numpy(xy).to(dev)
        d_off = torch.from_numpy(off).to(dev)
        scratch = scratch_for(dev, "icon_extract_cloth_bytes", C.c_int64(V), C.c_int64(F), C.c_int64(xy.shape[0]), C.c_int64(len(off) - 1))
        ov = torch.empty((V, 3), dtype=torch.float32, device=dev)
        of = torch.empty((F, 3), dtype=torch.int32, device=dev)
        ids = torch.empty(V, dtype=torch.int32, device=dev)
        hc = (C.c_int64 * 2)()
        check(L.icon_extract_cloth(_lib.ptr(v), C.c_int64(V), _lib.ptr(f), C.c_int64(F), f_i64,
                                   _lib.ptr(d_xy), _lib.ptr(d_off), C.c_int64(xy.shape[0]), C.c_int64(len(off) - 1),
                                   _lib.ptr(s), C.c_int64(0 if s is None else s.shape[0]), _lib.ptr(r),
                                   _lib.ptr(ov), _lib.ptr(of), _lib.ptr(ids), hc, _lib.ptr(scratch), C.c_int64(scratch.numel()), stream()),
              "icon_extract_cloth")
    nv, nf = int(hc[0]), int(hc[1])
    if nf == 0:
        return None
    return (ov[:nv], of[:nf], ids[:nv]) if return_index else (ov[:nv], of[:nf])


# ---- the reference's entry point -----------------------------------------------------------------------------------------------

class Garment:
    """what ``apps/infer.py:586-602`` uses of the mesh ``extract_cloth`` returns: ``vertices [V',3]`` float32, ``faces [F',3]``
    int32 and ``export(path)``; ``vert_ids [V']`` int32 - the index each vertex had in the reconstruction - lets a caller carry
    vertex colours over, which the reference drops.  numpy arrays on the host."""

    def __init__(self, vertices: np.ndarray, faces: np.ndarray, vert_ids: np.ndarray):
        self.vertices, self.faces, self.vert_ids = vertices, faces, vert_ids

    def export(self, path) -> None:
        """Wavefront OBJ: ``v x y z`` and ``f i j k`` lines; nine significant digits, which give every float32 back"""
        with open(path, "w") as fh:
            fh.writelines(f"v {x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in self.vertices.tolist())
            fh.writelines(f"f {i} {j} {k}\n" for i, j, k in (self.faces + 1).tolist())


def _mesh_of(obj, name: str):
    if hasattr(obj, "vertices") and hasattr(obj, "faces"):
        v, f = obj.vertices, obj.faces
    elif isinstance(obj, (tuple, list)) and len(obj) == 2:
        v, f = obj
    else:
        raise IconAmdError(f"extract_cloth: {name} must have .vertices and .faces or be a (verts, faces) pair, got {type(obj).__name__}")
    v = v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(np.asarray(v)))
    f = f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(np.asarray(f)))
    return v, f


def extract_cloth(recon, segmentation: dict, K, R, t, smpl=None, vert_segmentation=None):
    """Drop-in for ``lib.common.cloth_extraction.extract_cloth`` (called at apps/infer.py:586): ``recon`` / ``smpl`` - anything with
    ``.vertices`` and ``.faces``, or ``(verts, faces)`` pairs, host or device tensors or arrays; ``segmentation`` - the reference's
    dict (``coord_normalized``: the polygons, ``type_id``: the DeepFashion2 category); ``K``, ``R``, ``t`` as the reference takes
    them.  ``vert_segmentation``: the dict read from the reference's ``smpl_vert_segmentation.json``, or a ``(names, labels)`` pair
    as ``part_labels`` returns it - required when ``smpl`` is given.  ``smpl=None`` (where the reference dies on an unbound name):
    the polygons alone decide.  -> a ``Garment`` (``.vertices``, ``.faces``, ``.vert_ids``, ``.export(path)``) or ``None`` when no
    face is kept.  Runs on the HIP device the reconstruction lives on, else on the current one."""
    if not isinstance(segmentation, dict) or "coord_normalized" not in segmentation:
        raise IconAmdError("extract_cloth: segmentation must be a dict with 'coord_normalized' (and 'type_id' when smpl is given)")
    verts, faces = _mesh_of(recon, "recon")
    what = "extract_cloth"
    _check_points(verts, "recon vertices", what)
    if faces.dtype.is_floating_point or faces.dtype == torch.bool or faces.dim() != 2 or faces.shape[1] != 3:
        raise IconAmdError(f"{what}: recon faces must be an integer [F,3], got {faces.dtype} {list(faces.shape)}")
    polygons = polygons_to_model_plane(segmentation["coord_normalized"], K, R, t)
    src = remove = None
    if smpl is not None:
        src, _ = _mesh_of(smpl, "smpl")
        _check_points(src, "smpl vertices", what)
        if vert_segmentation is None:
            raise IconAmdError(f"{what}: smpl given without vert_segmentation (the dict of the reference's smpl_vert_segmentation.json, "
                               "or a (names, labels) pair); the library ships no copy of that file")
        if "type_id" not in segmentation:
            raise IconAmdError(f"{what}: segmentation has no 'type_id'")
        if isinstance(vert_segmentation, dict):
            names, labels = part_labels(vert_segmentation, src.shape[0])
        else:
            names, labels = vert_segmentation
            names, labels = [str(n) for n in names], np.asarray(labels)
            if labels.shape != (src.shape[0],) or labels.dtype.kind not in "iu" or (labels.size and (labels.min() < 0 or labels.max() >= len(names))):
                raise IconAmdError(f"{what}: labels must be [{src.shape[0]}] integers below {len(names)}, got {labels.dtype} {list(labels.shape)}")
        wanted = parts_to_remove(segmentation["type_id"])
        missing = [p for p in wanted if p not in names]
        if missing:
            raise IconAmdError(f"{what}: the part table has no {missing}")
        remove = torch.from_numpy(np.isin(labels, [names.index(p) for p in wanted]))
    if not faces.is_cuda and faces.numel() and (int(faces.min()) < 0 or int(faces.max()) >= verts.shape[0]):   # host data: no device involved
        raise IconAmdError(f"{what}: face index out of range")
    need_device(what)
    dev = verts.device if verts.is_cuda else torch.device("cuda", torch.cuda.current_device())
    f = faces.detach()
    f = f.to(dev) if f.dtype in (torch.int32, torch.int64) else f.to(dev, torch.int64)
    with torch.cuda.device(dev):
        out = extract_cloth_device(verts.detach().to(dev, torch.float32), f, polygons,
                                   None if src is None else src.detach().to(dev, torch.float32),
                                   None if remove is None else remove.to(dev), return_index=True)
    if out is None:
        return None
    return Garment(*(x.cpu().numpy() for x in out))

"""The cloth refinement step of ``apps/infer.py:405-476`` on the device, without pytorch3d.

Replaces, per iteration of that loop, ``LocalAffine`` (``lib/net/local_affine.py``: the deformation ``y = A x + b`` and the
stiffness / rigidity terms) and ``update_mesh_shape_prior_losses`` (``lib/dataset/mesh_util.py:168-176``: ``mesh_edge_loss``,
pytorch3d's ``mesh_normal_consistency`` and ``mesh_laplacian_smoothing(method="uniform")``) by two ``torch.autograd.Function``s
over four native calls (csrc/cloth.hip; the rule is DESIGN.md 4.16, parity unpinned like 4.13-4.15).  The mesh topology those
calls read - pytorch3d's ``edges_packed`` order, neighbour rows, face pairs - is built ONCE per mesh by ``ClothTopology``, from
torch operators on whatever device the faces live on; the native calls need a HIP device and there is no CPU path for them.

Differences from the reference, on purpose:

* ``LocalAffine.forward(x, return_stiff=True)`` returns the MEANS of the stiffness and rigidity terms (0-dim tensors) where
  the reference returns the ``[B,E,3,4]`` / ``[B,V]`` tensors: the loop only ever takes ``torch.mean`` of them
  (``apps/infer.py:457-458``), which is the identity on a 0-dim tensor, so the call site needs no change - and the stiffness
  tensor and its gradient are never materialised.
* ``x`` is a constant: a ``x`` that requires grad is refused, not silently given no gradient.
* The priors take ONE mesh (``[V,3]`` or ``[1,V,3]``); ``method="cot"`` / ``"cotcurv"`` are refused.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import IconAmdError, check
from ._native import need_device, scratch_for, stream

TERMS = {"edge": 1, "nc": 2, "laplacian": 4}                              # include/icon_amd.h: ICON_PRIOR_*


def _index_tensor(what: str, t, cols: int) -> torch.Tensor:
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if t.dim() == 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 2 or t.shape[1] != cols:
        raise IconAmdError(f"ClothTopology: {what} must be a [N,{cols}] tensor, got {tuple(t.shape)}")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise IconAmdError(f"ClothTopology: {what} must be an integer tensor, got {t.dtype}")
    return t.detach().to(torch.int64)


def _csr(rows: torch.Tensor, vals: torch.Tensor, n_rows: int, span: int):
    """entries ``vals`` (each in ``0..span-1``) grouped by ``rows``, ascending within a row, duplicates kept -> (offsets [n_rows+1], values)"""
    order = torch.argsort(rows * span + vals)
    off = torch.zeros(n_rows + 1, dtype=torch.int64, device=rows.device)
    off[1:] = torch.cumsum(torch.bincount(rows, minlength=n_rows), 0)
    return off, vals[order].contiguous()


class ClothTopology:
    """What the native cloth calls read of a mesh, built once (plumbing: torch operators, one synchronisation to validate).

    ``ClothTopology(faces, num_verts=V)``: ``faces [F,3]`` (or ``[1,F,3]``) integer, on any device.  ``ClothTopology(
    num_verts=V, edges=edges)``: from an edge list ``[E,2]`` alone - kept as given, duplicates included (a duplicated edge
    counts as often as it is listed); only what ``LocalAffine`` needs exists then (``has_faces`` is False).  An index outside
    ``0..V-1`` raises ``IconAmdError``.

    * ``edges [E,2]``: with faces, pytorch3d's ``edges_packed()`` - the unique ``(min, max)`` pairs in ascending ``min V + max``.
    * ``nbr_off [V+1]``, ``nbr [2E]``: row ``v`` lists the other end of every edge at ``v``, ascending, multiplicity kept (an
      edge ``(v, v)`` puts ``v`` into its own row twice, as it weighs in pytorch3d's Laplacian).
    * ``pairs [P,4] = (v0, v1, a, c)``: every unordered pair of face corners lying opposite one edge ``(v0 < v1)``, with their
      third vertices; edge by edge in the order of ``edges``, within an edge in the combination order ((0,1), (0,2), (1,2), ...)
      of the corners' positions ``3 f + k`` in the face list.  An edge of ``k`` faces gives ``k (k - 1) / 2`` pairs.
    * ``inc_off [V+1]``, ``inc [4P]``: row ``v`` lists ``pair * 4 + slot`` for every slot of ``pairs`` that holds ``v``, ascending.

    All int64; ``to(device=..., index_dtype=torch.int32)`` gives a copy the native calls read just the same."""

    _FIELDS = ("edges", "nbr_off", "nbr", "pairs", "inc_off", "inc")

    def __init__(self, faces=None, num_verts: Optional[int] = None, edges=None):
        if num_verts is None or int(num_verts) != num_verts or int(num_verts) < 1:
            raise IconAmdError(f"ClothTopology: num_verts must be a positive integer, got {num_verts}")
        if (faces is None) == (edges is None):
            raise IconAmdError("ClothTopology: give either faces or edges")
        V = self.num_verts = int(num_verts)
        self.pairs = self.inc_off = self.inc = None
        src = _index_tensor("faces", faces, 3) if faces is not None else _index_tensor("edges", edges, 2)
        if src.numel() and (int(src.min()) < 0 or int(src.max()) >= V):      # the one synchronisation
            raise IconAmdError(f"ClothTopology: an index lies outside 0..{V - 1}")
        if faces is None:
            self.edges = src.contiguous()
        else:
            f = src
            F = f.shape[0]
            # corner k of face f lies opposite the edge (f[k+1], f[k+2]); its position in the face list is 3 f + k
            e0 = torch.stack([f[:, 1], f[:, 2], f[:, 0]], 1).reshape(-1)
            e1 = torch.stack([f[:, 2], f[:, 0], f[:, 1]], 1).reshape(-1)
            third = f.reshape(-1)
            key = torch.minimum(e0, e1) * V + torch.maximum(e0, e1)
            ukey, inv = torch.unique(key, sorted=True, return_inverse=True)
            self.edges = torch.stack([ukey // V, ukey % V], 1).contiguous()
            order = torch.argsort(inv * (3 * F) + torch.arange(3 * F, device=f.device))    # by edge, then by position
            eid, oth = inv[order], third[order]
            count = torch.bincount(eid, minlength=ukey.shape[0])
            start = torch.cumsum(count, 0) - count
            n = eid.shape[0]
            rank = torch.arange(n, device=f.device) - start[eid]
            later = count[eid] - 1 - rank                                   # corners of the same edge behind this one
            first = torch.repeat_interleave(torch.arange(n, device=f.device), later)
            begin = torch.cumsum(later, 0) - later
            second = first + 1 + (torch.arange(first.shape[0], device=f.device) - begin[first])
            pe = self.edges[eid[first]]
            self.pairs = torch.stack([pe[:, 0], pe[:, 1], oth[first], oth[second]], 1).contiguous()
            P = self.pairs.shape[0]
            self.inc_off, self.inc = _csr(self.pairs.reshape(-1), torch.arange(4 * P, device=f.device), V, max(4 * P, 1))
        a, b = self.edges[:, 0], self.edges[:, 1]
        self.nbr_off, self.nbr = _csr(torch.cat([a, b]), torch.cat([b, a]), V, V)

    @property
    def has_faces(self) -> bool:
        return self.pairs is not None

    @property
    def num_edges(self) -> int:
        return int(self.edges.shape[0])

    @property
    def num_pairs(self) -> int:
        return int(self.pairs.shape[0]) if self.pairs is not None else 0

    @property
    def device(self) -> torch.device:
        return self.edges.device

    @property
    def index_dtype(self) -> torch.dtype:
        return self.edges.dtype

    def to(self, device=None, index_dtype=None) -> "ClothTopology":
        if index_dtype not in (None, torch.int32, torch.int64):
            raise IconAmdError(f"ClothTopology: index_dtype must be torch.int32 or torch.int64, got {index_dtype}")
        if index_dtype == torch.int32 and max(2 * self.num_edges, 4 * self.num_pairs, self.num_verts) >= 2 ** 31:
            raise IconAmdError("ClothTopology: this mesh does not fit int32 indices")
        out = object.__new__(ClothTopology)
        out.num_verts = self.num_verts
        for name in self._FIELDS:
            t = getattr(self, name)
            setattr(out, name, None if t is None else t.to(device=device if device is not None else t.device,
                                                            dtype=index_dtype if index_dtype is not None else t.dtype).contiguous())
        return out


def _on_device(what: str, topo: ClothTopology, *tensors) -> None:
    need_device(what)
    dev = tensors[0].device
    if not all(t.is_cuda and t.device == dev for t in tensors) or topo.device != dev:
        raise IconAmdError(f"{what}: the tensors and the topology must live on one HIP device (ClothTopology.to(device) moves it)")


def _i64(topo: ClothTopology) -> C.c_int:
    return C.c_int(1 if topo.index_dtype == torch.int64 else 0)


class _LocalAffineFn(torch.autograd.Function):
    """(x, A, b) float32, contiguous, on the device -> y, stiffness mean, rigidity mean; differentiable in A and b"""

    @staticmethod
    def forward(ctx, x, A, b, topo):
        B, V, E = x.shape[0], x.shape[1], topo.num_edges
        L = _lib.lib()
        with torch.cuda.device(x.device):
            scratch = scratch_for(x.device, "icon_local_affine_bytes", C.c_int64(B), C.c_int64(V), C.c_int64(E))
            y = torch.empty_like(x)
            stiff = torch.empty((), dtype=torch.float32, device=x.device)
            rigid = torch.empty((), dtype=torch.float32, device=x.device)
            check(L.icon_local_affine_forward(_lib.ptr(x), _lib.ptr(A), _lib.ptr(b), C.c_int64(B), C.c_int64(V), _lib.ptr(topo.edges),
                                              C.c_int64(E), _i64(topo), _lib.ptr(y), _lib.ptr(stiff), _lib.ptr(rigid),
                                              _lib.ptr(scratch), C.c_int64(scratch.numel()), stream()), "icon_local_affine_forward")
        ctx.save_for_backward(x, A, b)
        ctx.topo = topo
        return y, stiff, rigid

    @staticmethod
    def backward(ctx, gy, gs, gr):
        x, A, b = ctx.saved_tensors
        topo = ctx.topo
        B, V, E = x.shape[0], x.shape[1], topo.num_edges
        gy, gs, gr = (g.to(torch.float32).contiguous() for g in (gy, gs, gr))
        L = _lib.lib()
        with torch.cuda.device(x.device):
            gA, gb = torch.empty_like(A), torch.empty_like(b)
            check(L.icon_local_affine_backward(_lib.ptr(x), _lib.ptr(A), _lib.ptr(b), C.c_int64(B), C.c_int64(V), _lib.ptr(topo.nbr_off),
                                               _lib.ptr(topo.nbr), C.c_int64(E), _i64(topo), _lib.ptr(gy), _lib.ptr(gs), _lib.ptr(gr),
                                               _lib.ptr(gA), _lib.ptr(gb), stream()), "icon_local_affine_backward")
        return None, gA, gb, None


def local_affine_device(x: torch.Tensor, A: torch.Tensor, b: torch.Tensor, topo: ClothTopology):
    """``x [B,V,3]``, ``A [B,V,3,3]``, ``b [B,V,3,1]`` (float) and ``topo`` on one HIP device -> ``(y [B,V,3], stiffness, rigid)``:
    ``y_i = A_i x_i + b_i``; ``stiffness`` the mean over (B, E, 3, 4) of ``([A_i | b_i] - [A_j | b_j])^2`` over ``topo.edges``;
    ``rigid`` the mean over (B, V) of ``(det A_i - 1)^2`` - both 0-dim float32 tensors.  Differentiable in ``A`` and ``b``
    (the gradient flows back through a float32 cast); ``x`` is a constant and must not require grad.  Each direction is one
    native call on the current stream (two launches forward, one backward): nothing allocated by it, nothing read back, no
    floating-point atomics - equal bytes from run to run and from int32 and int64 topologies."""
    what = "local_affine_device"
    if not isinstance(topo, ClothTopology):
        raise IconAmdError(f"{what}: topo must be a ClothTopology")
    if not all(torch.is_tensor(t) and t.dtype.is_floating_point for t in (x, A, b)):
        raise IconAmdError(f"{what}: x, A and b must be floating-point tensors")
    if x.dim() != 3 or x.shape[2] != 3 or x.shape[0] < 1 or x.shape[1] != topo.num_verts:
        raise IconAmdError(f"{what}: x must be [B,{topo.num_verts},3], got {tuple(x.shape)}")
    B, V = x.shape[0], x.shape[1]
    if tuple(A.shape) != (B, V, 3, 3) or tuple(b.shape) != (B, V, 3, 1):
        raise IconAmdError(f"{what}: A must be [{B},{V},3,3] and b [{B},{V},3,1] for x {tuple(x.shape)} (B and V must agree), "
                           f"got {tuple(A.shape)} and {tuple(b.shape)}")
    if x.requires_grad:
        raise IconAmdError(f"{what}: x is a constant of the cloth loop and gets no gradient - pass x.detach()")
    _on_device(what, topo, x, A, b)
    return _LocalAffineFn.apply(x.to(torch.float32).contiguous(), A.to(torch.float32).contiguous(), b.to(torch.float32).contiguous(), topo)


class LocalAffine(torch.nn.Module):
    """Drop-in for ``lib.net.local_affine.LocalAffine``: the same constructor ``(num_points, batch_size=1, edges=None)``, the
    same parameters (``A [B,V,3,3]`` = identity, ``b [B,V,3,1]`` = 0; ``state_dict``s interchange), ``forward(x, return_stiff)``.

    With ``return_stiff=True`` it returns ``(y, stiffness, rigid)`` with the two MEANS (0-dim) where the reference returns the
    ``[B,E,3,4]`` and ``[B,V]`` tensors - ``torch.mean`` of them (``apps/infer.py:457-458``) is the identity, so the loop runs
    unchanged.  ``edges``: the ``[E,2]`` list (``ClothTopology(faces, V).edges`` is pytorch3d's ``edges_packed()``) or a
    ``ClothTopology``, whose lists are then shared and not built again; without edges ``return_stiff=True`` raises
    (``IconAmdError``; the reference raises a plain ``Exception`` there)."""

    def __init__(self, num_points, batch_size=1, edges=None):
        super().__init__()
        B, V = int(batch_size), int(num_points)
        self.A = torch.nn.Parameter(torch.eye(3).expand(B, V, 3, 3).clone())        # identity per (mesh, vertex)
        self.b = torch.nn.Parameter(torch.zeros(B, V, 3, 1))
        self.num_points = V
        if isinstance(edges, ClothTopology):
            if edges.num_verts != num_points:
                raise IconAmdError(f"LocalAffine: the topology has {edges.num_verts} vertices, num_points is {num_points}")
            self.edges, self.topo = edges.edges, edges
        else:
            self.edges = edges
            self.topo = ClothTopology(num_verts=num_points, edges=edges) if edges is not None else None
        self._bare = None

    def _topology(self, device: torch.device) -> ClothTopology:
        if self.topo is None:                                              # no edges: the deformation alone
            if self._bare is None or self._bare.device != device:
                self._bare = ClothTopology(num_verts=self.num_points, edges=torch.zeros((0, 2), dtype=torch.int64, device=device))
            return self._bare
        if self.topo.device != device:
            self.topo = self.topo.to(device)
        return self.topo

    def forward(self, x, return_stiff=False):
        if return_stiff and self.edges is None:
            raise IconAmdError("LocalAffine: return_stiff=True needs the edges the model was built without")
        need_device("LocalAffine")
        y, stiffness, rigid = local_affine_device(x, self.A, self.b, self._topology(self.A.device))
        return (y, stiffness, rigid) if return_stiff else y


def _mp_args(v, topo, target_length, mask):
    E, P = topo.num_edges, topo.num_pairs
    return (_lib.ptr(v), C.c_int64(v.shape[0]), _lib.ptr(topo.edges), _lib.ptr(topo.nbr_off), _lib.ptr(topo.nbr), C.c_int64(E)), \
           (C.c_int64(P), _i64(topo), C.c_float(target_length), C.c_int(mask))


def _mp_scratch(v, topo):
    return scratch_for(v.device, "icon_mesh_priors_bytes", C.c_int64(v.shape[0]), C.c_int64(topo.num_edges), C.c_int64(topo.num_pairs))


class _MeshPriorsFn(torch.autograd.Function):
    """verts (float32, contiguous, on the device) -> edge, nc, laplacian (0-dim); the other arguments are not differentiable"""

    @staticmethod
    def forward(ctx, v, topo, target_length, mask):
        head, tail = _mp_args(v, topo, target_length, mask)
        with torch.cuda.device(v.device):
            scratch = _mp_scratch(v, topo)
            out = [torch.empty((), dtype=torch.float32, device=v.device) for _ in range(3)]
            check(_lib.lib().icon_mesh_priors_forward(*head, _lib.ptr(topo.pairs), *tail, *(_lib.ptr(o) for o in out),
                                                      _lib.ptr(scratch), C.c_int64(scratch.numel()), stream()), "icon_mesh_priors_forward")
        ctx.save_for_backward(v)
        ctx.topo, ctx.target_length, ctx.mask = topo, target_length, mask
        return tuple(out)

    @staticmethod
    def backward(ctx, g_edge, g_nc, g_lap):
        v, = ctx.saved_tensors
        topo = ctx.topo
        head, tail = _mp_args(v, topo, ctx.target_length, ctx.mask)
        g = [t.to(torch.float32).contiguous() for t in (g_edge, g_nc, g_lap)]
        with torch.cuda.device(v.device):
            scratch = _mp_scratch(v, topo)                                   # this thread's and this stream's: autograd has its own
            grad = torch.empty_like(v)
            check(_lib.lib().icon_mesh_priors_backward(*head, _lib.ptr(topo.pairs), _lib.ptr(topo.inc_off), _lib.ptr(topo.inc), *tail,
                                                       *(_lib.ptr(t) for t in g), _lib.ptr(grad), _lib.ptr(scratch), C.c_int64(scratch.numel()),
                                                       stream()), "icon_mesh_priors_backward")
        return grad, None, None, None


def mesh_shape_prior_losses_device(verts: torch.Tensor, topo: ClothTopology, target_length: float = 0.0,
                                   terms: Sequence[str] = ("edge", "nc", "laplacian"), method: str = "uniform"):
    """``verts [V,3]`` or ``[1,V,3]`` (float) and ``topo`` (built from faces) on one HIP device -> ``(edge, nc, laplacian)``,
    0-dim float32 tensors, differentiable in ``verts``: ``mesh_edge_loss(target_length)``, pytorch3d's
    ``mesh_normal_consistency`` and ``mesh_laplacian_smoothing(method="uniform")`` of that one mesh.  A term
    that ``terms`` leaves out is not computed: it comes back as a zero that carries no gradient (``apps/infer.py`` weights
    ``edge`` and ``nc`` by 0).  Each direction is one native call of two launches on the current stream: nothing allocated by
    it, nothing read back, no floating-point atomics - equal bytes from run to run and from int32 and int64 topologies."""
    what = "mesh_shape_prior_losses_device"
    if method != "uniform":
        raise IconAmdError(f"{what}: only method='uniform' is built, got {method!r} (cot and cotcurv are not)")
    if not isinstance(topo, ClothTopology) or not topo.has_faces:
        raise IconAmdError(f"{what}: topo must be a ClothTopology built from faces")
    names = list(terms)
    if not names or any(t not in TERMS for t in names):
        raise IconAmdError(f"{what}: terms must be a non-empty subset of {tuple(TERMS)}, got {tuple(terms)}")
    if not torch.is_tensor(verts) or not verts.dtype.is_floating_point:
        raise IconAmdError(f"{what}: verts must be a floating-point tensor")
    if verts.dim() == 3 and verts.shape[0] != 1:
        raise IconAmdError(f"{what}: the priors take one mesh, got a batch of {verts.shape[0]} (B > 1 is not built)")
    v = verts[0] if verts.dim() == 3 else verts
    if v.dim() != 2 or tuple(v.shape) != (topo.num_verts, 3):
        raise IconAmdError(f"{what}: verts must be [{topo.num_verts},3] or [1,{topo.num_verts},3], got {tuple(verts.shape)}")
    _on_device(what, topo, v)
    mask = sum(TERMS[t] for t in set(names))
    out = _MeshPriorsFn.apply(v.to(torch.float32).contiguous(), topo, float(target_length), mask)
    return tuple(o if mask & TERMS[name] else torch.zeros((), dtype=torch.float32, device=v.device)
                 for o, name in zip(out, ("edge", "nc", "laplacian")))


def update_mesh_shape_prior_losses(verts: torch.Tensor, topo_or_faces, losses: dict, terms: Optional[Sequence[str]] = None) -> None:
    """The reference's ``update_mesh_shape_prior_losses(mesh, losses)`` with the mesh given as its (deformed) vertices and a
    ``ClothTopology`` - or the faces, from which a topology is built on EVERY call (build it once outside a loop).  Writes
    ``losses["edge" | "nc" | "laplacian"]["value"]``; ``terms`` (default: all three) as in ``mesh_shape_prior_losses_device``."""
    topo = topo_or_faces
    if not isinstance(topo, ClothTopology):
        v = verts[0] if torch.is_tensor(verts) and verts.dim() == 3 else verts
        topo = ClothTopology(topo_or_faces, num_verts=v.shape[0]).to(v.device)
    edge, nc, lap = mesh_shape_prior_losses_device(verts, topo, terms=terms if terms is not None else tuple(TERMS))
    losses["edge"]["value"], losses["nc"]["value"], losses["laplacian"]["value"] = edge, nc, lap

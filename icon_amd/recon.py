"""Dense grid driver: the ``reconEngine`` object of the reference, re-designed for MI355X.

The reference's ``Seg3dLossless`` (lib/common/seg3d_lossless.py:36, built at apps/ICON.py:78-90)
evaluates the occupancy network coarse-to-fine on ~1 % of the lattice and trilinearly
interpolates the last level (SURVEY.md §0 finding 1).  ``DenseReconEngine`` keeps its call
contract - ``reconEngine(opt=cfg, netG=netG, features=features, proj_matrix=None)`` ->
``Tensor[D,H,W]`` (z,y,x) or ``None``, ``export_mesh(occ)``, ``resolutions`` / ``b_min`` / ``b_max``
buffers, an ``nn.Module`` - but evaluates EVERY lattice point of the finest resolution on the GPU,
which is exactly what ``Seg3dLossless`` computes when ``resolutions == [R]`` (one query() call over the
whole lattice, seg3d_lossless.py:166-171).

Multi-GPU: the volume is sharded by Z-slab over the ranks of a ``torch.distributed`` process group
(backend "nccl" == RCCL on ROCm); one ``all_gather`` of equal padded slabs assembles the volume
on every rank.  In ``cmap_mode="reference"`` the reference's tiled outlier-cmap assignment
(lib/net/HGPIFuNet.py:303-305) couples all points of the call, so the ranks first exchange their
outlier sign lists (one small ``all_gather``); ``cmap_mode="local"`` needs no exchange.
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import IconAmdError, check
from ._native import faces_arg, need_device, scratch_for, stream


def slab_partition(res: int, world_size: int, weights=None):
    """Contiguous Z-slabs [(z0, z1)] * world_size of near-equal COST.  ``weights`` [res] is the relative cost of
    every plane (default: uniform -> slab sizes differ by at most one plane: 257 / 8 = 33 + 7 x 32, instead of
    the 7 x 33 + 26 of a ceil-division split whose short tail idles).  Deterministic in its inputs, so every
    rank derives the same cut from the same (replicated) mesh."""
    w = np.ones(res, np.float64) if weights is None else np.asarray(weights, np.float64).reshape(res)
    if not (w > 0).all():
        raise IconAmdError("slab_partition: plane weights must be positive")
    cum = np.concatenate([[0.0], np.cumsum(w)])
    total = cum[-1]
    cuts = [0]
    for r in range(1, world_size):
        target = total * r / world_size
        z = int(np.searchsorted(cum, target, side="left"))
        if z > 0 and abs(cum[z - 1] - target) <= abs(cum[z] - target):   # nearest plane boundary to the ideal cut
            z -= 1
        cuts.append(min(max(z, cuts[-1]), res))
    cuts.append(res)
    return [(cuts[r], cuts[r + 1]) for r in range(world_size)]


def slab_bounds(res: int, world_size: int, rank: int, weights=None):
    """Planes [z0, z1) of rank ``rank`` and the largest slab size of the partition (the padded length every
    rank contributes to the all_gather)."""
    parts = slab_partition(res, world_size, weights)
    z0, z1 = parts[rank]
    return z0, z1, max(b - a for a, b in parts)


def sign_message_bytes(points: int) -> int:
    """Bytes of a rank's message of the sign exchange for a slab of ``points`` lattice points:
    [int64 count][2 bits per outlier sign, four to a byte], padded to a multiple of 8 (the int64 headers of the
    gathered buffer stay aligned)."""
    return 8 + ((points + 3) // 4 + 7) // 8 * 8


def plane_weights(res: int, z_lo: float, z_hi: float, far_cost: float = 1.04) -> np.ndarray:
    """Relative cost of the lattice planes for a body whose vertices span [z_lo, z_hi] in world z: planes farther
    than the clip band from the body are pure far-field, where the exact nearest-triangle search visits more
    candidates; the MLP cost per point is uniform.  Measured on MI355X (tools/time_slab.py, equal 32-plane slabs of
    the 257^3 lattice, 8 ranks): 2.47 / 2.42 / 2.36 / 2.33 | 2.33 / 2.37 / 2.38 ms from the outside in - a far-field
    plane costs ~4 % more than one through the body (it was ~10 % before the round-2 work on the search)."""
    z = -1.0 + 2.0 * np.arange(res) / (res - 1)
    near = (z >= z_lo - 0.1) & (z <= z_hi + 0.1)
    return np.where(near, 1.0, far_cost)


def lattice_coords(res, b_min, b_max, align_corners: bool, device) -> torch.Tensor:
    """[1, W*H*D, 3] world coordinates in z,y,x-major order: create_grid3D
    (lib/common/seg3d_utils.py:122-136) followed by the mapping of batch_eval
    (lib/common/seg3d_lossless.py:125-137), evaluated with the same float32 torch ops.
    ``res``: an int (cubic lattice) or the reference's (W, H, D) triple (seg3d_lossless.py:66-71)."""
    W, H, D = (int(res),) * 3 if isinstance(res, (int, np.integer)) else (int(r) for r in res)
    ax, ay, az = (torch.linspace(0, n - 1, n, device=device).long() for n in (W, H, D))
    gd, gh, gw = torch.meshgrid([az, ay, ax], indexing="ij")
    coords = torch.stack([gw, gh, gd]).view(3, -1).t().unsqueeze(0)  # (x,y,z), x fastest
    rr = torch.tensor([W, H, D], device=device)
    if align_corners:
        c = coords.float() / (rr - 1)
    else:
        c = coords.float() / rr + (1.0 / rr.float()) / 2
    return c * (b_max - b_min) + b_min


class DenseReconEngine(nn.Module):
    """Signature-compatible with ``Seg3dLossless.__init__`` (lib/common/seg3d_lossless.py:37-51);
    the adaptive-only knobs (``faster``, ``use_cuda_impl``, ``use_shadow``, ``visualize``, ``debug``)
    are accepted and ignored (every lattice point is evaluated: there is no schedule to choose; ``AdaptiveReconEngine``
    refuses ``faster=False``).  Extra keyword arguments:

    engine        an ``IconQueryEngine`` (otherwise one is attached to ``netG`` on first call)
    process_group torch.distributed group to shard over (default: WORLD if initialised)
    shard         False -> every rank evaluates the whole lattice (replicas, no collectives)
    balance_slabs cost-weighted Z-slab cut (far-field planes count 1.1; see plane_weights); False -> equal plane counts
    overlap_gather  the volume all_gather in two halves, the first overlapping the second half of the slab's MLP kernel
    reserve_cus   sharded only: the persistent MLP kernel (one workgroup per CU, the whole CU) leaves this many CUs free so
                  that RCCL's kernels can run beside it (the overlap is otherwise a hope: they cannot co-reside on a CU);
                  costs reserve_cus / CUs of the MLP time (bench.py: config.reserve_cus_cost: 16 of 256 CUs = 0.7 % of a step).
                  None (default) = 16 when the volume gather overlaps the MLP kernel over a device backend (nccl = RCCL), else 0
    slab_layout   "ab" (default): with the overlapped gather every rank owns TWO Z-slabs - A_r in the lower part of the volume and
                  B_r in the upper part (lattice order: A_0 .. A_{w-1}, B_0 .. B_{w-1}) - so that each of the two volume
                  gathers lands in ONE contiguous block of the result: no assembly copies (round 5 cut one contiguous slab per
                  rank in halves: the gathered halves interleave and had to be copied into place - up to two 68 MB device
                  copies per 257^3 volume).  "contiguous": the round-5 layout (one slab per rank, cost-weighted cut); it is
                  also what runs without the overlapped gather, for the mesh exchange and for backends without a second workspace
    gather_to     None (default): every rank receives the volume (all_gather).  A rank number: only that rank does (gather) -
                  forward() returns the volume (or None when empty) THERE and None on every other rank; the marching-cubes
                  consumer is one process, and 7/8 of an all_gather's receive traffic serves nobody
    backend       object providing eval_slab / slab_features / slab_finish (tests inject a CPU
                  checker here; the default is the HIP engine)
    """

    def __init__(self, query_func=None, b_min=((-1.0, 1.0, -1.0),), b_max=((1.0, -1.0, 1.0),), resolutions=(257,),
                 channels=1, balance_value=0.5, align_corners=False, visualize=False, debug=False,
                 use_cuda_impl=False, faster=False, use_shadow=False, engine=None, process_group=None,
                 shard=True, backend=None, balance_slabs=True, overlap_gather=True, reserve_cus=None, slab_layout="ab", gather_to=None,
                 **kwargs):
        super().__init__()
        self.query_func = query_func
        self.register_buffer("b_min", torch.tensor(b_min).float().unsqueeze(1))   # [1,1,3]
        self.register_buffer("b_max", torch.tensor(b_max).float().unsqueeze(1))
        resolutions = list(resolutions)
        if type(resolutions[0]) is int or isinstance(resolutions[0], (np.integer,)):
            res_t = torch.tensor([(int(r), int(r), int(r)) for r in resolutions])
        else:
            res_t = torch.tensor(resolutions)
        self.register_buffer("resolutions", res_t)
        self.batchsize = self.b_min.size(0)
        assert self.batchsize == 1
        self.balance_value = balance_value
        self.channels = channels
        assert self.channels == 1
        self.align_corners = align_corners
        for r in res_t:
            assert r[0] % 2 == 1 and r[1] % 2 == 1, \
                f"resolution {r} need to be odd becuase of align_corner."
        if any(len({int(v) for v in r}) != 1 for r in res_t) and query_func is None:
            raise IconAmdError("per-axis resolutions are evaluated through query_func (one query over the materialised lattice): pass it")
        self.engine = engine
        self.backend = backend
        self.process_group = process_group
        self.shard = shard
        self.balance_slabs = balance_slabs
        self.overlap_gather = overlap_gather
        if slab_layout not in ("ab", "contiguous"):
            raise IconAmdError("slab_layout must be 'ab' or 'contiguous'")
        self.slab_layout = slab_layout
        self.gather_to = None if gather_to is None else int(gather_to)
        self.reserve_cus = None if reserve_cus is None else int(reserve_cus)   # CUs the persistent MLP kernel leaves to the collective's kernels when sharded (None: auto)
        self.last_stats = {}

    # ------------------------------------------------------------------------------------------
    def _dist(self):
        import torch.distributed as dist
        if not self.shard or not dist.is_available() or not dist.is_initialized():
            return None, 1, 0
        g = self.process_group
        return dist, dist.get_world_size(g), dist.get_rank(g)

    def _res(self):
        """``resolutions`` as Python ints [[W, H, D], ...].  The buffer lives on the device once the module is moved
        there (it is a registered buffer, as upstream); every ``int(self.resolutions[...])`` is then a synchronous
        D2H copy - a dozen of them per forward() cost more than the sign-list kernels.  Read once per (tensor, version)."""
        key = (self.resolutions.data_ptr(), self.resolutions._version)
        if getattr(self, "_res_key", None) != key:
            self._res_cache = [[int(v) for v in row] for row in self.resolutions.cpu().tolist()]
            self._res_key = key
        return self._res_cache

    def _lattice_fast_path(self, proj_matrix) -> bool:
        r = self._res()[-1]
        ok = bool(self.align_corners) and proj_matrix is None and r[0] == r[1] == r[2]
        if not ok:
            return False
        # the bounding-box buffers live on the device: compare them once per (tensor, version), not per call
        key = (self.b_min.data_ptr(), self.b_min._version, self.b_max.data_ptr(), self.b_max._version)
        if getattr(self, "_bbox_key", None) != key:
            self._bbox_ok = (torch.equal(self.b_min.cpu().flatten(), torch.tensor([-1.0, 1.0, -1.0]))
                             and torch.equal(self.b_max.cpu().flatten(), torch.tensor([1.0, -1.0, 1.0])))
            self._bbox_key = key
        return self._bbox_ok

    def _backend_for(self, netG):
        if self.backend is not None:
            return self.backend
        from .engine import IconQueryEngine
        if isinstance(netG, IconQueryEngine):
            return netG
        if self.engine is not None:
            return self.engine
        eng = getattr(netG, "icon_amd_engine", None)
        if eng is None:
            eng = IconQueryEngine.attach(netG)
        return eng

    def forward(self, **kwargs):
        """kwargs as forwarded to query_func (seg3d_lossless.py:139): opt, netG, features, proj_matrix."""
        netG = kwargs.get("netG")
        features = kwargs.get("features")
        proj_matrix = kwargs.get("proj_matrix", None)
        if not self._lattice_fast_path(proj_matrix):
            return self._forward_generic(**kwargs)
        be = self._backend_for(netG)
        res = self._res()[-1][0]
        im_feat = features[-1] if isinstance(features, (list, tuple)) else features
        dist, world, rank = self._dist()
        if world == 1:
            occ = be.eval_slab(im_feat, res, 0, res)
        else:
            occ = self._forward_sharded(be, im_feat, res, dist, world, rank)
        if occ is None:                              # gather_to: this rank is not the destination - its kernels and sends are enqueued;
            if im_feat.is_cuda:                      # drain the stream as the None test does on the destination
                torch.cuda.current_stream(im_feat.device).synchronize()
        else:
            occ = self._none_if_empty(occ)           # (reads a count back: the stream is idle after it)
        # ... so every launch of this call has reported: bad SMPL input (device mesh build) and a shared-walk search that gave
        # up raise HERE, with this image's volume, not one image late.  Sharded: every collective of the step has completed on
        # every rank by now - a rank that raises leaves the others consistent (they meet the error at the next rendezvous)
        if hasattr(be, "poll_mesh_status"):
            be.poll_mesh_status()
        if hasattr(be, "poll_work_status"):
            be.poll_work_status()
        return occ

    def forward_mesh(self, **kwargs):
        """``export_mesh(forward(**kwargs))`` in one step - on one rank exactly that; SHARDED (one image over N GPUs) the ranks
        exchange MESHES instead of the volume: every rank triangulates the cell layers of its own Z-slab (icon_mc_count_range;
        the neighbour's first plane - one plane, 264 KB at 257^3 - is the only part of the volume that travels), the keyed
        vertices and faces are gathered (~6 MB at 257^3 instead of the 68 MB volume) and merged by key: the same vertices and
        faces, in the same order, as marching cubes on the gathered volume.  -> (verts, faces) CPU tensors as export_mesh, or
        None where forward() returns None.  The volume itself exists on no rank: use forward() when it is needed."""
        netG = kwargs.get("netG")
        features = kwargs.get("features")
        dist, world, rank = self._dist()
        if world == 1 or not self._lattice_fast_path(kwargs.get("proj_matrix", None)):
            occ = self.forward(**kwargs)
            return None if occ is None else self.export_mesh(occ)
        be = self._backend_for(netG)
        if not hasattr(be, "slab_finish_gathered"):
            raise IconAmdError("forward_mesh: the sharded mesh exchange needs the HIP engine as backend")
        res = self._res()[-1][0]
        im_feat = features[-1] if isinstance(features, (list, tuple)) else features
        slab, parts = self._forward_sharded(be, im_feat, res, dist, world, rank, local_only=True)
        return self._gather_mesh(slab, parts, res, dist, world, rank, im_feat.device)

    @staticmethod
    def _hip_slab_mesh(buf, z0, res, zc0, zc1, halo, level):
        """marching cubes over the cell layers [zc0, zc1) of the volume whose planes z0, z0 + 1, ... are `buf` (device), the
        x / y edge crossings of layer zc1 included when `halo`; -> (keys [nv] i64, verts [nv,3] f32, faces [nf,3] i64 local)"""
        if not buf.is_cuda:
            raise IconAmdError("forward_mesh: the slab triangulation runs on the HIP device (there is no CPU path)")
        dev = buf.device
        L = _lib.lib()
        work = _mc_workspace(dev)
        virt = C.c_void_p(buf.data_ptr() - z0 * res * res * 4)                    # where plane 0 of the whole volume would be
        cv, cf = C.c_int64(0), C.c_int64(0)
        with torch.cuda.device(dev):
            check(L.icon_mc_count_range(virt, C.c_int(res), C.c_float(level), C.c_int(zc0), C.c_int(zc1), C.c_int(1 if halo else 0),
                                        work.h, stream(), C.byref(cv), C.byref(cf)), "icon_mc_count_range")
            nv, nf = cv.value, cf.value
            verts = torch.empty((max(nv, 1), 3), dtype=torch.float32, device=dev)
            faces = torch.empty((max(nf, 1), 3), dtype=torch.int64, device=dev)
            keys = torch.empty((max(nv, 1),), dtype=torch.int64, device=dev)
            if nv:
                check(L.icon_mc_emit_keyed(_lib.ptr(verts), _lib.ptr(faces), _lib.ptr(keys), work.h, stream()), "icon_mc_emit_keyed")
        return keys[:nv], verts[:nv], faces[:nf]

    def _gather_mesh(self, slab, parts, res, dist, world, rank, dev):
        g = self.process_group
        z0, z1 = parts[rank]
        nz = z1 - z0
        # every rank's first plane: the halo of the rank below it
        first = slab[:1].contiguous() if nz > 0 else torch.zeros((1, res, res), dtype=torch.float32, device=dev)
        firsts = self._all_gather_cat(dist, first, world, g)                      # [world, res, res]
        # forward()'s None rule (_none_if_empty): nothing above 0.5 on the reference's COARSEST lattice - this rank's part of it
        rs = self._res()
        st = [max((rs[-1][k] - 1) // max(rs[0][k] - 1, 1), 1) for k in range(3)]   # x, y, z
        any_pos = bool(nz > 0 and (slab[(-z0) % st[2]:nz:st[2], ::st[1], ::st[0]] > 0.5).any())
        nxt = next((r for r in range(rank + 1, world) if parts[r][1] > parts[r][0]), None)
        nv = nf = 0
        verts = torch.empty((0, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((0, 3), dtype=torch.int64, device=dev)
        keys = torch.empty((0,), dtype=torch.int64, device=dev)
        if nz > 0:
            halo = nxt is not None
            buf = torch.empty((nz + 1, res, res), dtype=torch.float32, device=dev)
            buf[:nz] = slab[:nz]
            if halo:
                buf[nz] = firsts[nxt]
            # a cell layer z reads the planes z + 1 and z + 2: this rank triangulates the layers whose lower plane is its own
            zc0, zc1 = max(z0 - 1, 0), (z1 - 1 if halo else res - 1)
            if zc1 > zc0:
                mesher = getattr(self, "slab_mesher", None) or self._hip_slab_mesh     # (tests inject a CPU stand-in, like `backend`)
                keys, verts, faces = mesher(buf, z0, res, zc0, zc1, halo, float(self.balance_value))
                nv, nf = int(keys.shape[0]), int(faces.shape[0])
        sizes = self._all_gather_cat(dist, torch.tensor([[nv, nf, int(any_pos)]], dtype=torch.int64, device=dev), world, g).tolist()
        if not any(s[2] for s in sizes):
            return None                                                          # forward() returns None: nothing above 0.5 anywhere
        mv, mf = max(max(s[0] for s in sizes), 1), max(max(s[1] for s in sizes), 1)

        # ONE message per rank: [keys i64 x mv | vertices f32 x 3 mv | faces i32 x 3 mf], padded to the largest rank
        nb_k, nb_v, nb_f = mv * 8, mv * 12, mf * 12
        msg = torch.zeros(nb_k + nb_v + nb_f, dtype=torch.uint8, device=dev)
        if nv:
            msg[:nb_k].view(torch.int64)[:nv] = keys[:nv]
            msg[nb_k:nb_k + nb_v].view(torch.float32).view(mv, 3)[:nv] = verts[:nv]
        if nf:
            msg[nb_k + nb_v:].view(torch.int32).view(mf, 3)[:nf] = faces[:nf].to(torch.int32)
        allm = self._all_gather_cat(dist, msg, world, g).view(world, -1)
        all_k = allm[:, :nb_k].contiguous().view(torch.int64).view(world, mv)
        all_v = allm[:, nb_k:nb_k + nb_v].contiguous().view(torch.float32).view(world, mv, 3)
        all_f = allm[:, nb_k + nb_v:].contiguous().view(torch.int32).view(world, mf, 3).to(torch.int64)
        out_v, out_f = merge_keyed_meshes([all_k[r, : sizes[r][0]] for r in range(world)], [all_v[r, : sizes[r][0]] for r in range(world)],
                                          [all_f[r, : sizes[r][1]] for r in range(world)])
        self.last_stats = dict(gather="mesh", exchanged_bytes=int(world * (res * res * 4 + 24 + mv * 20 + mf * 12)), collectives=3, slabs=parts,
                               verts=int(out_v.shape[0]), faces=int(out_f.shape[0]))
        return out_v.cpu(), out_f.cpu()

    @staticmethod
    def _all_gather_cat(dist, t, world, group):
        """all_gather of one equal-shaped tensor per rank, concatenated along dim 0 (ONE collective into
        one output tensor, no per-rank list / cat copies).  RCCL ('nccl') moves device tensors directly;
        a gloo group (CPU tests, or several ranks debugging on one GPU) stages device tensors through the host."""
        if t.is_cuda and dist.get_backend(group) == "gloo":
            out = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype)
            dist.all_gather_into_tensor(out, t.cpu().contiguous(), group=group)
            return out.to(t.device)
        out = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        dist.all_gather_into_tensor(out, t.contiguous(), group=group)
        return out

    def _plane_weights(self, be, res):
        """cost model of the Z-slab cut (see plane_weights); None -> uniform"""
        if not self.balance_slabs:
            return None
        zr = getattr(be, "mesh_z_range", None)
        zr = zr() if callable(zr) else None
        return None if zr is None else plane_weights(res, zr[0], zr[1])

    def _shard_buffers(self, key, per, res, stride, dev):
        """slab / message buffers of the sharded path, allocated once per (resolution, world, device)"""
        if getattr(self, "_shard_key", None) != key:
            self._shard_slab = torch.zeros((per, res, res), dtype=torch.float32, device=dev)
            self._shard_msg = torch.zeros(stride, dtype=torch.int8, device=dev)
            self._shard_key = key
        return self._shard_slab, self._shard_msg

    def _slab_cuts(self, be, res, dist, world, rank, dev):
        """The Z-slab partition every rank uses.  The cost-weighted cut depends on float min/max of the SMPL vertices;
        ranks whose replicas of those tensors differ in the last bit (non-deterministic upstream kernels) could derive
        different cuts and then disagree on message sizes and offsets - so rank 0's cut is the cut: it is broadcast
        once per (resolution, world, body) and cached (every rank misses the cache on the same call: the key changes
        exactly when filter() produced new SMPL tensors, which all ranks do in lockstep)."""
        if not self.balance_slabs:
            return slab_partition(res, world, None)
        zr = getattr(be, "mesh_z_range", None)
        if callable(zr):
            zr()                                                     # binds the mesh handle: its key is part of the cache key
        key = (res, world, getattr(be, "_mesh_key", None))
        if getattr(self, "_cuts_key", None) == key and key[2] is not None:
            return self._cuts
        parts = slab_partition(res, world, self._plane_weights(be, res))
        g = self.process_group
        cpu_group = dist.get_backend(g) == "gloo"
        t = torch.tensor([a for a, _ in parts] + [parts[-1][1]], dtype=torch.int64, device="cpu" if cpu_group else dev)
        dist.broadcast(t, src=dist.get_global_rank(g, 0) if g is not None else 0, group=g)
        c = [int(v) for v in t.tolist()]
        parts = [(c[r], c[r + 1]) for r in range(world)]
        self._cuts_key, self._cuts = key, parts
        return parts

    def _forward_sharded(self, be, im_feat, res, dist, world, rank, local_only=False):
        g = self.process_group
        dev = im_feat.device
        want = self.reserve_cus
        if want is None:                 # auto: RCCL's kernels need CUs of their own to run BESIDE the persistent MLP grid
            want = 16 if (self.overlap_gather and dist.get_backend(g) == "nccl") else 0
        if hasattr(be, "_work") and getattr(self, "_reserved", None) != want:
            be._work().set_reserve_cus(want)
            if getattr(be, "split_features", False):
                be._work(1).set_reserve_cus(want)
            self._reserved = want
        self.reserve_cus_effective = want
        parts = self._slab_cuts(be, res, dist, world, rank, dev)
        z0, z1 = parts[rank]
        per = max(b - a for a, b in parts)
        # message of the sign exchange: [int64 count][2 bits per outlier sign, padded to the largest slab], 8-byte aligned
        stride = sign_message_bytes(per * res * res)
        slab, msg = self._shard_buffers((res, world, rank, str(dev), per), per, res, stride, dev)
        need_exchange = (getattr(be, "cmap_mode", "local") == "reference" and getattr(be, "prior_type", "icon") == "icon"
                         and "cmap" in getattr(be, "smpl_feats", ("cmap",)))   # the tiled cmap rule is what couples the ranks
        pieces = hasattr(be, "slab_finish_gathered")
        if (self.slab_layout == "ab" and pieces and self.overlap_gather and not local_only and getattr(be, "split_features", False)
                and -(-res // world) > 1 and 2 * world <= 64):
            return self._forward_sharded_ab(be, im_feat, res, dist, world, rank, need_exchange)
        if self.gather_to is not None and not local_only:
            raise IconAmdError("gather_to needs the 'ab' slab layout (overlap_gather=True, the HIP engine as backend)")
        # the volume is gathered in two halves of every rank's (padded) slab: the first half travels over xGMI while
        # the second half is still in the MLP kernel
        per_a = (per + 1) // 2 if (self.overlap_gather and pieces and per > 1 and not local_only) else per
        handles = []

        def gather_async(t):
            if t.is_cuda and dist.get_backend(g) == "gloo":                    # debugging aid: staged through the host, synchronous
                return self._all_gather_cat(dist, t, world, g), None
            out = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            return out, dist.all_gather_into_tensor(out, t, group=g, async_op=True)

        # Split phase 1 (round 5): with the volume gathered in two halves anyway, each half-slab also runs ITS OWN geometry pass
        # (its own workspace) and exchanges its own sign message - asynchronously: the first half's all_gather is in flight while
        # k_nearest of the second half runs, instead of every rank's MLP waiting for one blocking exchange behind the whole
        # slab's search.  A rank's outlier list is (first half) ++ (second half) in the lattice's order, so the 2 x world
        # messages, interleaved [r0a, r0b, r1a, r1b, ...], are the very list of the unsplit protocol: the same bits.
        split = bool(pieces and need_exchange and per_a < per and getattr(be, "split_features", False) and 2 * world <= 64)
        order = []                                           # what was enqueued, in order (tests read it)
        if split:
            stride_h = sign_message_bytes(per_a * res * res)
            hkey = (res, world, rank, str(dev), per_a)
            if getattr(self, "_shard_half_key", None) != hkey:
                self._shard_half_msg = torch.zeros((2, stride_h), dtype=torch.int8, device=dev)
                self._shard_half_key = hkey
            zm = min(z1, z0 + per_a)
            halves = ((z0, zm), (zm, z1))
            got, waits = [], []
            for hf, (a0, a1) in enumerate(halves):
                m = self._shard_half_msg[hf]
                m[:8].zero_()
                if a1 > a0:
                    be.slab_features(im_feat, res, a0, a1, msg=m, work=hf)
                order.append(f"features_{'ab'[hf]}")
                g_h, hd = gather_async(m)
                order.append(f"gather_signs_{'ab'[hf]}" + ("" if hd is None else "_async"))
                got.append(g_h)
                waits.append(hd)
            for hd in waits:
                if hd is not None:
                    hd.wait()
            order.append("wait_signs")
            gathered = torch.stack([got[0].view(world, stride_h), got[1].view(world, stride_h)], 1).reshape(-1)   # [world, 2, stride_h]
            vols = []
            for hf, (a0, a1) in enumerate(halves):
                if a1 > a0:
                    be.slab_finish_gathered(res, a0, a1, gathered, stride_h, 2 * world, 2 * rank + hf, out=slab[a0 - z0: a1 - z0], device=dev, work=hf)
                order.append(f"finish_{'ab'[hf]}")
                v_h, hd = gather_async(slab[:per_a] if hf == 0 else slab[per_a:])
                order.append(f"gather_volume_{'ab'[hf]}" + ("" if hd is None else "_async"))
                vols.append(v_h)
                handles.append(hd)
            for hd in handles:
                if hd is not None:
                    hd.wait()
            allv = torch.empty((world, per, res, res), dtype=torch.float32, device=vols[0].device)
            allv[:, :per_a] = vols[0].view(world, per_a, res, res)
            allv[:, per_a:] = vols[1].view(world, per - per_a, res, res)
            self.last_stats = dict(exchanged_bytes=2 * stride_h * world, collectives=4, slabs=parts, split_features=True, order=order)
        elif pieces:
            gathered = None
            if need_exchange:
                # ONE collective, no host synchronisation: every rank contributes a fixed-size message; phase 1 writes
                # straight into it and phase 2 consumes the gathered buffer as it is (K, rank offset and segment lookup
                # happen on the device), so the exchange and the MLP launch are enqueued back to back.
                msg[:8].zero_()
                if z1 > z0:
                    be.slab_features(im_feat, res, z0, z1, msg=msg)
                gathered = self._all_gather_cat(dist, msg, world, g)
            elif z1 > z0:
                be.slab_features(im_feat, res, z0, z1)
            zm = min(z1, z0 + per_a)
            if zm > z0:
                be.slab_finish_gathered(res, z0, z1, gathered, stride, world, rank, out=slab[: z1 - z0], za=z0, zb=zm, device=dev)
            if local_only:                       # forward_mesh: the slab stays here, meshes travel
                return slab, parts
            vol_a, h = gather_async(slab[:per_a])
            handles.append(h)
            vol_b = None
            if per_a < per:
                if z1 > zm:
                    be.slab_finish_gathered(res, z0, z1, gathered, stride, world, rank, out=slab[: z1 - z0], za=zm, zb=z1, device=dev)
                vol_b, h = gather_async(slab[per_a:])
                handles.append(h)
            for h in handles:
                if h is not None:
                    h.wait()
            if vol_b is None:
                allv = vol_a.view(world, per, res, res)
            else:
                allv = torch.empty((world, per, res, res), dtype=torch.float32, device=vol_a.device)
                allv[:, :per_a] = vol_a.view(world, per_a, res, res)
                allv[:, per_a:] = vol_b.view(world, per - per_a, res, res)
            self.last_stats = dict(exchanged_bytes=stride * world if need_exchange else 0, collectives=(1 if need_exchange else 0) + len(handles),
                                   slabs=parts)
        else:
            # backends without the device-side protocol: counts through the host, explicit global list
            if need_exchange:
                if z1 > z0:
                    signs, count = be.slab_features(im_feat, res, z0, z1)
                else:
                    signs = torch.empty(0, dtype=torch.int8, device=dev)
                    count = torch.zeros(1, dtype=torch.int64, device=dev)
                counts = self._all_gather_cat(dist, count.view(1), world, g).tolist()      # one host sync
                kmax = max(max(counts), 1)
                mine = torch.zeros(kmax, dtype=torch.int8, device=dev)
                mine[:counts[rank]] = signs[:counts[rank]]
                gl = self._all_gather_cat(dist, mine, world, g).view(world, kmax)
                if sum(counts):
                    signs_global = torch.cat([gl[r, :c] for r, c in enumerate(counts)]).contiguous()
                else:
                    signs_global = mine[:0]
                if z1 > z0:
                    be.slab_finish(res, z0, z1, signs_global, sum(counts), sum(counts[:rank]),
                                   out=slab[: z1 - z0], device=dev)
                self.last_stats = dict(outliers=sum(counts), exchanged_bytes=kmax * world, slabs=parts)
            else:
                if z1 > z0:
                    be.eval_slab(im_feat, res, z0, z1, out=slab[: z1 - z0])
                self.last_stats = dict(exchanged_bytes=0, collectives=1, slabs=parts)
            allv = self._all_gather_cat(dist, slab, world, g).view(world, per, res, res)
        if all(b - a == per for a, b in parts):
            return allv.view(world * per, res, res)[:res]
        return torch.cat([allv[r, : b - a] for r, (a, b) in enumerate(parts)], 0)   # unequal slabs: drop each rank's padding planes

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def ab_pieces(res: int, world: int):
        """The 'ab' partition: per = ceil(res / world) planes per rank, pa = ceil(per / 2) of them in the A part [0, world pa) of the
        volume and pb = per - pa in the B part behind it; rank r owns A_r = [r pa, (r + 1) pa) and B_r = [world pa + r pb,
        world pa + (r + 1) pb), clipped to the lattice (the last pieces may be short or empty).  -> (pa, pb, [(A_r, B_r)])"""
        per = -(-res // world)
        pa = (per + 1) // 2
        pb = per - pa
        clip = lambda z: min(z, res)
        return pa, pb, [((clip(r * pa), clip((r + 1) * pa)), (clip(world * pa + r * pb), clip(world * pa + (r + 1) * pb))) for r in range(world)]

    def _forward_sharded_ab(self, be, im_feat, res, dist, world, rank, need_exchange):
        """Two slabs per rank, each a complete pipeline on its own workspace: geometry pass, its own 2-bit sign message, asynchronous
        exchange; MLP; asynchronous volume gather STRAIGHT into its block of the result.  Lattice order of the 2 x world pieces =
        A_0 .. A_{w-1}, B_0 .. B_{w-1} = the order the two sign gathers leave their messages in ONE buffer [2, world, stride]: the
        very outlier list of the unsharded call (piece h of rank r is message h world + r).  The volume is ONE fresh buffer
        [world per, res, res]; gather A fills [0, world pa), gather B the rest; the result is its first `res` planes - a view."""
        g = self.process_group
        dev = im_feat.device
        pa, pb, pieces = self.ab_pieces(res, world)
        mine = pieces[rank]
        gloo_dev = dev.type == "cuda" and dist.get_backend(g) == "gloo"       # debugging aid: device tensors staged through the host
        dst = self.gather_to
        if dst is not None and not (0 <= dst < world):
            raise IconAmdError(f"gather_to={dst}: no such rank in a group of {world}")
        key = (res, world, rank, str(dev), "ab")
        if getattr(self, "_ab_key", None) != key:
            stride = sign_message_bytes(pa * res * res)
            self._ab_slab = [torch.zeros((pa, res, res), dtype=torch.float32, device=dev), torch.zeros((max(pb, 1), res, res), dtype=torch.float32, device=dev)]
            self._ab_msg = torch.zeros((2, stride), dtype=torch.int8, device=dev)
            self._ab_stride = stride
            self._ab_key = key
        slab, msg, stride = self._ab_slab, self._ab_msg, self._ab_stride
        receives = dst is None or dst == rank
        vol = torch.empty(((pa + pb) * world, res, res), dtype=torch.float32, device=dev) if receives else None
        blocks = (slice(0, world * pa), slice(world * pa, world * (pa + pb)))
        order = []

        def gather_signs(h, sig):
            if gloo_dev:
                out = torch.empty(world * stride, dtype=torch.int8)
                dist.all_gather_into_tensor(out, msg[h].cpu(), group=g)
                sig[h].view(-1).copy_(out)
                return None
            return dist.all_gather_into_tensor(sig[h].view(-1), msg[h], group=g, async_op=True)

        def gather_volume(h):
            n = pa if h == 0 else pb
            if n == 0:
                return None
            src = slab[h][:n]
            if dst is None:
                if gloo_dev:
                    out = torch.empty((world * n, res, res), dtype=torch.float32)
                    dist.all_gather_into_tensor(out, src.cpu(), group=g)
                    vol[blocks[h]].copy_(out)
                    return None
                return dist.all_gather_into_tensor(vol[blocks[h]], src, group=g, async_op=True)
            root = dist.get_global_rank(g, dst) if g is not None else dst
            if gloo_dev:
                lst = [torch.empty((n, res, res), dtype=torch.float32) for _ in range(world)] if receives else None
                dist.gather(src.cpu(), lst, dst=root, group=g)
                if receives:
                    vol[blocks[h]].copy_(torch.cat(lst))
                return None
            # the destination receives every rank's piece directly in its place (one contiguous view per rank)
            lst = [vol[blocks[h]][r * n:(r + 1) * n] for r in range(world)] if receives else None
            return dist.gather(src, lst, dst=root, group=g, async_op=True)

        sig = torch.empty((2, world, stride), dtype=torch.int8, device=dev) if need_exchange else None
        waits = []
        if need_exchange:
            for h, (z0, z1) in enumerate(mine):
                msg[h][:8].zero_()
                if z1 > z0:
                    be.slab_features(im_feat, res, z0, z1, msg=msg[h], work=h)
                order.append(f"features_{'ab'[h]}")
                hd = gather_signs(h, sig)
                order.append(f"gather_signs_{'ab'[h]}" + ("" if hd is None else "_async"))
                waits.append(hd)
            for hd in waits:
                if hd is not None:
                    hd.wait()
            order.append("wait_signs")
        handles = []
        for h, (z0, z1) in enumerate(mine):
            if not need_exchange:
                if z1 > z0:
                    be.slab_features(im_feat, res, z0, z1, work=h)
                order.append(f"features_{'ab'[h]}")
            if z1 > z0:
                be.slab_finish_gathered(res, z0, z1, sig.view(-1) if need_exchange else None, stride, 2 * world, h * world + rank,
                                        out=slab[h][: z1 - z0], device=dev, work=h)
            order.append(f"finish_{'ab'[h]}")
            hd = gather_volume(h)
            order.append(f"gather_volume_{'ab'[h]}" + ("" if hd is None else "_async"))
            handles.append(hd)
        for hd in handles:
            if hd is not None:
                hd.wait()
        self.last_stats = dict(exchanged_bytes=2 * stride * world if need_exchange else 0, collectives=(2 if need_exchange else 0) + 2,
                               slabs=[(a[0], b[1]) for a, b in pieces], pieces=pieces, split_features=True, order=order, layout="ab",
                               gather_to=dst, assembly_copies=0)
        return vol[:res] if receives else None

    def _forward_generic(self, **kwargs):
        """Any b_min/b_max/align_corners/proj_matrix: materialise the lattice coordinates exactly as
        batch_eval does and issue ONE query over them (Seg3dLossless with a single resolution)."""
        if self.query_func is None:
            raise IconAmdError("generic lattice path needs query_func")
        W, H, D = self._res()[-1]                              # per-axis resolutions (seg3d_lossless.py:66-71) take this path
        feats = kwargs.get("features")
        dev = (feats[-1] if isinstance(feats, (list, tuple)) else feats).device
        pts = lattice_coords((W, H, D), self.b_min.to(dev), self.b_max.to(dev), self.align_corners, dev)
        occ = self.query_func(**kwargs, points=pts)
        if type(occ) is list:
            occ = torch.stack(occ)
        assert len(occ.size()) == 3, "query_func should return a occupancy with shape of [bz, C, N]"
        return self._none_if_empty(occ.view(D, H, W))

    def _none_if_empty(self, occ):
        """The reference returns None when nothing exceeds 0.5 on its coarsest lattice
        (seg3d_lossless.py:173-177); those points are the stride-s sub-lattice of ours."""
        rs = self._res()
        st = [max((rs[-1][k] - 1) // max(rs[0][k] - 1, 1), 1) for k in range(3)]   # x, y, z
        if occ.is_cuda and occ.is_contiguous() and occ.dtype == torch.float32 and occ.shape[0] == occ.shape[1] == occ.shape[2]:
            # one native kernel + the stream wait the reference's own test implies (icon_volume_any_above)
            hit = C.c_int(0)
            with torch.cuda.device(occ.device):
                check(_lib.lib().icon_volume_any_above(_lib.ptr(occ), C.c_int(occ.shape[0]), C.c_int(st[0]), C.c_int(st[1]), C.c_int(st[2]),
                                                       C.c_float(0.5), _mc_workspace(occ.device).h, stream(), C.byref(hit)), "icon_volume_any_above")
            return occ if hit.value else None
        if (occ[::st[2], ::st[1], ::st[0]] > 0.5).sum() == 0:
            return None
        return occ

    # ------------------------------------------------------------------------------------------
    def export_mesh(self, occupancys):
        """lib/common/seg3d_lossless.py:583-604: marching cubes at balance_value on occ[1:,1:,1:];
        returns (verts [Nv,3] float32 in voxel units, x,y,z order; faces [Nf,3] int64)."""
        if len(set(occupancys.shape)) != 1:
            # per-axis resolutions: the marching-cubes kernels take a cube - pad the high end of the short axes with
            # zeros (the lattice's own outer shell is 0 by in_cube, so the padding adds no surface and moves no vertex)
            n = max(occupancys.shape)
            padded = occupancys.new_zeros((n, n, n))
            padded[: occupancys.shape[0], : occupancys.shape[1], : occupancys.shape[2]] = occupancys
            occupancys = padded
        if occupancys.is_cuda:
            verts, faces = export_mesh_device(occupancys, float(self.balance_value))
            return verts.cpu(), faces.cpu()          # the reference returns CPU tensors (:601-602)
        occ = occupancys.detach().to("cpu", torch.float32).contiguous()
        return export_mesh_numpy(occ.numpy(), float(self.balance_value))


    # ------------------------------------------------------------------------------------------
    # normal-map preview of a volume (lib/common/seg3d_lossless.py:498-581; used by apps/ICON.py:706)
    def find_vertices(self, sdf, direction="front"):
        """First voxel above 0.5 along the viewing direction for every (x, y) column, the sub-voxel depth
        of the 0.5 crossing and a finite-difference normal (seg3d_lossless.py:498-558).
        -> X [N], Y [N] (long), Z [N] (float), norm [N,3]"""
        resolution = sdf.size(2)
        if direction == "left":
            sdf = sdf.permute(2, 1, 0)
        elif direction == "back":
            sdf = sdf.flip(0)
        elif direction == "right":
            sdf = sdf.flip(2).permute(2, 1, 0)
        elif direction != "front":
            raise IconAmdError(f"unknown direction {direction!r}")
        vol = sdf.flip(0).permute(2, 1, 0)                        # [x, y, depth]
        inside = vol > 0.5
        hit = inside.any(dim=2)
        first = inside.to(torch.uint8).argmax(dim=2)             # first voxel above the level (the reference's shadow mask keeps only it)
        xy = hit.nonzero(as_tuple=False)
        X, Y = xy[:, 0], xy[:, 1]
        Zi = first[X, Y]
        zc, yc, xc = (Zi - 2).clamp(0, resolution), (Y - 2).clamp(0, resolution), (X - 2).clamp(0, resolution)
        v1, v2, v3, v4 = vol[X, Y, Zi], vol[X, Y, zc], vol[X, yc, Zi], vol[xc, Y, Zi]
        Z = (zc.float() * (0.5 - v1) / (v2 - v1) + Zi.float() * (v2 - 0.5) / (v2 - v1)).clamp(0, resolution)
        norm = torch.stack([v4 - v1, v3 - v1, v2 - v1], dim=1)
        norm = norm / torch.norm(norm, p=2, dim=1, keepdim=True)
        return X.long(), Y.long(), Z, norm

    def render_normal(self, resolution, X, Y, Z, norm):
        image = torch.ones((1, 3, resolution, resolution), dtype=torch.float32, device=norm.device)
        image[0, :, Y, X] = ((norm + 1) / 2.0).clamp(0, 1).t()
        return image

    def display(self, sdf):
        """[res, 4*res, 3] uint8: front | left | right | back normal renderings (seg3d_lossless.py:566-581)"""
        res = self._res()[-1][-1]
        views = [self.render_normal(res, *self.find_vertices(sdf, d)) for d in ("front", "left", "right", "back")]
        image = torch.cat(views, dim=3)
        return np.uint8(image.detach().cpu().numpy()[0].transpose(1, 2, 0) * 255.0)


def mesh_components(faces: torch.Tensor, n_verts: int) -> torch.Tensor:
    """[V] int32 component label of every vertex (the smallest vertex index of its component), computed on
    the device by icon_mesh_components (union-find over the faces)."""
    if not faces.is_cuda:
        raise IconAmdError("mesh_components needs device tensors (there is no CPU path)")
    f = faces.detach().to(torch.int64).reshape(-1, 3).contiguous()
    labels = torch.empty(int(n_verts), dtype=torch.int32, device=f.device)
    check(_lib.lib().icon_mesh_components(_lib.ptr(f), C.c_int64(f.shape[0]), C.c_int64(int(n_verts)), _lib.ptr(labels), stream()),
          "icon_mesh_components")
    return labels


def face_components(faces: torch.Tensor, n_verts: int) -> torch.Tensor:
    """[F] int64 component label of every FACE under trimesh's notion of connectivity (graph.split ->
    face_adjacency): two faces are adjacent when they share an EDGE that exactly two faces use - faces that merely
    touch in a vertex (marching-cubes pinch points) are NOT connected.  The edge grouping is torch plumbing (sort by
    edge key); the components themselves come from the device union-find (icon_mesh_components on the adjacency
    graph, one node per face).  Label = the smallest face index of the component."""
    f = faces.detach().to(torch.int64).reshape(-1, 3)
    F = f.shape[0]
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    key = torch.minimum(e[:, 0], e[:, 1]) * int(n_verts) + torch.maximum(e[:, 0], e[:, 1])
    fid = torch.arange(F, device=f.device).repeat(3)
    order = torch.argsort(key)
    ks, fs = key[order], fid[order]
    _, counts = torch.unique_consecutive(ks, return_counts=True)
    starts = torch.cumsum(counts, 0) - counts
    two = starts[counts == 2]                                    # edges used by exactly two faces (grouping.group_rows(..., require_count=2))
    if two.numel() == 0:
        return torch.arange(F, device=f.device)
    a, b = fs[two], fs[two + 1]
    pairs = torch.stack([a, b, b], 1).contiguous()              # an adjacency as a degenerate "triangle" of the face graph
    return mesh_components(pairs, F).long()


def clean_mesh(verts: torch.Tensor, faces: torch.Tensor):
    """Drop-in for ``lib.dataset.mesh_util.clean_mesh`` (mesh_util.py:778-791): trimesh's ``split(only_watertight=
    False)`` - connected components over FACE adjacency (shared edges; see face_components) - and the component with
    the most vertices kept (ties: the one containing the lowest-index face); vertices and faces keep their relative
    order, as trimesh's submesh does.  Returns (verts float32, faces int32) on the device of ``verts`` - the reference
    returns ``.float()`` / ``.int()`` tensors on ``verts.device``.  Inputs on the host (export_mesh returns CPU
    tensors, seg3d_lossless.py:601-602) are moved to the current HIP device for the labelling.
    ONE native call since round 4 (icon_clean_mesh, csrc/clean_mesh.hip: edge hash table, union-find over the faces, vertex
    counts, order-preserving compaction; 2.0 ms of torch sort / unique / bincount operators before)."""
    need_device("clean_mesh")
    out_dev = verts.device
    dev = verts.device if verts.is_cuda else torch.device("cuda", torch.cuda.current_device())
    v = verts.detach().to(dev, torch.float32).reshape(-1, 3).contiguous()
    f = faces.detach().to(dev, torch.int64).reshape(-1, 3).contiguous()
    if f.shape[0] == 0 or v.shape[0] == 0:
        return v.float().to(out_dev), f.int().to(out_dev)
    with torch.cuda.device(dev):
        ov = torch.empty_like(v)
        of = torch.empty((f.shape[0], 3), dtype=torch.int32, device=dev)
        hc = (C.c_int64 * 2)()
        check(_lib.lib().icon_clean_mesh(_lib.ptr(v), C.c_int64(v.shape[0]), _lib.ptr(f), C.c_int64(f.shape[0]), _lib.ptr(ov), _lib.ptr(of),
                                         hc, _mc_workspace(dev).h, stream()), "clean_mesh")
    return ov[: hc[0]].to(out_dev), of[: hc[1]].to(out_dev)


_mc_tls = threading.local()


def _mc_workspace(device: torch.device):
    """marching-cubes scratch: one workspace per (thread, device) - a process may drive several GPUs, from several threads"""
    from .engine import Workspace
    pool = getattr(_mc_tls, "pool", None)
    if pool is None:
        pool = _mc_tls.pool = {}
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in pool:
        pool[idx] = Workspace()
    return pool[idx]


def _qc_shapes(verts, faces, image):
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] == 0:
        raise IconAmdError(f"query_color: verts must be [V,3], got {tuple(verts.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
        raise IconAmdError(f"query_color: faces must be [F,3], got {tuple(faces.shape)}")
    if faces.dtype.is_floating_point or faces.dtype == torch.bool:
        raise IconAmdError(f"query_color: faces must be an integer tensor, got {faces.dtype}")
    if image.dim() != 4 or image.shape[1] != 3 or image.shape[2] == 0 or image.shape[3] == 0:
        raise IconAmdError(f"query_color: image must be [1,3,H,W], got {tuple(image.shape)}")
    if image.shape[0] != 1:
        raise IconAmdError(f"query_color: image batch must be 1 (one grid of vertices is sampled), got {image.shape[0]}")


def _query_color_launch(verts, faces, image, image_size, return_vis, return_bad):
    """validates, enqueues icon_query_color on the current stream -> (colors, vis or None, bad or None); bad: a device int32 [1],
    the number of faces the call skipped because they name a vertex that does not exist (copied out of the scratch header on
    the same stream)"""
    _qc_shapes(verts, faces, image)
    need_device("query_color")
    if not (verts.is_cuda and faces.is_cuda and image.is_cuda) or not (verts.device == faces.device == image.device):
        raise IconAmdError("query_color_device: verts, faces and image must live on one HIP device (query_color moves host tensors)")
    dev = verts.device
    v = verts.detach().to(torch.float32).contiguous()
    f, f_i64 = faces_arg(faces)
    img = image.detach().to(torch.float32).contiguous()
    L = _lib.lib()
    with torch.cuda.device(dev):
        scratch = scratch_for(dev, "icon_query_color_bytes", C.c_int64(v.shape[0]), C.c_int64(f.shape[0]), C.c_int(int(image_size)))
        colors = torch.empty((v.shape[0], 3), dtype=torch.float32, device=dev)
        vis = torch.empty(v.shape[0], dtype=torch.float32, device=dev) if return_vis else None
        check(L.icon_query_color(_lib.ptr(v), C.c_int64(v.shape[0]), _lib.ptr(f), C.c_int64(f.shape[0]), f_i64,
                                 _lib.ptr(img), C.c_int(img.shape[2]), C.c_int(img.shape[3]), C.c_int(int(image_size)), _lib.ptr(colors),
                                 _lib.ptr(vis), _lib.ptr(scratch), C.c_int64(scratch.numel()), stream()), "icon_query_color")
        bad = scratch[:4].view(torch.int32).clone() if return_bad else None     # first word of the header (include/icon_amd.h)
    return colors, vis, bad


def query_color_device(verts: torch.Tensor, faces: torch.Tensor, image: torch.Tensor, image_size: int = 2 ** 12, return_vis: bool = False):
    """``query_color`` with everything left on the device: ``verts [V,3]``, ``faces [F,3]`` (int32 - what clean_mesh returns -
    or int64 - what export_mesh_device returns - read in place), ``image [1,3,H,W]``, all on one HIP device ->
    ``colors [V,3]`` float32 there (and ``vis [V]`` with ``return_vis``).  ONE native call (icon_query_color) enqueued on the
    current stream: nothing is allocated by it, nothing read back, the stream is not waited for - so a face that names a vertex
    that does not exist cannot raise here; such a face is skipped (it covers no pixel and adds to no normal).  The call's
    scratch is cached per (thread, device, stream): calls on different streams do not share it."""
    colors, vis, _ = _query_color_launch(verts, faces, image, image_size, return_vis, False)
    return (colors, vis) if return_vis else colors


def query_color(verts: torch.Tensor, faces: torch.Tensor, image: torch.Tensor, device=None) -> torch.Tensor:
    """Drop-in for ``lib.common.render.query_color`` (render.py:60-84; apps/infer.py:531 colours the reconstructed mesh with it):
    ``verts [V,3]``, ``faces [F,3]``, ``image [1,3,H,W]`` in [-1,1], host or device tensors -> ``colors [V,3]`` float32 on the CPU,
    0..255: the image sampled at (x, -y) for the vertices ``get_visibility(xy, z, faces[:, [0,2,1]])`` marks, the vertex
    normal mapped to a colour for the others.  ``device``: the HIP device to run on (default: where ``verts`` lives, else the
    current one).  No pytorch3d involved; there is no CPU path."""
    verts, faces, image = torch.as_tensor(verts), torch.as_tensor(faces), torch.as_tensor(image)
    _qc_shapes(verts, faces, image)
    if not faces.is_cuda and (int(faces.min()) < 0 or int(faces.max()) >= verts.shape[0]):      # host data: no device involved
        raise IconAmdError("query_color: face index out of range")
    need_device("query_color")
    dev = torch.device(device) if device is not None else (verts.device if verts.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    if dev.type != "cuda":
        raise IconAmdError(f"query_color: device must be a HIP device, got {dev} (there is no CPU fallback)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    f = faces.detach()
    f = f.to(dev) if f.dtype in (torch.int32, torch.int64) else f.to(dev, torch.int64)
    with torch.cuda.device(dev):
        colors, _, bad = _query_color_launch(verts.detach().to(dev, torch.float32), f, image.detach().to(dev, torch.float32), 2 ** 12, False, faces.is_cuda)
    out = colors.cpu()                                                    # the reference returns a CPU tensor: this waits for the stream
    if bad is not None and int(bad.item()):                                # device faces were not looked at before the launch: the call counted what it skipped
        raise IconAmdError("query_color: face index out of range")
    return out


def merge_keyed_meshes(keys, verts, faces):
    """The pieces of a sharded triangulation (DenseReconEngine.forward_mesh) -> one mesh.  Per rank, in rank order: keys [nv] int64
    (3 * cell + edge direction = the vertex's place in the vertex order of marching cubes on the whole volume; the crossings
    of a plane two ranks share appear in both, with the same coordinates), verts [nv,3], faces [nf,3] indexing the rank's own
    vertices.  Vertices: sorted unique keys; faces: renumbered through the inverse map, concatenated in rank order (= cell
    order).  -> (verts [V,3] float32, faces [F,3] int64)"""
    kk, vv = torch.cat(list(keys)), torch.cat(list(verts))
    uniq, inv = torch.unique(kk, sorted=True, return_inverse=True)
    out_v = torch.empty((uniq.shape[0], 3), dtype=torch.float32, device=vv.device)
    out_v[inv] = vv.to(torch.float32)
    off, ff = 0, []
    for k, f in zip(keys, faces):
        ff.append(inv[f.to(torch.int64) + off])
        off += int(k.shape[0])
    out_f = torch.cat(ff) if ff else torch.empty((0, 3), dtype=torch.int64, device=vv.device)
    return out_v, out_f.reshape(-1, 3)


def export_mesh_device(occ: torch.Tensor, level: float = 0.5):
    """Marching cubes on the GPU (icon_mc_count / icon_mc_emit): device tensors in, device tensors out."""
    occ = occ.detach().to(torch.float32).contiguous()
    assert occ.dim() == 3 and occ.shape[0] == occ.shape[1] == occ.shape[2]
    _mc_work = _mc_workspace(occ.device)
    L = _lib.lib()
    nv, nf = C.c_int64(0), C.c_int64(0)
    check(L.icon_mc_count(_lib.ptr(occ), C.c_int(occ.shape[0]), C.c_float(level), _mc_work.h, stream(), C.byref(nv), C.byref(nf)),
          "icon_mc_count")
    verts = torch.empty((max(nv.value, 1), 3), dtype=torch.float32, device=occ.device)
    faces = torch.empty((max(nf.value, 1), 3), dtype=torch.int64, device=occ.device)
    if nv.value and nf.value:
        check(L.icon_mc_emit(_lib.ptr(verts), _lib.ptr(faces), _mc_work.h, stream()), "icon_mc_emit")
    return verts[: nv.value], faces[: nf.value]


def export_mesh_numpy(occ: np.ndarray, level: float = 0.5):
    occ = np.ascontiguousarray(occ, dtype=np.float32)
    assert occ.ndim == 3 and occ.shape[0] == occ.shape[1] == occ.shape[2]
    res = occ.shape[0]
    L = _lib.lib()
    nv, nf = C.c_int64(0), C.c_int64(0)
    check(L.icon_export_mesh(_lib.ptr(occ), C.c_int(res), C.c_float(level), None, C.byref(nv), None, C.byref(nf)),
          "icon_export_mesh(count)")
    verts = np.empty((max(nv.value, 1), 3), np.float32)
    faces = np.empty((max(nf.value, 1), 3), np.int64)
    check(L.icon_export_mesh(_lib.ptr(occ), C.c_int(res), C.c_float(level), _lib.ptr(verts), C.byref(nv),
                             _lib.ptr(faces), C.byref(nf)), "icon_export_mesh")
    return torch.from_numpy(verts[: nv.value].copy()), torch.from_numpy(faces[: nf.value].copy())


class AdaptiveReconEngine(DenseReconEngine):
    lattice_level0 = True      # answer the coarsest (dense) level with the lattice kernels; False: through query_func like the rest
    native = True              # run the whole schedule as ONE native call (icon_adaptive_eval) where its conditions hold; False:
                               # the host-driven schedule below (torch bookkeeping around HIP queries) - the two give the same volume

    """The reference's coarse-to-fine schedule (``Seg3dLossless._forward_faster``,
    lib/common/seg3d_lossless.py:152-265, the mode apps/ICON.py:89 selects) on top of the fast
    query: evaluate the coarsest lattice, then at every finer level only the voxels near the
    0.5 boundary of the trilinearly upsampled field (dilated by a 9^3 / 7^3 / 3^3 box), and only
    interpolate at the last level.  Since round 4 the schedule runs as ONE native call (``icon_adaptive_eval``,
    csrc/adaptive.hip: every step a HIP kernel, nothing read back between the levels) whenever the standard box /
    align_corners / doubling resolutions / fused f16x3 path hold; the code below is the host-driven form of the same
    schedule for everything else (and the checker of the native one: tests compare the two volumes bit for bit).  ~1 % of the dense lattice is queried (SURVEY.md §0 finding 1), with
    exactly the reference's batches - same points, same order - so the result equals the
    reference's volume up to float rounding of the interpolation (tests compare against
    tests/golden/seg3d_body_adaptive_33_65.npz).  The grid bookkeeping is torch plumbing, as upstream;
    the queries go through ``query_func`` -> ``IconQueryEngine.query`` (HIP).
    """

    def __init__(self, *args, **kwargs):
        # ``faster`` is the 11th parameter of Seg3dLossless.__init__ behind self (lib/common/seg3d_lossless.py:37-51) and ours
        faster = args[10] if len(args) > 10 else kwargs.get("faster", False)
        if not faster:
            raise IconAmdError(
                "AdaptiveReconEngine evaluates Seg3dLossless._forward_faster (lib/common/seg3d_lossless.py:152-265) and needs "
                "faster=True, as the reference's only call site passes it (apps/ICON.py:89).  faster=False - the constructor default "
                "upstream and here - selects the lossless schedule Seg3dLossless._forward (:267-478: re-query the neighbours of every "
                "voxel whose inferred value contradicts the interpolated one), which this package does not implement; upstream's own "
                "_forward raises IndexError at its second level under every PyTorch since 1.5 (float tensors used as indices, :343: "
                "coords_accum = coords / stride).  DenseReconEngine evaluates every lattice point and needs no schedule.")
        super().__init__(*args, **kwargs)

    def forward_mesh(self, **kwargs):
        """``export_mesh(self.forward(**kwargs))`` - the mesh of THIS class's coarse-to-fine volume on every rank.  (The inherited
        form would take the sharded dense route when world > 1: another field - evaluated everywhere instead of interpolated at
        the last level - at ~100x the points.  The schedule is a per-image job of well under a millisecond: nothing to shard.)"""
        occ = self.forward(**kwargs)
        return None if occ is None else self.export_mesh(occ)

    def forward(self, **kwargs):
        import torch.nn.functional as F
        if self.query_func is None:
            raise IconAmdError("AdaptiveReconEngine needs query_func")
        res_list = [r[0] for r in self._res()]
        last = res_list[-1]
        feats = kwargs.get("features")
        dev = (feats[-1] if isinstance(feats, (list, tuple)) else feats).device
        b_min, b_max = self.b_min.to(dev), self.b_max.to(dev)
        rr_cache = []

        def batch_eval(coords):                      # coords [1,N,3] in finest-lattice index units (x,y,z)
            if not rr_cache:                         # (made on first use: a host-to-device copy the native schedule never needs)
                rr_cache.append(torch.tensor([last, last, last], device=dev))
            rr = rr_cache[0]
            if self.align_corners:
                c = coords.float() / (rr - 1)
            else:
                c = coords.float() / rr + (1.0 / rr.float()) / 2
            occ = self.query_func(**kwargs, points=c * (b_max - b_min) + b_min)
            if type(occ) is list:
                occ = torch.stack(occ)
            return occ

        def dilate(mask, k):
            # SmoothConv3D(k) > 0 (seg3d_utils.py:169-181: a k^3 box filter of a 0/1 mask) == box dilation;
            # a box is separable, so three 1-D max filters give exactly the same voxel set as the
            # reference's dense conv3d (which cost 1.9 of the 6 ms of this schedule)
            r = (k - 1) // 2
            m = F.max_pool3d(mask, (k, 1, 1), stride=1, padding=(r, 0, 0))
            m = F.max_pool3d(m, (1, k, 1), stride=1, padding=(0, r, 0))
            m = F.max_pool3d(m, (1, 1, k), stride=1, padding=(0, 0, r))
            return (m > 0)[0, 0]

        # the standard box, align_corners, no projection, an engine behind netG: the dense level can use the lattice kernels
        # (only an engine that is already there - never attach one behind the caller's back: the queries of this class go
        #  through whatever query_func / netG the caller passed)
        lattice_engine = None
        if self.lattice_level0 and self._lattice_fast_path(kwargs.get("proj_matrix", None)):
            from .engine import IconQueryEngine
            netG = kwargs.get("netG")
            cand = netG if isinstance(netG, IconQueryEngine) else (self.engine or getattr(netG, "icon_amd_engine", None))
            if isinstance(cand, IconQueryEngine) and self.query_func is not None and getattr(self.query_func, "__module__", "") == "icon_amd.engine":
                lattice_engine = cand
        # the whole schedule as kernels on the stream (csrc/adaptive.hip): boundary test, dilation, compaction in the reference's
        # point order, one query per level, scatter, upsample - no torch op, no read-back between the levels
        if (self.native and self.lattice_level0 and lattice_engine is not None and len(res_list) >= 1
                and all(res_list[k] == 2 * res_list[k - 1] - 1 for k in range(1, len(res_list)))):
            im_feat = feats[-1] if isinstance(feats, (list, tuple)) else feats
            got = []
            why = lattice_engine.native_schedule_reason(im_feat, _handle_out=got)
            if why is None:
                vol, counts, any_pos = lattice_engine.adaptive_eval(im_feat, res_list, float(self.balance_value), _mlp=got[0] if got else None)
                self.last_stats = dict(queries=[counts[0]] + [c for c in counts[1:-1] if c > 0], native=True)
                return vol if any_pos else None
            refused = why
        else:
            refused = None
        occupancys = done = None                     # done[z,y,x]: voxel already evaluated (the reference keeps a
        self.last_stats = dict(queries=[], native=False)   # sorted coordinate list, coords_accum, for the same purpose)
        if refused is not None:
            self.last_stats["native_refused"] = refused     # why the one-call schedule did not run (bench.py / tests read it)
        for level, res in enumerate(res_list):
            stride = (last - 1) // (res - 1)
            if level == 0:
                if lattice_engine is not None and (last - 1) % (res - 1) == 0:
                    # the coarsest level IS a dense lattice: its points (multiples of the stride, mapped by batch_eval) are
                    # bit for bit the points of the res^3 lattice, in the same z,y,x order and as ONE call - so the lattice
                    # kernels answer it (packet search over 4x4x4 blocks instead of one wavefront per scattered point)
                    im_feat = feats[-1] if isinstance(feats, (list, tuple)) else feats
                    occupancys = lattice_engine.eval_slab(im_feat, res, 0, res).view(1, 1, res, res, res)
                    self.last_stats["queries"].append(res ** 3)
                else:
                    ar = torch.linspace(0, last - 1, res, device=dev).long()
                    gd, gh, gw = torch.meshgrid([ar, ar, ar], indexing="ij")
                    coords = torch.stack([gw, gh, gd]).view(3, -1).t().unsqueeze(0)
                    occupancys = batch_eval(coords).view(1, 1, res, res, res)
                    self.last_stats["queries"].append(int(coords.shape[1]))
                if (occupancys > 0.5).sum() == 0:
                    return None
                done = torch.ones((res, res, res), dtype=torch.bool, device=dev)
                continue
            if level == len(res_list) - 1:           # "last step no examine" (seg3d_lossless.py:157,186-203)
                occupancys = F.interpolate(occupancys.float(), size=(res, res, res), mode="trilinear", align_corners=True)
                break
            valid = F.interpolate((occupancys > self.balance_value).float(), size=(res, res, res), mode="trilinear",
                                  align_corners=True)
            occupancys = F.interpolate(occupancys.float(), size=(res, res, res), mode="trilinear", align_corners=True)
            prev_done, done = done, torch.zeros((res, res, res), dtype=torch.bool, device=dev)
            done[::2, ::2, ::2] = prev_done          # coords_accum * 2
            is_boundary = dilate(((valid > 0.0) & (valid < 1.0)).float(), 9 if level == 1 else (7 if level == 2 else 3))
            is_boundary &= ~done
            point_coords = is_boundary.permute(2, 1, 0).nonzero(as_tuple=False).unsqueeze(0)    # (x,y,z), z fastest
            if point_coords.size(1) == 0:
                continue
            idx = point_coords[:, :, 2] * res * res + point_coords[:, :, 1] * res + point_coords[:, :, 0]
            vals = batch_eval(point_coords * stride)
            self.last_stats["queries"].append(int(point_coords.shape[1]))
            occupancys = occupancys.reshape(1, 1, -1).scatter_(2, idx.unsqueeze(1), vals).view(1, 1, res, res, res)
            done.view(-1)[idx.view(-1)] = True
        return occupancys[0, 0]

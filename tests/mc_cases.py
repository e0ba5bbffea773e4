"""The volumes of the marching-cubes size / level / slab tests (tests/test_mc_cases.py on the CPU, tests/test_gpu_mc_sizes.py on
the device) and the comparison with the independent classic implementation (oracle/mc_classic.py) - numpy only, no GPU.

Every generator returns a float32 [res, res, res] array (z slowest, as the reference's volume), seeded, finite values only.
Marching cubes runs on ``vol[1:, 1:, 1:]`` (lib/common/seg3d_lossless.py:585): the CROPPED grid has n = res - 1 points per axis,
its points are the "cells" of csrc/mc_device.hip (a point is the low corner of a cube when all three indices are < n - 1).

Sizes: SIZES_SMALL covers the four residues of (res - 1) % 4 (k_mc_classify4 serves residue 0, k_mc_classify the rest) from one
cube up, cell counts 8 ... 4,913: below one 1,024-cell workgroup, at a multiple of it (res 17: 16^3 = 4 x 1,024) and just past
one (res 18).  SIZES_SCAN sits on the switch from the one-workgroup scan of the block totals to the two-pass scan: res 204 has
8,170 blocks, res 205 has 8,291, the switch is at 8,192.
"""
import math
import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import mc_classic  # noqa: E402

SIZES_SMALL = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 17, 18]
SIZES_MID = [34, 35, 36, 37, 50]
SIZES_SCAN = [204, 205, 206]
KINDS = ["noise", "at_level", "border"]
LEVELS = ["0.5", "0.37", "0.0"]          # "0.0": level 0.0 on the level-0.5 volume minus 0.5


# ---------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------
def noise(res, seed):
    """uniform [0, 1): open at the border, every ambiguous configuration"""
    return np.random.RandomState(seed).random_sample((res, res, res)).astype(np.float32)


def noise_box(shape, seed):
    """the same for a (D, H, W) box: DenseReconEngine.export_mesh pads it to a cube"""
    return np.random.RandomState(seed).random_sample(tuple(shape)).astype(np.float32)


def ellipsoid(res):
    """the closed surface of test_merge_of_keyed_mesh_pieces_restores_the_whole_mesh"""
    z, y, x = np.meshgrid(*([np.linspace(-1, 1, res)] * 3), indexing="ij")
    return (0.7 - np.sqrt(x * x + 0.8 * y * y + 1.3 * z * z)).astype(np.float32) + np.float32(0.5)


def at_level(res, level):
    """noise with every 7th sample of the cropped grid exactly float32(level): coincident crossings, t = 0 and t = 1.  (Counted
    in the cropped grid: every 7th sample of a 7^3 volume lies in its plane x = 0, which marching cubes never reads.)"""
    v = noise(res, 7000 + res)
    crop = v[1:, 1:, 1:].copy()
    crop.reshape(-1)[::7] = np.float32(level)
    v[1:, 1:, 1:] = crop
    return v


def border(res):
    """inside (0.6 .. 1) everywhere except the outer shell of the cropped grid (0 .. 0.3): the surface runs through the last
    cube of every row, column and plane - the cells next to the points whose corner strides both classify kernels clamp"""
    rs = np.random.RandomState(9000 + res)
    v = (0.6 + 0.4 * rs.random_sample((res, res, res))).astype(np.float32)
    out = (0.3 * rs.random_sample((res, res, res))).astype(np.float32)
    shell = np.ones((res, res, res), bool)
    shell[2:res - 1, 2:res - 1, 2:res - 1] = False          # cropped indices 1 .. n - 2 are the interior
    v[shell] = out[shell]
    return v


def slab_sparse(res):
    """an ellipsoid confined to the middle third of z: some slab ranges hold nothing"""
    z, y, x = np.meshgrid(*([np.linspace(-1, 1, res)] * 3), indexing="ij")
    return (0.3 - np.sqrt(0.5 * x * x + 0.4 * y * y + 1.0 * z * z)).astype(np.float32) + np.float32(0.5)


def case(kind, res, level_id):
    """-> (volume, level) of one named case; ``level`` is what the caller hands to the library (a Python float)"""
    lv = 0.37 if level_id == "0.37" else 0.5
    if kind == "noise":
        vol = noise(res, 997 + res)                            # (res 3 is ONE cube: this seed's is cut at all three levels)
    elif kind == "at_level":
        vol = at_level(res, lv)
    elif kind == "border":
        vol = border(res)
    else:
        raise ValueError(kind)
    if level_id == "0.0":
        return vol - np.float32(0.5), 0.0
    return vol, lv


def f32_level(level):
    """the level as the library receives it (a c_float): 0.37 is not a float32"""
    return float(np.float32(level))


# ---------------------------------------------------------------------------------------------
# what a case contains (conditions the CPU tests assert, so that a GPU test cannot pass on an empty case)
# ---------------------------------------------------------------------------------------------
def config_index(vol, level):
    """[n-1, n-1, n-1] cube configurations of the cropped grid (Bourke's corner numbering on the array axes), bit = inside"""
    s = np.asarray(vol, np.float32)[1:, 1:, 1:] > np.float32(level)
    n0, n1, n2 = s.shape
    idx = np.zeros((n0 - 1, n1 - 1, n2 - 1), np.int64)
    for m, (dx, dy, dz) in enumerate(mc_classic.CORNERS):
        idx |= s[dx:n0 - 1 + dx, dy:n1 - 1 + dy, dz:n2 - 1 + dz].astype(np.int64) << m
    return idx


def crossed_edges(vol, level):
    """-> {array axis (0 = z, 1 = y, 2 = x): bool array over the lattice edges of the cropped grid along that axis, indexed by
    the edge's lower end point (z, y, x)}: True where the end points lie on different sides (inside = value > level)"""
    ins = np.asarray(vol, np.float32)[1:, 1:, 1:] > np.float32(level)
    out = {}
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        out[ax] = ins[tuple(lo)] != ins[tuple(hi)]
    return out


def layer_crossings(vol, level):
    """per z layer of the cropped grid: the number of crossed edges whose lower end point lies in it (x, y and z edges)"""
    c = crossed_edges(vol, level)
    n = vol.shape[0] - 1
    per = np.zeros(n, np.int64)
    per += c[1].reshape(n, -1).sum(1) + c[2].reshape(n, -1).sum(1)
    per[: n - 1] += c[0].reshape(n - 1, -1).sum(1)
    return per


# ---------------------------------------------------------------------------------------------
# the independent reference and the comparison
# ---------------------------------------------------------------------------------------------
def classic_mesh(vol, level, blocks=False):
    """oracle/mc_classic.py on vol[1:,1:,1:] as PyMCubes reads the array, after the reference's own [:, [2,1,0]] / [:, [0,2,1]]
    (seg3d_lossless.py:594-596) -> (verts [Nv,3] float64 (x, y, z), faces [Nf,3])"""
    sub = np.ascontiguousarray(np.asarray(vol, np.float32)[1:, 1:, 1:])
    if blocks:
        cv, cf = mc_classic.marching_cubes_blocks(sub, f32_level(level), set_below=True, block=64)
    else:
        cv, cf = mc_classic.marching_cubes(sub, f32_level(level), set_below=True)
    return cv[:, [2, 1, 0]], cf[:, [0, 2, 1]]


def vertex_bound(res):
    """what a float32 implementation may differ by from the float64 reference, in voxels: the coordinate x + t is one float32
    rounding of a value <= res - 2 (half an ulp of the largest coordinate: 2^(floor(log2(res - 2)) - 24)), and t is three
    correctly rounded float32 operations on a value in [0, 1] (difference, difference, quotient: 3 x 2^-24 and the second-order
    terms, allowed as 4 x 2^-24)"""
    cmax = max(res - 2, 1)
    return 2.0 ** (math.floor(math.log2(cmax)) - 24) + 4 * 2.0 ** -24


def _canonical_rows(ids):
    """the lexicographically smallest rotation of every triangle: winding kept"""
    ids = np.asarray(ids, np.int64)
    rots = np.stack([ids, ids[:, [1, 2, 0]], ids[:, [2, 0, 1]]], 1)
    m = int(ids.max()) + 2 if ids.size else 2
    key = (rots[..., 0] * m + rots[..., 1]) * m + rots[..., 2]
    return rots[np.arange(len(ids)), np.argmin(key, axis=1)]


def compare_with_classic(v, f, cv, cf, bound):
    """(a float32 mesh, the classic float64 mesh) -> dict.  Reference vertices that ``bound`` cannot tell apart are one PLACE:
    the same position (a sample exactly at the level puts the crossings of up to six edges on its lattice point) or positions
    within 2 x bound of each other, chained (a sample a few float32 steps off the level puts them NEXT to the lattice point);
    every vertex of ours is assigned the place of the nearest reference position (max-norm).  ``same_vertex_set``: equal
    counts, every vertex within ``bound`` of that position, every place taken as often as the reference takes it.  Triangles
    as triples of places, rotation-free, winding kept, compared as multisets: ``only_ours`` / ``only_theirs`` / ``flipped`` (a
    triangle with two corners in one place has no winding and equals its mirror image).  ``place_extent``: the largest
    max-norm extent of a place - places are what they are meant to be, the crossings around ONE lattice point, while it stays
    far below a voxel (a condition on the CASE, asserted by the callers: <= 16 x bound)."""
    from scipy.spatial import cKDTree
    v = np.asarray(v, np.float64).reshape(-1, 3)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    cv = np.asarray(cv, np.float64).reshape(-1, 3)
    cf = np.asarray(cf, np.int64).reshape(-1, 3)
    out = {"verts": (len(v), len(cv)), "faces": (len(f), len(cf)), "bound": bound}
    if len(v) == 0 or len(cv) == 0:
        out.update(same_vertex_set=len(v) == len(cv), max_vertex_diff=0.0, place_extent=0.0,
                   only_ours=len(f), only_theirs=len(cf), flipped=0)
        return out
    from scipy.sparse import coo_matrix, csgraph
    pos, pinv = np.unique(cv, axis=0, return_inverse=True)
    tree = cKDTree(pos)
    pairs = tree.query_pairs(2 * bound, p=np.inf, output_type="ndarray")
    _, label = csgraph.connected_components(coo_matrix((np.ones(len(pairs), bool), (pairs[:, 0], pairs[:, 1])), shape=(len(pos), len(pos))),
                                            directed=False)
    label = label.astype(np.int64)
    nplace = int(label.max()) + 1
    cinv = label[pinv.reshape(-1)]
    lo, hi = np.full((nplace, 3), np.inf), np.full((nplace, 3), -np.inf)
    np.minimum.at(lo, label, pos)
    np.maximum.at(hi, label, pos)
    out["place_extent"] = float((hi - lo).max())
    dist, near = tree.query(v, k=1, p=np.inf)
    near = label[near]
    out["max_vertex_diff"] = float(dist.max())
    out["same_vertex_set"] = bool(len(v) == len(cv) and dist.max() <= bound and
                                  np.array_equal(np.bincount(near, minlength=nplace), np.bincount(cinv, minlength=nplace)))
    ra, rb = _canonical_rows(near[f]), _canonical_rows(cinv[cf])
    pack = lambda r: np.sort((r[:, 0] * nplace + r[:, 1]) * nplace + r[:, 2])      # nplace^3 < 2^63 up to 2 M places
    if nplace < 2_000_000 and np.array_equal(pack(ra), pack(rb)):
        out.update(only_ours=0, only_theirs=0, flipped=0)     # the same multiset: nothing to list
        return out
    ta, tb = Counter(map(tuple, ra.tolist())), Counter(map(tuple, rb.tolist()))
    oa, ob = ta - tb, tb - ta
    flipped = 0
    for (a, b, c), k in oa.items():
        mirror = tuple(_canonical_rows(np.array([[a, c, b]], np.int64))[0].tolist())
        flipped += min(k, ob.get(mirror, 0))
    out.update(only_ours=sum(oa.values()) - flipped, only_theirs=sum(ob.values()) - flipped, flipped=flipped)
    return out


def assert_same_as_classic(c):
    """the assertions of both test files on a compare_with_classic result"""
    assert c["place_extent"] <= 16 * c["bound"], c            # the case, not the code under test: a place is one lattice point's
    assert c["verts"][0] == c["verts"][1] and c["faces"][0] == c["faces"][1], c
    assert c["same_vertex_set"], c
    assert c["only_ours"] == 0 and c["only_theirs"] == 0 and c["flipped"] == 0, c
    assert c["max_vertex_diff"] <= c["bound"], c


def plane_cuts(res, k):
    """every way to cut the planes 0 .. res - 1 into k + 1 non-empty parts: tuples (0, c1, ..., ck, res)"""
    from itertools import combinations
    return [(0,) + c + (res,) for c in combinations(range(1, res), k)]

"""The voxeliser's test cases (tests/test_vox_reference.py on the CPU, tests/test_gpu_voxelize.py on the GPU) and their float64
references (tests/vox_reference.py), built once per session.

A case is a dict: verts [V,3] f32 (the first n_surface are the surface vertices), n_surface, table [V,3] f32 (the code table
padded to V rows with huge values: only the first n_surface rows are the voxeliser's), tets [T,4] i64, exact (every float32
operation on it is exact at the case's resolution: the reference runs two-way)."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import batch_pamir as bp
import vox_reference as vr

HUGE = np.float32(1e30)
UNDECIDED_CAP = 0.005             # of the reference's occupied voxels; a condition on the inputs, checked before any result is read


def _case(verts, n_surface, tets, seed, exact=False):
    verts = np.ascontiguousarray(verts, np.float32)
    table = np.full((len(verts), 3), HUGE, np.float32)
    table[:n_surface] = np.random.RandomState(seed).uniform(0.0, 1.0, (n_surface, 3))
    return dict(verts=verts, n_surface=int(n_surface), table=table, tets=np.ascontiguousarray(tets, np.int64), exact=exact)


@lru_cache(maxsize=None)
def body():
    vv, tets, code = bp.tetra_body()
    return dict(verts=vv, n_surface=len(code), table=np.concatenate([code, np.full((len(vv) - len(code), 3), HUGE, np.float32)]),
                tets=tets, exact=False)


def random_tets(n, seed, lo=0.1, hi=0.4):
    """[n,4,3] f64: seeded tetrahedra with every edge length in [lo, hi], inside the cube, both orientations as they fall"""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        P = rng.uniform(-0.42, 0.42, 3) + rng.uniform(-0.2, 0.2, (4, 3))
        e = np.linalg.norm(P[:, None] - P[None], axis=-1)[np.triu_indices(4, 1)]
        if e.min() >= lo and e.max() <= hi and np.abs(P).max() < 0.5:
            out.append(P)
    return np.stack(out)


def orientation(c):
    """the sign of every tetrahedron's volume (float64), 0 where an index is out of range"""
    P = c["verts"].astype(np.float64)
    t = c["tets"]
    ok = ((t >= 0) & (t < len(P))).all(1)
    Q = P[np.where(ok[:, None], t, 0)]
    return np.where(ok, np.sign(np.linalg.det(Q[:, 1:] - Q[:, :1])), 0.0)


@lru_cache(maxsize=None)
def mixed(n=200, seed=7, n_surface=300):
    """n random tetrahedra; the surface vertices are the first n_surface of their 4 n vertices"""
    P = random_tets(n, seed)
    return _case(P.reshape(-1, 3), n_surface, np.arange(4 * n).reshape(n, 4), seed + 1)


@lru_cache(maxsize=None)
def mirrored():
    b = body()
    return dict(b, tets=np.ascontiguousarray(b["tets"][:, [0, 1, 3, 2]]))


LATTICE_RES = 16


@lru_cache(maxsize=None)
def lattice(n=150, seed=11):
    """vertex coordinates on multiples of 1/32: at res 16 every centre (odd multiples of 1/32), difference and product of three
    is exact in float32 (integers below 2^17 over 2^15), so the inside test has no rounding at all"""
    rng = np.random.RandomState(seed)
    P = np.clip(rng.randint(-12, 13, (n, 1, 3)) + rng.randint(-6, 7, (n, 4, 3)), -16, 16) / 32.0
    c = _case(P.reshape(-1, 3), 4 * n - 50, np.arange(4 * n).reshape(n, 4), seed + 1, exact=True)
    assert np.array_equal(c["verts"].astype(np.float64) * 32, np.round(c["verts"].astype(np.float64) * 32))
    return c


def boundary_hits(c, res):
    """(tetrahedron, voxel) pairs with the centre exactly on a face, edge or vertex of a tetrahedron of non-zero volume"""
    s, ok = vr.dense_signed(c["verts"], c["tets"], res)
    return int(((s >= 0).all(-1) & (s == 0).any(-1) & ok[:, None]).sum())


@lru_cache(maxsize=None)
def clamps(big=False):
    """tetrahedra straddling each of the six faces of the [-0.5,0.5]^3 cube, one wholly outside on either side, and (big) one
    that contains the whole cube"""
    base = random_tets(8, 23, lo=0.15, hi=0.4)
    P = []
    for k in range(3):
        for side in (-1.0, 1.0):
            T = base[len(P)].copy()
            T[:, k] += side * 0.5 - T[:, k].mean()                     # centred on the face: vertices on both sides of it
            assert T[:, k].min() < side * 0.5 < T[:, k].max()
            P.append(T)
    P.append(base[6] - base[6].mean(0) + [0.9, 0.8, 0.85])             # wholly outside, + side
    P.append(base[7] - base[7].mean(0) - [0.9, 0.75, 0.8])             # wholly outside, - side
    assert (P[6] > 0.5).all() and (P[7] < -0.5).all()
    if big:
        P.append(np.array([[-1.0, -1, -1], [5, -1, -1], [-1, 5, -1], [-1, -1, 5]]))   # x, y, z >= -1 and x + y + z <= 3
    P = np.stack(P)
    return _case(P.reshape(-1, 3), 20, np.arange(4 * len(P)).reshape(len(P), 4), 29)


@lru_cache(maxsize=None)
def skipped(valid_only=False):
    """valid rows interleaved with rows the voxeliser skips: an index of -1, V, 2^40, and the three kinds of zero-volume row
    (a repeated vertex, four coplanar vertices, all four equal).  The zero-volume rows use extra vertices on multiples of 1/32 in
    the plane z = 3/32, so that their volume is zero in any arithmetic (and no centre of res 20 or 33 lies in that plane)."""
    n = 60
    P = random_tets(n, 31).reshape(-1, 3)
    flat = np.array([[-8, -8, 3], [8, -6, 3], [-4, 10, 3], [6, 7, 3], [0, 0, 3]]) / 32.0
    verts = np.concatenate([P, flat])
    V, L = len(verts), 4 * n
    good = np.arange(4 * n).reshape(n, 4)
    bad = np.array([[-1, 1, 2, 3], [4, V, 6, 7], [8, 9, 2 ** 40, 11], [12, 13, 14, -2 ** 40], [V + 5, V, V, V],
                    [L, L + 1, L + 1, L + 2], [L, L, L + 1, L + 2], [L + 3, L + 1, L + 2, L + 1],        # a repeated vertex
                    [L, L + 1, L + 2, L + 3], [L + 4, L + 2, L + 1, L],                                  # four coplanar
                    [L + 4, L + 4, L + 4, L + 4], [5, 5, 5, 5], [0, 0, 0, 0]], np.int64)                 # all equal
    rows, g = [], 0
    for i, b in enumerate(bad):
        rows += [b] + list(good[g:g + 4 + i % 3])
        g += 4 + i % 3
    rows += list(good[g:])
    tets = good if valid_only else np.stack(rows)
    assert valid_only or len(tets) == n + len(bad)
    return _case(verts, 150, tets, 37)


TILE_SURFACES = (1, 255, 256, 257, 513)


@lru_cache(maxsize=None)
def tiles(n_surface):
    """n_surface surface vertices (scattered points: the Gaussian average does not ask them to belong to a tetrahedron), then
    the interior ones that 60 tetrahedra use; the rows of the code table past n_surface are huge"""
    rng = np.random.RandomState(41)
    surf = rng.uniform(-0.5, 0.5, (TILE_SURFACES[-1], 3))[:n_surface]
    P = random_tets(60, 43).reshape(-1, 3)
    return _case(np.concatenate([surf, P]), n_surface, n_surface + np.arange(240).reshape(60, 4), 47 + n_surface)


def subject(verts):
    """the body's tetrahedra and codes on another subject's vertices (tests/batch_pamir.py)"""
    return dict(body(), verts=np.ascontiguousarray(verts, np.float32))


CASES = {"body": body, "mirrored": mirrored, "mixed": mixed, "lattice": lattice, "clamps": clamps, "clamps_big": lambda: clamps(True),
         "skipped": skipped, "skipped_valid": lambda: skipped(True), **{f"tiles{n}": (lambda n=n: tiles(n)) for n in TILE_SURFACES}}


def get(name):
    if name.startswith("subject"):                          # subject<b>of<B>
        b, B = map(int, name[7:].split("of"))
        return subject(bp.subjects(B)["verts"][b])
    return CASES[name]()


@lru_cache(maxsize=None)
def reference(name, res, sigma=0.05):
    """(values [R,R,R,3] f64, sure_in, undecided) of a case, read-only"""
    c = get(name)
    out = vr.reference(c["verts"], c["n_surface"], c["table"], c["tets"], res, sigma, exact=c["exact"])
    for a in out:
        a.setflags(write=False)
    return out


def check_cap(name, res, sigma=0.05):
    """the reference of a case, after the condition on its inputs: undecided voxels <= 0.5 % of the occupied ones (none if exact)"""
    values, sure_in, und = reference(name, res, sigma)
    n_in, n_und = int(sure_in.sum()), int(und.sum())
    print(f"{name} res {res}: reference occupied {n_in}, undecided {n_und}")
    assert n_und <= (0 if get(name)["exact"] else UNDECIDED_CAP * n_in), (name, res, n_in, n_und)
    return values, sure_in, und


def compare(name, res, sigma, got, occ, tol):
    """the acceptance of one volume: got [R,R,R,3] f32 and its occupancy [R,R,R] (0 / 1) against the case's reference.  Returns
    the largest value difference."""
    values, sure_in, und = check_cap(name, res, sigma)
    occ = np.asarray(occ).astype(bool)
    dec = ~und
    bad = int((occ[dec] != sure_in[dec]).sum())
    assert bad == 0, f"{name} res {res}: occupancy differs from the reference at {bad} decided voxels, first (z,y,x) {np.argwhere((occ != sure_in) & dec)[:5].tolist()}"
    assert not np.isnan(got).any()
    assert (got[~occ] == 0.0).all(), f"{name} res {res}: an outside voxel is not exactly 0"
    err = float(np.abs(got[occ] - values[occ]).max()) if occ.any() else 0.0     # undecided voxels taken inside: the average there
    print(f"{name} res {res} sigma {sigma}: max |value - reference| = {err:.3e} over {int(occ.sum())} occupied voxels")
    assert err <= tol, f"{name} res {res} sigma {sigma}: max |value - reference| = {err:.3e} > {tol}"
    return err

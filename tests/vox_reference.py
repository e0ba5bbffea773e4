"""An independent float64 statement of the PaMIR semantic voxeliser (icon_semantic_voxelize / _batch, oracle orc_semantic_voxelize),
written from the definition in the header of icon_amd/csrc/vox_kernels.hip and sharing no expression with either:

  voxel (z,y,x) has centre p = ((x,y,z) + 0.5) / R - 0.5;  occ = p lies in or on at least one tetrahedron whose four
  indices name existing vertices and whose volume is not zero;
  out[z][y][x] = occ * sum_v w_v code_v / (1e-3 + sum_v w_v),  w_v = exp(-|p - v|^2 / (2 sigma^2)) over the first V_surf vertices.

Inside test.  For each of the four faces of a tetrahedron (the face opposite vertex l is the other three vertices, in index
order, origin the first): n = (P_j - P_i) x (P_k - P_i), g_l(p) = n . p - n . P_i, h_l = n . (P_l - P_i).  p is inside or on the
tetrahedron iff for every face it lies on the side of the opposite vertex or on the face: s_l = g_l(p) * sign(h_l) >= 0.  No
orientation convention, no face list with a global sign, no float32 and no float32 bounding box: the candidates of a tetrahedron
are the voxels whose float64 centre lies in its float64 min/max widened by one voxel; all (tetrahedron, candidate) pairs are
evaluated, a few million at a time.

Three-way answer.  The code under test evaluates its determinants in float32; a voxel whose centre is closer to a face than
that evaluation can resolve may go either way.  Every s comes with a forward bound tau for a float32 evaluation of the same
determinant: edges and offset taken from the face's first vertex, cross product of the edges, dot product with the offset, in
any order of the additions and with or without fma (u = 2^-24).  The origin is part of the statement: for the needle-shaped
tetrahedra of the body (13,776 surface triangles joined to one interior vertex) an evaluation from the far vertex would have a
bound many times larger.

  tau = u * (C_ROUND * sum|terms| + sum_k |n_k|^ e_k)

  sum|terms|: the six products |e1_a e2_b w_c| of the expanded determinant (the permanent of the absolute edge / offset
      components).
  C_ROUND = 9: a term passes through at most 8 roundings - 3 subtractions (e1, e2, w = p - origin), the rounded product and the
      rounded difference of the cross product (with or without fma), the product with w, and 2 additions of the dot product;
      (1 + u)^8 - 1 < 8.000001 u, and one more unit covers that, the float64 evaluation here and |terms| being taken from exact
      rather than rounded components.  Counted, not tuned.
  the second summand: a float32 centre.  For R a power of two (x + 0.5) / R - 0.5 is exact however it is evaluated: e_k = 0.
      Otherwise, with q = (x + 0.5) / R = p + 0.5, a rounded reciprocal and a rounded product (or one rounded division) leave
      |q^ - q| <= 2 u q, and the subtraction of 0.5 is exact for q^ in [1/4, 1] (Sterbenz) and rounds by at most u |p| below:
      e_k = 2 q_k + |p_k| [q_k < 1/4] in units of u.  It moves s by at most |n_k|^ e_k, |n_k|^ the two absolute products of n_k.

  sure inside: some tetrahedron has all four s > tau;   sure outside: every tetrahedron has some s < -tau;   undecided: the rest.

A tetrahedron whose own volume is within its bound of zero (|h_l| <= tau for some l) may be skipped or taken with either
orientation by a float32 evaluation: it makes no voxel sure inside, and a candidate is sure outside of it only when two of its
g_l differ in sign beyond their bounds after the orientation pattern of the face enumeration (read off the unit simplex by the
same code, not written down) is taken out.  If every term of its volume is zero (a vertex repeated in the right slots, all
equal) it is skipped for sure.  With exact=True (inputs for which every float32 and float64 operation is exact: `lattice`) tau = 0:
the answer is two-way, a zero volume is skipped, and no voxel may be exempt.

Gaussian average: float64 throughout from the float32 inputs (sigma is the float32 the C ABI receives), exact centres.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
C_ROUND = 9.0
CHUNK = 1 << 21                                             # (tetrahedron, candidate) pairs evaluated at a time
_OTHERS = ((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2))      # the face opposite vertex l: the other three, in index order


def centres(res: int) -> np.ndarray:
    return (np.arange(res, dtype=np.float64) + 0.5) / res - 0.5


def _perm(a, b, w):
    """sum of the six |products| of det[a; b; w] for absolute component arrays [..., 3]"""
    return (a[..., 0] * (b[..., 1] * w[..., 2] + b[..., 2] * w[..., 1]) + a[..., 1] * (b[..., 0] * w[..., 2] + b[..., 2] * w[..., 0])
            + a[..., 2] * (b[..., 0] * w[..., 1] + b[..., 1] * w[..., 0]))


def _faces(P):
    """P [T,4,3] -> normals [T,4,3], offsets n . origin [T,4], h [T,4]"""
    n = np.stack([np.cross(P[:, j] - P[:, i], P[:, k] - P[:, i]) for (i, j, k) in _OTHERS], 1)
    off = np.stack([(n[:, l] * P[:, i]).sum(-1) for l, (i, j, k) in enumerate(_OTHERS)], 1)
    h = np.stack([(n[:, l] * (P[:, l] - P[:, i])).sum(-1) for l, (i, j, k) in enumerate(_OTHERS)], 1)
    return n, off, h


_PATTERN = np.sign(_faces(np.array([[[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]]))[2][0])     # the signs of h_l in one orientation


def _centre_error(pts, res):
    """per axis, in units of u: the distance of a float32 centre from the exact one"""
    if res & (res - 1) == 0:
        return np.zeros_like(pts)
    q = pts + 0.5
    return 2.0 * q + np.abs(pts) * (q < 0.25)


def _tau(P, pts, res):
    """the bounds [M,4] of s_l for tetrahedra P [M,4,3] at the points pts [M,3]"""
    err = _centre_error(pts, res)
    out = np.empty((len(pts), 4))
    for l, (i, j, k) in enumerate(_OTHERS):
        a, b = np.abs(P[:, j] - P[:, i]), np.abs(P[:, k] - P[:, i])
        nabs = np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)
        out[:, l] = C_ROUND * _perm(a, b, np.abs(pts - P[:, i])) + (err * nabs).sum(-1)
    return U * out


def _tau_volume(P):
    """[T]: the bound of the tetrahedron's own determinant, the largest of the four h_l"""
    best = np.zeros(len(P))
    for l, (i, j, k) in enumerate(_OTHERS):
        best = np.maximum(best, _perm(np.abs(P[:, j] - P[:, i]), np.abs(P[:, k] - P[:, i]), np.abs(P[:, l] - P[:, i])))
    return U * C_ROUND * best


def dense_signed(verts, tets, res: int):
    """every voxel against every tetrahedron, for small cases: s [T,R^3,4] (voxels in flat (z,y,x) order) and ok [T], the rows
    whose indices exist and whose h_l are all non-zero"""
    P_all = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    tets = np.asarray(tets, np.int64).reshape(-1, 4)
    ok = ((tets >= 0) & (tets < len(P_all))).all(1)
    n, off, h = _faces(P_all[np.where(ok[:, None], tets, 0)].reshape(-1, 4, 3))
    c = centres(res)
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    pts = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1)
    s = np.sign(h)[:, None, :] * (np.einsum("tlk,nk->tnl", n, pts) - off[:, None, :])
    return s, ok & (h != 0.0).all(1)


def occupancy(verts, tets, res: int, exact: bool = False):
    """(sure_in, undecided) [R,R,R] bool, indexed (z,y,x)"""
    P_all = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    tets = np.asarray(tets, np.int64).reshape(-1, 4)
    c = centres(res)
    step = 1.0 / res
    n_vox = res ** 3
    sure_in = np.zeros(n_vox, bool)
    maybe = np.zeros(n_vox, bool)                           # not sure outside of some tetrahedron
    tets = tets[((tets >= 0) & (tets < len(P_all))).all(1)]
    P = P_all[tets].reshape(-1, 4, 3)
    n, off, h = _faces(P)
    tv = np.zeros(len(P)) if exact else _tau_volume(P)
    keep = (h != 0.0).all(1) if exact else ~((tv == 0.0) & (h == 0.0).all(1))
    unsure = (np.abs(h) <= tv[:, None]).any(1) & keep & (not exact)
    sign = np.where(unsure[:, None], _PATTERN[None, :], np.sign(h))
    mn, mx = P.min(1), P.max(1)
    lo = np.stack([np.searchsorted(c, mn[:, k] - step, "left") for k in range(3)], 1)       # (x, y, z) index ranges: centres
    hi = np.stack([np.searchsorted(c, mx[:, k] + step, "right") for k in range(3)], 1)      # within [mn - step, mx + step]
    dims = np.maximum(hi - lo, 0)
    cnt = np.where(keep, dims.prod(1), 0)
    D = mx - mn
    E = D + step
    pair = D[:, [1, 0, 0]] * D[:, [2, 2, 1]]
    cheap = np.zeros(len(P)) if exact else U * (C_ROUND * 2.0 * (pair * E).sum(1) + 3.0 * 2.0 * pair.sum(1))   # >= every tau in the box
    sgn = [np.ascontiguousarray(sign[:, l]) for l in range(4)]
    nrm = [[np.ascontiguousarray(n[:, l, k]) for k in range(3)] for l in range(4)]
    offs = [np.ascontiguousarray(off[:, l]) for l in range(4)]
    order = np.nonzero(cnt)[0]
    ends = np.cumsum(cnt[order])
    a = 0
    while a < len(order):
        b = max(a + 1, int(np.searchsorted(ends, (ends[a - 1] if a else 0) + CHUNK, "right")))
        ids = order[a:b]
        a = b
        k = cnt[ids]
        tid = np.repeat(ids, k)
        loc = np.arange(k.sum()) - np.repeat(np.cumsum(k) - k, k)
        nx, ny = dims[tid, 0], dims[tid, 1]
        x, y, z = lo[tid, 0] + loc % nx, lo[tid, 1] + (loc // nx) % ny, lo[tid, 2] + loc // (nx * ny)
        flat = (z * res + y) * res + x
        px, py, pz = c[x], c[y], c[z]
        ch, un = cheap[tid], unsure[tid]
        cols = []
        for l in range(4):                                  # face by face, dropping the pairs a face already puts outside for sure
            sl = sgn[l][tid] * (nrm[l][0][tid] * px + nrm[l][1][tid] * py + nrm[l][2][tid] * pz - offs[l][tid])
            cols.append(sl)
            go = (sl >= -ch) | un
            if not go.all():
                tid, flat, px, py, pz, ch, un = tid[go], flat[go], px[go], py[go], pz[go], ch[go], un[go]
                cols = [col[go] for col in cols]
        s = np.stack(cols, 1)
        if exact:
            sure_in[flat[(s >= 0.0).all(1)]] = True
            continue
        smin = s.min(1)
        sure_in[flat[(smin > ch) & ~un]] = True
        close = np.where(un, ~((smin < -ch) & (s.max(1) > ch)), np.abs(smin) <= ch)
        if not close.any():
            continue
        tid, flat, s, un = tid[close], flat[close], s[close], un[close]
        tau = _tau(P[tid], np.stack([px[close], py[close], pz[close]], 1), res)
        inn = (s > tau).all(1) & ~un
        out = np.where(un, (s < -tau).any(1) & (s > tau).any(1), (s < -tau).any(1))
        sure_in[flat[inn]] = True
        maybe[flat[~inn & ~out]] = True
    shape = (res, res, res)
    return sure_in.reshape(shape), (maybe & ~sure_in).reshape(shape)


def gaussian_average(verts, n_surface: int, code, res: int, sigma: float, flat) -> np.ndarray:
    """[len(flat), 3] float64: the Gaussian-weighted average of the surface codes at the voxels with flat (z,y,x) index `flat`"""
    Vs = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)[:n_surface]
    code = np.asarray(code, np.float32).astype(np.float64).reshape(-1, 3)[:n_surface]
    k2 = 1.0 / (2.0 * float(np.float32(sigma)) ** 2)
    c = centres(res)
    flat = np.asarray(flat, np.int64)
    out = np.empty((len(flat), 3))
    rows = max(1, (1 << 22) // max(1, len(Vs)))
    for a in range(0, len(flat), rows):
        f = flat[a:a + rows]
        d2 = ((c[f % res][:, None] - Vs[None, :, 0]) ** 2 + (c[(f // res) % res][:, None] - Vs[None, :, 1]) ** 2
              + (c[f // (res * res)][:, None] - Vs[None, :, 2]) ** 2)
        w = np.exp(-d2 * k2)
        out[a:a + rows] = (w @ code) / (1e-3 + w.sum(1))[:, None]
    return out


def reference(verts, n_surface: int, code, tets, res: int, sigma: float, exact: bool = False):
    """(values [R,R,R,3] float64, sure_in [R,R,R] bool, undecided [R,R,R] bool).  values holds the Gaussian average at every
    sure-inside and undecided voxel (an undecided voxel the code under test leaves outside must be exactly 0 there instead) and
    0 elsewhere."""
    sure_in, undecided = occupancy(verts, tets, res, exact)
    values = np.zeros((res ** 3, 3))
    flat = np.nonzero((sure_in | undecided).reshape(-1))[0]
    values[flat] = gaussian_average(verts, n_surface, code, res, sigma, flat)
    return values.reshape(res, res, res, 3), sure_in, undecided

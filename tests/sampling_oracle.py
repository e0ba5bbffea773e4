"""numpy float64 statement of the training sampler's rule: what ``PIFuDataset.get_sampling_geo``
(lib/dataset/PIFuDataset.py:483-607, ``is_sdf=False``) computes, with the generator, the order of the draws and the permutation
stated so that a device lane can reproduce any of them from (seed, stream, index) alone.

Two entry points: ``draws`` - the Philox draws; ``assemble`` - the rule applied to GIVEN draws (numpy's own, recorded from a run of
the reference, in tests/test_sampling.py; ``draws``' in tests/test_gpu_sampling.py).  The inside test is injected.
"""
import numpy as np

STREAM_VERTEX, STREAM_OFFSET, STREAM_SPACE, STREAM_ZNOISE, STREAM_PERM = 0, 1, 2, 3, 4
Z_SCALE, Z_THICKNESS = 0.40, 0.5          # PIFuDataset.py:529-538
FEISTEL_ROUNDS = 4
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


# ---- the generator ---------------------------------------------------------------------------------------------------------

def philox4x32(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11): ``ctr`` four and ``key`` two uint32 words (scalars or arrays) -> four uint32 arrays"""
    c = [np.asarray(x, dtype=np.uint64) & _U32 for x in ctr]
    k = [np.asarray(x, dtype=np.uint64) & _U32 for x in key]
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _U32]
        k = [(k[0] + np.uint64(_W0)) & _U32, (k[1] + np.uint64(_W1)) & _U32]
    return [x.astype(np.uint32) for x in c]


def philox(seed, index, stream):
    """key = the 64-bit seed, counter = (index low, index high, stream, 0) -> two uint64 words (x0 = words 0 | 1 << 32, x1 = 2 | 3 << 32)"""
    seed = int(seed) & (2 ** 64 - 1)
    index = np.asarray(index, dtype=np.uint64)
    o = philox4x32([index & _U32, index >> np.uint64(32), np.uint64(stream), np.uint64(0)], [seed & 0xFFFFFFFF, seed >> 32])
    o = [x.astype(np.uint64) for x in o]
    return o[0] | (o[1] << np.uint64(32)), o[2] | (o[3] << np.uint64(32))


def uniform(x):
    """((x >> 11) + 0.5) * 2^-53 in float64 (the sum rounds to even above 2^52: the value lies in (0, 1])"""
    return ((x >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def normal(x0, x1):
    """Box-Muller, the cosine branch: sqrt(-2 ln u(x0)) * cos(2 pi * u(x1))"""
    return np.sqrt(-2.0 * np.log(uniform(x0))) * np.cos(6.283185307179586 * uniform(x1))


def mulhi(x, m):
    """floor(x * m / 2^64) for uint64 x and 0 < m < 2^31"""
    m = np.uint64(m)
    return (((x >> np.uint64(32)) * m + (((x & _U32) * m) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


def feistel_bits(n):
    """the smallest even bit width (at least 2) whose range covers [0, n)"""
    b = 2
    while (1 << b) < n:
        b += 2
    return b


def perm(seed, n):
    """the keyed bijection of [0, n): FEISTEL_ROUNDS rounds (L, R) -> (R, L ^ F_r(R)) over ``feistel_bits(n)`` bits, F_r(R) = the low
    half-width bits of word 0 of philox(seed, index = r << 32 | R, STREAM_PERM); a value >= n walks on through the same network"""
    h = np.uint64(feistel_bits(n) // 2)
    mask = (np.uint64(1) << h) - np.uint64(1)
    out = np.arange(n, dtype=np.uint64)
    todo = np.arange(n)
    while todo.size:
        x = out[todo]
        left, right = x >> h, x & mask
        for r in range(FEISTEL_ROUNDS):
            f = philox(seed, (np.uint64(r) << np.uint64(32)) | right, STREAM_PERM)[0] & mask
            left, right = right, left ^ f
        x = (left << h) | right
        out[todo] = x
        todo = todo[x >= np.uint64(n)]
    return out.astype(np.int64)


# ---- the rule --------------------------------------------------------------------------------------------------------------

def source_counts(N, zray, R):
    """-> (nS, nU, nZ, n) in the reference's concatenation order: surface, space, z-ray"""
    nS, nU = 4 * N, N // 4
    nZ = nS * R if zray else 0
    return nS, nU, nZ, nS + nU + nZ


def draws(seed, V, N, sigma_geo, zray, R):
    """-> dict(ids int64 [nS], offsets f64 [nS] (sigma_geo * normal), u f64 [nU,3], znoise f64 [nZ] (0.40 * normal), perm int64 [n])"""
    nS, nU, nZ, n = source_counts(N, zray, R)
    ids = mulhi(philox(seed, np.arange(nS), STREAM_VERTEX)[0], V)
    offsets = float(sigma_geo) * normal(*philox(seed, np.arange(nS), STREAM_OFFSET))
    u = uniform(philox(seed, np.arange(3 * nU), STREAM_SPACE)[0]).reshape(nU, 3)
    znoise = Z_SCALE * normal(*philox(seed, np.arange(nZ), STREAM_ZNOISE))
    return dict(ids=ids, offsets=offsets, u=u, znoise=znoise, perm=perm(seed, n))


def project(points, m):
    """rows of float64 ``points [k,3]`` through the affine ``m`` (at least [3,4]): ((m0 x + m1 y) + m2 z) + t per row"""
    x, y, z = points[:, 0:1], points[:, 1:2], points[:, 2:3]
    return ((m[None, :3, 0] * x + m[None, :3, 1] * y) + m[None, :3, 2] * z) + m[None, :3, 3]


def sources(verts, normals, calib, calib_inv, ids, offsets, u, znoise, R):
    """the float64 samples in source order [n,3]; ``znoise`` empty: no z-ray samples"""
    verts, normals = np.asarray(verts, dtype=np.float64), np.asarray(normals, dtype=np.float64)
    calib, calib_inv = np.asarray(calib, dtype=np.float64), np.asarray(calib_inv, dtype=np.float64)
    surface = verts[ids] + normals[ids] * np.asarray(offsets, dtype=np.float64).reshape(-1, 1)
    space = project(2.0 * np.asarray(u, dtype=np.float64).reshape(-1, 3) - 1.0, calib_inv)
    parts = [surface, space]
    if len(znoise):
        cube = np.repeat(project(surface, calib), R, axis=0)
        cube[:, 2] = cube[:, 2] + Z_THICKNESS * np.asarray(znoise, dtype=np.float64)
        parts.append(project(cube, calib_inv))
    return np.concatenate(parts, 0)


def balance(all_samples, inside, N):
    """the truncation of PIFuDataset.py:562-599 on the shuffled list -> (samples f32 [N,3], labels f32 [N], counts int [2]); rows
    past counts.sum() are zero"""
    inside = np.asarray(inside, dtype=bool)
    ins, outs = all_samples[inside], all_samples[~inside]
    if len(ins) > N // 2:
        ins, outs = ins[:N // 2], outs[:N // 2]
    else:
        outs = outs[:N - len(ins)]
    samples, labels = np.zeros((N, 3), np.float32), np.zeros(N, np.float32)
    samples[:len(ins)], samples[len(ins):len(ins) + len(outs)] = ins, outs
    labels[:len(ins)] = 1.0
    return samples, labels, np.array([len(ins), len(outs)], dtype=np.int64)


def assemble(verts, normals, calib, ids, offsets, u, znoise, perm, inside_fn, N, R=1, calib_inv=None):
    """the rule applied to given draws -> dict(all_samples f32 [n,3] (slot i = source perm[i]), inside bool [n], source int64 [n]
    (0 surface, 1 space, 2 z-ray), samples, labels, counts).  ``inside_fn``: float32 [k,3] -> bool [k]."""
    calib = np.asarray(calib, dtype=np.float64)
    if calib_inv is None:
        full = np.eye(4)
        full[:3] = calib[:3]
        calib_inv = np.linalg.inv(full)
    src = sources(verts, normals, calib, calib_inv, ids, offsets, u, znoise, R)
    perm = np.asarray(perm, dtype=np.int64)
    all_samples = np.ascontiguousarray(src[perm].astype(np.float32))
    nS, nU = len(ids), len(np.asarray(u).reshape(-1, 3))
    source = (perm >= nS).astype(np.int64) + (perm >= nS + nU)
    inside = np.asarray(inside_fn(all_samples), dtype=bool)
    samples, labels, counts = balance(all_samples, inside, N)
    return dict(all_samples=all_samples, inside=inside, source=source, samples=samples, labels=labels, counts=counts)

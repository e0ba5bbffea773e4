"""Seeded inputs shared by tests/test_garment.py (CPU: the oracle against matplotlib / sklearn / the reference) and
tests/test_gpu_garment.py (the device against the oracle).  numpy only."""
import numpy as np


def star_polygon(rng, n, r0=0.35, r1=1.0, center=(0.0, 0.0)):
    """a simple polygon of n vertices: sorted angles, random radii"""
    a = np.sort(rng.uniform(0, 2 * np.pi, n))
    r = rng.uniform(r0, r1, n)
    return np.stack([center[0] + r * np.cos(a), center[1] + r * np.sin(a)], 1)


def lattice_polygon(rng, n):
    """coordinates on the 1/8 lattice: vertices, edges and shared y values are hit exactly by lattice points"""
    return np.round(star_polygon(rng, n) * 8) / 8


def tangle_polygon(rng, n):
    """vertices in random order: self-intersecting"""
    return rng.uniform(-1, 1, (n, 2))


def mixed_points(rng, N, dtype=np.float64):
    """half on the 1/8 lattice of [-1.25, 1.25]^2, half anywhere"""
    lat = rng.randint(-10, 11, (N // 2, 2)) / 8.0
    free = rng.uniform(-1.25, 1.25, (N - N // 2, 2))
    return np.concatenate([lat, free]).astype(dtype)


def cloud(rng, V, lattice=False):
    """V float32 vertices in [-1.25, 1.25]^2 x [-0.3, 0.3]; lattice: half of the (x, y) on the 1/8 lattice"""
    xy = mixed_points(rng, V, np.float32) if lattice else rng.uniform(-1.25, 1.25, (V, 2)).astype(np.float32)
    rng.shuffle(xy)
    return np.concatenate([xy, rng.uniform(-0.3, 0.3, (V, 1)).astype(np.float32)], 1)


def faces_covering(rng, V, F):
    """F faces over V vertices; when F >= V every vertex is named by a face (face i starts at vertex i)"""
    f = rng.randint(0, V, (F, 3))
    k = min(V, F)
    f[:k, 0] = np.arange(k)
    return f.astype(np.int64)


def source(rng, verts, Vs):
    """Vs float32 source vertices scattered around the cloud, and a byte per source vertex: about 40 % are 'removed'"""
    lo, hi = verts.min(0) - 0.1, verts.max(0) + 0.1
    src = rng.uniform(lo, hi, (Vs, 3)).astype(np.float32)
    return src, (rng.uniform(size=Vs) < 0.4)


def not_vacuous(o, with_source=True):
    """the three conditions every non-degenerate case must meet on the ORACLE's side"""
    frac = o["selected"].mean()
    assert 0.05 <= frac <= 0.95, f"{100 * frac:.1f} % of the vertices selected"
    if with_source:
        assert (o["selected"] & ~o["keep_v"]).any(), "no selected vertex is removed by its label"
    assert o["keep_v"].any(), "no selected vertex is kept"

"""The training sampler's rule on the CPU: tests/sampling_oracle.py against a recorded run of the reference's
own get_sampling_geo (tests/golden/sampling_geo_ref.npz, written by tests/make_sampling_golden.py), the generator against its
published vectors and its moments, the permutation, and the balancing's edge cases.  The device side is tests/test_gpu_sampling.py."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [p for p in (HERE, ROOT) if p not in sys.path]

import sampling_oracle as so  # noqa: E402
from icon_amd import synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "sampling_geo_ref.npz")

# a calibration as the loader holds it (float32 entries): a scale into the image cube, y flipped, a small rotation, a shift
_c, _s = np.float32(np.cos(0.2)), np.float32(np.sin(0.2))
CALIB = np.array([[_c / 128, 0, _s / 128, 0.03125], [0, -1 / 128, 0, 0.0625], [-_s / 128, 0, _c / 128, -0.015625], [0, 0, 0, 1]],
                 dtype=np.float32).astype(np.float64)
# the same without the rotation: every product and sum of a float32 projection is exact whatever the order of operations
CALIB_EXACT = np.array([[1 / 128, 0, 0, 0.03125], [0, -1 / 128, 0, 0.0625], [0, 0, 1 / 128, -0.015625], [0, 0, 0, 1]], dtype=np.float64)

# the recorded runs: scan, N, sigma_geo, zray_type, ray_sample_num, is_valid, numpy seed
CASES = {
    "ico": ("ico", 64, 5.0, False, 1, False, 11),
    "ico_z2": ("ico", 64, 5.0, True, 2, False, 12),
    "ico_z1": ("ico", 64, 5.0, True, 1, False, 13),
    "ico_valid": ("ico", 64, 5.0, True, 2, True, 14),
    "small_sparse": ("small", 64, 20.0, False, 1, False, 15),         # few inside samples: the second balancing branch
    "body": ("body", 2000, 5.0, False, 1, False, 16),
    "body_z1": ("body", 2000, 5.0, True, 1, False, 17),
}

_scans = {}


def scan(name):
    """-> (verts f32 [V,3], faces int64 [F,3], vert_normals f32 [V,3]) in a scan's units (about 100 per metre)"""
    if name not in _scans:
        if name == "ico":
            v, f = synth.icosphere(2, radius=60.0, center=(3.0, -2.0, 1.0))
        elif name == "small":
            v, f = synth.icosphere(2, radius=2.0, center=(3.0, -2.0, 1.0))
        elif name == "odd":                                            # V = 642: not a multiple of 64
            v, f = synth.icosphere(3, radius=45.0, center=(-1.0, 4.0, 2.0))
        else:
            v, f = synth.load_body_mesh()
            v = (v * np.float32(100.0)).astype(np.float32)
        _scans[name] = (v, f, orc.vertex_normals(v, f))
    return _scans[name]


def inside_fn(name):
    v, f, _ = scan(name)
    return lambda pts: orc.check_sign(v, f, np.ascontiguousarray(pts, dtype=np.float32))


def ulp_distance(a, b):
    """float32 arrays -> the distance in units in the last place, as int64"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---- the reference, loaded from where it lies (only tests/make_sampling_golden.py needs it) -----------------------------------

class _Anything(types.ModuleType):
    """a module that has every name: what the reference's loader imports and get_sampling_geo never touches"""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


_STAND_INS = ["lib", "lib.renderer", "lib.renderer.mesh", "lib.dataset", "lib.dataset.hoppeMesh", "lib.dataset.body_model", "lib.common",
              "lib.common.render", "lib.dataset.mesh_util", "lib.pare", "lib.pare.pare", "lib.pare.pare.utils",
              "lib.pare.pare.utils.geometry", "termcolor", "PIL", "trimesh", "vedo", "kaolin", "kaolin.ops", "kaolin.ops.mesh",
              "torchvision", "torchvision.transforms", "ipdb"]


def load_reference():
    """the reference's PIFuDataset.get_sampling_geo, its module imported from the reference tree with stand-ins for what it imports
    (its own ``projection`` is taken from lib/dataset/mesh_util.py); None where the tree is absent"""
    import ast
    from oracle import ref_loader
    root = ref_loader.REFERENCE_ROOT
    path, util = os.path.join(root, "lib", "dataset", "PIFuDataset.py"), os.path.join(root, "lib", "dataset", "mesh_util.py")
    if not (os.path.isfile(path) and os.path.isfile(util)):
        return None
    import torch
    with open(util) as fh:
        tree = ast.parse(fh.read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "projection"]
    scope = {"np": np, "torch": torch}
    exec(compile(ast.Module(body=fn, type_ignores=[]), util, "exec"), scope)
    saved = {k: sys.modules.get(k) for k in _STAND_INS}
    for k in _STAND_INS:
        sys.modules[k] = _Anything(k)
    sys.modules["lib.dataset.mesh_util"].projection = scope["projection"]
    try:
        spec = importlib.util.spec_from_file_location("_reference_pifu_dataset", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, m in saved.items():
            if m is None:
                del sys.modules[k]
            else:
                sys.modules[k] = m
    return mod.PIFuDataset.get_sampling_geo


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


# ---- against the recorded run of the reference ---------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_rule_matches_reference_run(golden, case):
    """assemble() fed numpy's own recorded draws gives the reference's samples_geo / labels_geo: labels and row order exactly, the
    coordinates within 1 float32 ulp (the reference rounds its float64 once; its matrix products sum in the BLAS's order)"""
    name, N, sigma, zray, R, is_valid, _ = CASES[case]
    g = {k[len(case) + 1:]: golden[k] for k in golden.files if k.startswith(case + ".")}
    v, f, vn = scan(name)
    Z = zray and not is_valid
    assert len(g["znoise"]) == (4 * N * R if Z else 0)
    out = so.assemble(v, vn, CALIB, g["ids"], g["offsets"], g["u"], g["znoise"], g["perm"], inside_fn(name), N, R)
    assert np.array_equal(out["inside"], g["inside_all"].astype(bool))
    m = int(out["counts"].sum())
    assert m == len(g["labels"]) and g["samples"].shape == (m, 3)
    assert np.array_equal(out["labels"][:m], g["labels"])
    assert int(ulp_distance(out["samples"][:m], g["samples"]).max()) <= 1
    n_in = int(g["inside_all"].sum())
    assert (n_in > N // 2) == (case != "small_sparse"), "the cases cover both balancing branches"
    assert tuple(out["counts"]) == ((N // 2, N // 2) if n_in > N // 2 else (n_in, N - n_in))


def test_golden_covers_the_issue(golden):
    assert {CASES[c][0] for c in CASES} >= {"ico", "body"} and {CASES[c][1] for c in CASES} == {64, 2000}
    assert {(CASES[c][3] and not CASES[c][5], CASES[c][4]) for c in CASES} >= {(False, 1), (True, 1), (True, 2)}
    assert any(CASES[c][5] for c in CASES)
    assert all(f"{c}.samples" in golden.files for c in CASES)


# ---- the permutation ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 4095, 4096, 4097, 34000, 66000])
def test_perm_is_a_bijection(n):
    for seed in (0, 1, 0xDEADBEEF, 2 ** 64 - 1):
        p = so.perm(seed, n)
        assert p.shape == (n,) and np.array_equal(np.sort(p), np.arange(n))
    if n >= 64:
        assert not np.array_equal(so.perm(1, n), so.perm(2, n))
        assert (so.perm(1, n) == np.arange(n)).mean() < 0.1


def test_perm_width():
    assert [so.feistel_bits(n) for n in (1, 4, 5, 16, 17, 4096, 4097, 66000, 2 ** 31 - 1)] == [2, 2, 4, 4, 6, 12, 14, 18, 32]
    for n in (1, 5, 4097, 66000):                                      # the range is below 4 n: fewer than four expected walks
        assert (1 << so.feistel_bits(n)) < 4 * max(n, 2)


# ---- the generator -----------------------------------------------------------------------------------------------------------

def test_philox_known_answers():
    """the known-answer vectors of Random123 (kat_vectors: philox4x32 10)"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(x) for x in so.philox4x32(ctr, key)) == want
    x0, x1 = so.philox(0x299f31d0a4093822, np.array([0x85a308d3243f6a88], dtype=np.uint64), 0x13198a2e)
    o = so.philox4x32((0x243f6a88, 0x85a308d3, 0x13198a2e, 0), (0xa4093822, 0x299f31d0))
    assert int(x0[0]) == int(o[0]) | int(o[1]) << 32 and int(x1[0]) == int(o[2]) | int(o[3]) << 32


def test_integer_and_uniform_maps():
    x = np.array([0, 1, 2 ** 63, 2 ** 64 - 1, 0x123456789ABCDEF0], dtype=np.uint64)
    for m in (1, 162, 6890, 2 ** 31 - 1):
        assert so.mulhi(x, m).tolist() == [(int(v) * m) >> 64 for v in x]
    u = so.uniform(x)
    assert u[0] == 0.5 * 2.0 ** -53 and u[3] == 1.0 and u[2] == (2.0 ** 52 + 0.5) * 2.0 ** -53 and (u > 0).all()


def test_stream_moments():
    """5 sigma bounds from the sample size: mean and variance of the uniform and the normal stream, their lag-1 correlation, the
    vertex ids' mean; streams of two seeds differ"""
    n = 200_000
    idx = np.arange(n)
    for seed in (3, 2 ** 40 + 7):
        u = so.uniform(so.philox(seed, idx, so.STREAM_SPACE)[0])
        assert abs(u.mean() - 0.5) <= 5 * np.sqrt(1 / 12 / n)
        assert abs(((u - 0.5) ** 2).mean() - 1 / 12) <= 5 * np.sqrt(1 / 180 / n)
        assert abs(((u[1:] - 0.5) * (u[:-1] - 0.5)).mean()) <= 5 * (1 / 12) / np.sqrt(n)
        g = so.normal(*so.philox(seed, idx, so.STREAM_OFFSET))
        assert abs(g.mean()) <= 5 / np.sqrt(n)
        assert abs((g * g).mean() - 1.0) <= 5 * np.sqrt(2 / n)
        assert abs((g ** 4).mean() - 3.0) <= 5 * np.sqrt(96 / n)
        assert abs((g[1:] * g[:-1]).mean()) <= 5 / np.sqrt(n)
        ids = so.mulhi(so.philox(seed, idx, so.STREAM_VERTEX)[0], 6890)
        assert ids.min() >= 0 and ids.max() < 6890
        assert abs(ids.mean() - 6889 / 2) <= 5 * np.sqrt((6890 ** 2 - 1) / 12 / n)
    assert not np.array_equal(so.philox(3, idx[:8], 0)[0], so.philox(4, idx[:8], 0)[0])
    assert not np.array_equal(so.philox(3, idx[:8], 0)[0], so.philox(3, idx[:8], 1)[0])


def test_draws_shapes_and_scales():
    d = so.draws(5, 162, 64, 5.0, True, 2)
    assert d["ids"].shape == (256,) and d["offsets"].shape == (256,) and d["u"].shape == (16, 3) and d["znoise"].shape == (512,) and d["perm"].shape == (784,)
    e = so.draws(5, 162, 64, 10.0, False, 2)
    assert np.array_equal(e["ids"], d["ids"]) and np.array_equal(e["offsets"], 2.0 * d["offsets"]) and e["znoise"].shape == (0,) and e["perm"].shape == (272,)


# ---- the balancing's edge cases ----------------------------------------------------------------------------------------------

def _balance_case(flags, N):
    flags = np.asarray(flags, dtype=bool)
    pts = np.arange(3 * len(flags), dtype=np.float32).reshape(-1, 3) + 1
    s, l, c = so.balance(pts, flags, N)
    k = int(c.sum())
    assert s.shape == (N, 3) and l.shape == (N,) and (s[k:] == 0).all() and (l[k:] == 0).all()
    assert (l[:c[0]] == 1).all() and (l[c[0]:k] == 0).all()
    assert np.array_equal(s[:c[0]], pts[flags][:c[0]]) and np.array_equal(s[c[0]:k], pts[~flags][:c[1]])
    return tuple(int(x) for x in c)


def test_balance_edge_cases():
    rng = np.random.RandomState(5)
    N, n = 64, 272
    assert _balance_case(np.zeros(n), N) == (0, 64)                                        # n_in = 0
    assert _balance_case(np.ones(n), N) == (32, 0)                                         # all inside: the outside samples run short
    for n_in, want in ((32, (32, 32)), (33, (32, 32)), (31, (31, 33)), (270, (32, 2))):    # N // 2 exactly, N // 2 + 1, short outside
        flags = np.zeros(n, bool)
        flags[rng.permutation(n)[:n_in]] = True
        assert _balance_case(flags, N) == want
    flags = rng.rand(4 * 7 + 1) < 0.5                                                      # odd N: N // 2 = 3, N // 4 = 1
    assert int(flags.sum()) > 3 and _balance_case(flags, 7) == (3, 3)
    assert _balance_case(flags & (np.arange(29) < 4), 7) == (int(flags[:4].sum()), 7 - int(flags[:4].sum()))
    for N in (1, 2, 3):                                                                    # N < 4: no space samples
        assert so.source_counts(N, True, 2) == (4 * N, 0, 8 * N, 12 * N)
        assert _balance_case(np.arange(4 * N) % 2 == 0, N) == (N // 2, N // 2)
        assert _balance_case(np.zeros(4 * N), N) == (0, N)


def test_assemble_small_n_and_source_order():
    """N < 4 end to end, and the concatenation order: surface, space, z-ray"""
    v, f, vn = scan("ico")
    for N, zray, R in ((1, True, 2), (3, False, 1), (5, True, 1)):
        nS, nU, nZ, n = so.source_counts(N, zray, R)
        d = so.draws(9, len(v), N, 5.0, zray, R)
        out = so.assemble(v, vn, CALIB, d["ids"], d["offsets"], d["u"], d["znoise"], d["perm"], inside_fn("ico"), N, R)
        assert out["all_samples"].shape == (n, 3) and np.bincount(out["source"], minlength=3).tolist() == [nS, nU, nZ]
        src = so.sources(v, vn, CALIB, np.linalg.inv(CALIB), d["ids"], d["offsets"], d["u"], d["znoise"], R)
        assert np.array_equal(src[:nS], v[d["ids"]].astype(np.float64) + vn[d["ids"]].astype(np.float64) * d["offsets"][:, None])
        cube = so.project(src[nS:nS + nU], CALIB)
        assert cube.shape == (nU, 3) and (np.abs(cube) <= 1 + 1e-9).all() and np.allclose(cube, 2 * d["u"] - 1, atol=1e-12)
        if zray:                                                      # a z-ray sample differs from its surface sample along the cube's z only
            a, b = so.project(src[nS + nU:], CALIB), np.repeat(so.project(src[:nS], CALIB), R, axis=0)
            assert np.allclose(a[:, :2], b[:, :2], atol=1e-9) and np.allclose(a[:, 2] - b[:, 2], 0.5 * d["znoise"], atol=1e-9)


# ---- how far the device's libm may move a coordinate ---------------------------------------------------------------------------

# the device runs of tests/test_gpu_sampling.py: scan, N, sigma_geo, zray, R, seed
GPU_CASES = {
    "tiny": ("ico", 8, 5.0, False, 1, 101),
    "ico_z2": ("ico", 64, 5.0, True, 2, 102),
    "odd_z1": ("odd", 64, 5.0, True, 1, 103),
    "body": ("body", 2000, 5.0, False, 1, 104),
    "body_z1": ("body", 2000, 5.0, True, 1, 105),
    "shipped": ("body", 8000, 5.0, True, 1, 106),
}
COORD_DIFF_CAP = 1e-4          # at most one coordinate in 10,000 may differ at all (and by 1 float32 ulp)


@pytest.mark.parametrize("case", list(GPU_CASES))
def test_last_bits_stay_inside_the_cap(case):
    """log, cos and sqrt of another libm differ by a few float64 ulps: the oracle against itself with both normal streams moved by
    up to 8 float64 ulps keeps every float32 coordinate within 1 ulp and all but one in 10,000 equal - the bound the device is held to"""
    name, N, sigma, zray, R, seed = GPU_CASES[case]
    v, f, vn = scan(name)
    d = so.draws(seed, len(v), N, sigma, zray, R)
    inv = np.linalg.inv(CALIB)
    a = so.sources(v, vn, CALIB, inv, d["ids"], d["offsets"], d["u"], d["znoise"], R).astype(np.float32)
    rng = np.random.RandomState(seed)
    wiggle = lambda x: x * (1.0 + rng.randint(-8, 9, size=x.shape) * 2.0 ** -52)
    b = so.sources(v, vn, CALIB, inv, d["ids"], wiggle(d["offsets"]), d["u"], wiggle(d["znoise"]), R).astype(np.float32)
    dist = ulp_distance(a, b)
    assert int(dist.max()) <= 1 and (dist != 0).sum() <= int(COORD_DIFF_CAP * dist.size)

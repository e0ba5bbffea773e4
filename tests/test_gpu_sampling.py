"""icon_amd.sampling on the device - ScanMesh / sample_geo_device / GeoSampler / smpl_signs_device over icon_sample_geo
(csrc/sample_geo.hip) - against the numpy statement of the rule (tests/sampling_oracle.py; DESIGN.md 4.21, pinned to a recorded
run of the reference by tests/test_sampling.py).

What is an integer is held to EQUALITY: the vertex ids, the permutation, the inside flags (oracle.check_sign on the device's own
float32 samples), the balanced output given the device's own shuffled list.  The coordinates pass through log, cos and sqrt of the
device's libm: within 1 float32 ulp, and at most one in 10,000 different at all (test_sampling.test_last_bits_stay_inside_the_cap).

Shapes: N = 8 (n = 34, less than a wavefront), N = 64 with z-rays (n = 784 and 528: several workgroups, a ragged last one, a V
that is no multiple of 64), N = 2000 (n = 8,500 / 16,500: two and three rounds of the balancing scan) for the statistics, and the
shipped N = 8000 with z-rays once (n = 66,000: nine rounds)."""
import numpy as np
import pytest
import torch

import sampling_oracle as so
import test_sampling as ts
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


_scan_cache, _run_cache = {}, {}


def dev_scan(name):
    from icon_amd.sampling import ScanMesh
    if name not in _scan_cache:
        v, f, vn = ts.scan(name)
        _scan_cache[name] = ScanMesh(_dev(v), _dev(f), _dev(vn))
    return _scan_cache[name]


def run(name, N, sigma, zray, R, seed, calib=None):
    """one device call with return_all, copied to the host, and the oracle's draws for it: computed once, shared, left unchanged"""
    from icon_amd.sampling import sample_geo_device
    key = (name, N, sigma, zray, R, seed, calib is None)
    if key not in _run_cache:
        s, l, c, extra = sample_geo_device(dev_scan(name), ts.CALIB if calib is None else calib, N, sigma, zray_type=zray, ray_sample_num=R,
                                           seed=seed, return_all=True)
        assert s.dtype == torch.float32 and l.dtype == torch.float32 and c.dtype == torch.int32 and s.is_cuda and s.shape == (N, 3) and l.shape == (N,)
        out = dict(samples=s.cpu().numpy(), labels=l.cpu().numpy(), counts=c.cpu().numpy(), **{k: t.cpu().numpy() for k, t in extra.items()})
        out["draws"] = so.draws(seed, dev_scan(name).V, N, sigma, zray, R)
        _run_cache[key] = out
    return _run_cache[key]


def case_run(case):
    return run(*ts.GPU_CASES[case])


@pytest.mark.parametrize("case", list(ts.GPU_CASES))
def test_integers_equal_the_oracle(case):
    name, N, sigma, zray, R, seed = ts.GPU_CASES[case]
    r, d = case_run(case), case_run(case)["draws"]
    nS, nU, nZ, n = so.source_counts(N, zray, R)
    assert r["source"].shape == (n,) and np.array_equal(r["source"], d["perm"])
    src = d["perm"]
    want = np.where(src < nS, d["ids"][np.minimum(src, nS - 1)], -1)
    if nZ:
        want = np.where(src >= nS + nU, d["ids"][np.clip(src - nS - nU, 0, nZ - 1) // R], want)
    assert np.array_equal(r["vertex"], want)
    assert np.bincount((src >= nS).astype(int) + (src >= nS + nU), minlength=3).tolist() == [nS, nU, nZ]


@pytest.mark.parametrize("case", list(ts.GPU_CASES))
def test_coordinates_within_one_ulp(case):
    name, N, sigma, zray, R, seed = ts.GPU_CASES[case]
    r = case_run(case)
    d = r["draws"]
    v, f, vn = ts.scan(name)
    want = so.sources(v, vn, ts.CALIB, np.linalg.inv(ts.CALIB), d["ids"], d["offsets"], d["u"], d["znoise"], R)[d["perm"]].astype(np.float32)
    dist = ts.ulp_distance(r["all_samples"], want)
    print(f"{case}: {int((dist != 0).sum())} of {dist.size} coordinates differ, at most {int(dist.max())} ulp")
    assert int(dist.max()) <= 1
    assert int((dist != 0).sum()) <= int(ts.COORD_DIFF_CAP * dist.size)


@pytest.mark.parametrize("case", list(ts.GPU_CASES))
def test_inside_flags(case):
    """the labels' rule on the device's own float32 samples: oracle.check_sign, and the library's sdf_query"""
    name = ts.GPU_CASES[case][0]
    r = case_run(case)
    assert np.array_equal(r["all_inside"], ts.inside_fn(name)(r["all_samples"]))
    assert 0.05 < r["all_inside"].mean() < 0.95
    q = dev_scan(name).handle.sdf_query(_dev(r["all_samples"]))["inside"]
    assert np.array_equal(q.cpu().numpy(), r["all_inside"])


def _balanced(r, N):
    s, l, c = so.balance(r["all_samples"], r["all_inside"], N)
    assert np.array_equal(r["counts"], c)
    assert r["samples"].tobytes() == s.tobytes() and r["labels"].tobytes() == l.tobytes()
    return int(r["all_inside"].sum()), tuple(int(x) for x in c)


@pytest.mark.parametrize("case", list(ts.GPU_CASES))
def test_final_output(case):
    N = ts.GPU_CASES[case][1]
    n_in, c = _balanced(case_run(case), N)
    assert n_in > N // 2 and c == (N // 2, N // 2)


def test_final_output_few_inside():
    """a small sphere with a large sigma_geo: n_in <= N // 2, every inside sample is kept; then a tiny sigma_geo: the first branch"""
    n_in, c = _balanced(run("small", 64, 20.0, False, 1, 201), 64)
    assert 0 < n_in <= 32 and c == (n_in, 64 - n_in)
    n_in, c = _balanced(run("small", 64, 20.0, True, 2, 202), 64)
    assert 0 < n_in <= 32 and c == (n_in, 64 - n_in)
    n_in, c = _balanced(run("small", 64, 0.01, False, 1, 203), 64)
    assert n_in > 32 and c == (32, 32)


def test_final_output_short_outside():
    """the outside samples run short: a scan most of whose vertices lie loose inside it (no face names them), a tiny sigma_geo and a
    calibration whose cube lies inside the scan - counts sum below N and the rows past them are zero"""
    from icon_amd.sampling import ScanMesh, sample_geo_device
    v, f, vn = ts.scan("ico")
    rng = np.random.RandomState(3)
    loose = (np.array([3.0, -2.0, 1.0]) + rng.uniform(-8, 8, (4000, 3))).astype(np.float32)
    verts = np.concatenate([v, loose])
    normals = np.concatenate([vn, np.tile(np.float32([0, 1, 0]), (4000, 1))])
    calib = ts.CALIB_EXACT.copy()
    calib[:3] *= 8.0                                                   # the cube is +-16 units around (-4, 8, 2)
    scan = ScanMesh(_dev(verts), _dev(f), _dev(normals))
    N = 64
    s, l, c, extra = sample_geo_device(scan, calib, N, 0.01, seed=301, return_all=True)
    r = dict(samples=s.cpu().numpy(), labels=l.cpu().numpy(), counts=c.cpu().numpy(), all_samples=extra["all_samples"].cpu().numpy(),
             all_inside=extra["all_inside"].cpu().numpy())
    assert np.array_equal(r["all_inside"], orc.check_sign(v, f, r["all_samples"]))
    n_in, c = _balanced(r, N)
    n_out = len(r["all_inside"]) - n_in
    assert 0 < n_out < N // 2 and c == (N // 2, n_out)
    assert (r["samples"][sum(c):] == 0).all() and (r["labels"][sum(c):] == 0).all() and (r["labels"][:32] == 1).all()


@pytest.mark.parametrize("case", ["body", "body_z1"])
def test_statistics_against_the_reference_run(case):
    """N = 2000: the inside share of the shuffled list against the reference's own run of the same settings (another generator,
    the same distribution): two binomial shares, 5 sigma of their difference; and the surface-source slots in the first half of
    the list against the hypergeometric expectation of a uniform shuffle"""
    name, N, sigma, zray, R, seed = ts.GPU_CASES[case]
    assert ts.CASES[case][:5] == (name, N, sigma, zray, R)
    r = case_run(case)
    ref = np.load(ts.GOLDEN)[f"{case}.inside_all"]
    n = len(ref)
    assert len(r["all_inside"]) == n
    p_dev, p_ref = r["all_inside"].mean(), ref.mean()
    p = 0.5 * (p_dev + p_ref)
    print(f"{case}: inside share {p_dev:.4f} (device) / {p_ref:.4f} (reference run), bound {5 * np.sqrt(2 * p * (1 - p) / n):.4f}")
    assert abs(p_dev - p_ref) <= 5 * np.sqrt(2 * p * (1 - p) / n)
    nS = 4 * N
    m = n // 2
    got = int((r["source"][:m] < nS).sum())
    mean, var = m * nS / n, m * (nS / n) * (1 - nS / n) * (n - m) / (n - 1)
    print(f"{case}: {got} surface slots in the first {m}, expected {mean:.1f} +- {np.sqrt(var):.1f}")
    assert abs(got - mean) <= 5 * np.sqrt(var)


def test_determinism_seed_and_stream():
    from icon_amd.sampling import sample_geo_device
    scan = dev_scan("ico")
    call = lambda seed: sample_geo_device(scan, ts.CALIB, 64, 5.0, zray_type=True, ray_sample_num=2, seed=seed)
    a, b, other = call(102), call(102), call(103)
    ref = case_run("ico_z2")
    for x, y, key in zip(a, b, ("samples", "labels", "counts")):
        assert torch.equal(x, y) and x.cpu().numpy().tobytes() == ref[key].tobytes()
    assert not torch.equal(a[0], other[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = call(102)
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    assert all(torch.equal(x, y) for x, y in zip(a, call(102 + 2 ** 64)))          # the seed is taken modulo 2^64


def test_faces_dtype_and_own_normals():
    from icon_amd.sampling import ScanMesh, sample_geo_device
    v, f, vn = ts.scan("odd")
    ref = case_run("odd_z1")
    for faces, normals in ((_dev(f).to(torch.int32), _dev(vn)), (_dev(f), None)):
        scan = ScanMesh(_dev(v), faces, normals)
        if normals is None:                                           # the handle's S1 normals are the oracle's
            assert np.array_equal(scan.vert_normals.cpu().numpy(), vn)
        s, l, c = sample_geo_device(scan, ts.CALIB, 64, 5.0, zray_type=True, ray_sample_num=1, seed=103)
        assert s.cpu().numpy().tobytes() == ref["samples"].tobytes() and l.cpu().numpy().tobytes() == ref["labels"].tobytes()


def test_is_valid_disables_zray_and_geo_sampler():
    from icon_amd.sampling import GeoSampler, sample_geo_device
    scan = dev_scan("ico")
    plain = sample_geo_device(scan, ts.CALIB, 64, 5.0, seed=7, return_all=True)
    valid = sample_geo_device(scan, ts.CALIB, 64, 5.0, zray_type=True, ray_sample_num=2, is_valid=True, seed=7, return_all=True)
    assert valid[3]["all_samples"].shape == (272, 3) and all(torch.equal(x, y) for x, y in zip(plain[:3], valid[:3]))
    sampler = GeoSampler(dict(num_sample_geo=64, sigma_geo=5.0, zray_type=True, ray_sample_num=2))
    out = sampler.get_sampling_geo(dict(mesh=scan, calib=torch.from_numpy(ts.CALIB).float()), is_valid=True, seed=7)
    assert set(out) == {"samples_geo", "labels_geo"} and torch.equal(out["samples_geo"], plain[0]) and torch.equal(out["labels_geo"], plain[1])
    out = sampler.get_sampling_geo(dict(mesh=scan, calib=ts.CALIB), seed=102)
    ref = case_run("ico_z2")
    assert out["samples_geo"].cpu().numpy().tobytes() == ref["samples"].tobytes() and out["labels_geo"].shape == (64,)
    few = GeoSampler(dict(num_sample_geo=64, sigma_geo=20.0)).get_sampling_geo(dict(mesh=dev_scan("small"), calib=ts.CALIB), seed=201)
    assert few["samples_geo"].shape == (64, 3) and 0 < int(few["labels_geo"].sum()) <= 32


def test_bad_arguments_raise():
    from icon_amd._lib import IconAmdError
    from icon_amd.sampling import GeoSampler, ScanMesh, sample_geo_device, smpl_signs_device
    scan = dev_scan("ico")
    v, f, vn = ts.scan("ico")
    with pytest.raises(IconAmdError):
        GeoSampler(dict(num_sample_geo=64, sigma_geo=5.0)).get_sampling_geo(dict(mesh=scan, calib=ts.CALIB), is_sdf=True, seed=1)
    with pytest.raises(IconAmdError):
        ScanMesh(torch.from_numpy(v), _dev(f))                         # a host tensor
    with pytest.raises(IconAmdError):
        ScanMesh(_dev(v), _dev(f), torch.from_numpy(vn))
    for N in (0, -3):
        with pytest.raises(IconAmdError):
            sample_geo_device(scan, ts.CALIB, N, 5.0, seed=1)
    with pytest.raises(IconAmdError):
        sample_geo_device(scan, ts.CALIB, 64, 5.0, zray_type=True, ray_sample_num=0, seed=1)
    with pytest.raises(IconAmdError):
        sample_geo_device(scan, np.zeros((4, 4)), 64, 5.0, seed=1)     # a singular calibration
    with pytest.raises(IconAmdError):
        sample_geo_device((v, f), ts.CALIB, 64, 5.0, seed=1)
    with pytest.raises(IconAmdError):
        smpl_signs_device(scan.handle, torch.zeros(4, 3), ts.CALIB)


def test_smpl_signs():
    """pts_signs of load_smpl: the projected samples against the SMPL mesh, 2 (inside - 0.5); the calibration without a rotation
    projects float32 samples exactly, so the oracle sees the very points the device tests"""
    from icon_amd import synth
    from icon_amd.engine import MeshHandle
    from icon_amd.sampling import smpl_signs_device
    sv, sf = synth.icosphere(2)
    V = len(sv)
    smpl = MeshHandle(_dev(sv), _dev(sf), torch.zeros((V, 3), device="cuda"), torch.zeros(V, device="cuda"))
    r = run("ico", 64, 5.0, True, 2, 102)
    m = int(r["counts"].sum())
    pts = r["samples"][:m]
    signs = smpl_signs_device(smpl, _dev(pts), torch.from_numpy(ts.CALIB_EXACT).float())
    proj = (pts.astype(np.float64) @ ts.CALIB_EXACT[:3, :3].T + ts.CALIB_EXACT[:3, 3]).astype(np.float32)
    want = 2.0 * (orc.check_sign(sv, sf, proj).astype(np.float32) - 0.5)
    assert signs.dtype == torch.float32 and signs.shape == (m,) and np.array_equal(signs.cpu().numpy(), want)
    assert (want > 0).any() and (want < 0).any()

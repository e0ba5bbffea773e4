"""GPU tests of the one-call coarse-to-fine schedule (icon_adaptive_eval, csrc/adaptive.hip) with the pamir and pifu priors.

A level of the schedule launches the fused MLP kernel with N = r^3, an upper bound; the real count lives on the device.  These
priors run the non-SMALL kernel, whose launcher may hand part of every span to a pool of tiles drawn at run time
(icon_work_set_steal): the tests compare the native schedule with the host-driven one (AdaptiveReconEngine.native = False, whose
queries carry their count on the host) under several partitions, pin the examined levels to the float64 oracle, and check that
the settings examined do reach the regime where a pool sized from the bound and spans cut from the real count disagree
(tests/test_host.py::test_fused_kernel_tile_partition_with_device_side_count restates it on the host)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from common import assets, orc, vol_assets
from test_gpu_parity import T, dev, make_engine

pytestmark = pytest.mark.gpu

OCC_TOL = 1e-4
RES = [33, 65, 129, 257]
# (permille, group, reserved CUs): all static, the default, a static run one tile short of the span, everything pooled, and a
# smaller grid (another `rem` for the same counts)
STEALS = [(0, 1, 0), (150, 2, 0), (40, 1, 0), (1000, 1, 0), (40, 1, 16)]
TILE = 256                                       # points per tile of the non-SMALL kernel (kTilePts)


def bits(t):
    return t.contiguous().view(torch.int32)


def vol_engine(prior, sd, vol):
    from icon_amd.engine import IconQueryEngine
    eng = IconQueryEngine(prior_type=prior)
    if vol is not None:
        eng.set_volume_features(T(vol))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in sd.items()})
    return eng


def recon(res_list, query_func=None):
    from icon_amd.engine import query_func as qf
    from icon_amd.recon import AdaptiveReconEngine
    return AdaptiveReconEngine(query_func=query_func or qf, b_min=[[-1.0, 1.0, -1.0]], b_max=[[1.0, -1.0, 1.0]],
                               resolutions=res_list, align_corners=True, faster=True).to(dev())


def recording(log):
    """query_func that also keeps (points [N,3], occ [N]) of every call.  functools.wraps keeps the package's __module__:
    AdaptiveReconEngine answers the coarsest level with the lattice kernels only behind the package's own query_func, as in the
    host-driven runs of tests/test_gpu_parity.py"""
    from icon_amd.engine import query_func

    @functools.wraps(query_func)
    def qf(opt, netG, features, points, proj_matrix=None):
        occ = query_func(opt, netG, features, points, proj_matrix)
        log.append((points[0].cpu().numpy().copy(), occ.reshape(-1).cpu().numpy().copy()))
        return occ
    return qf


def call_args(case):
    return dict(opt=SimpleNamespace(num_views=1), netG=case.eng, features=[case.feat], proj_matrix=None)


def make_case(prior):
    """The synthetic MLP has no sdf channel: its field is ~0.5 +- 0.05 everywhere, so the boundary band could cover all of the
    lattice or none of it.  The last layer's bias is shifted (a constant shift of the output: last_op None) so that a quarter
    of the 33^3 level lies above 0.5, from a dense evaluation at 33."""
    feat_np, vol, sd = vol_assets(prior)
    feat = T(feat_np)
    occ = vol_engine(prior, sd, vol).eval_slab(feat, 33, 0, 33).cpu().numpy().ravel()
    s = np.sort(occ)[::-1]
    k = occ.size // 4
    sd = dict(sd)
    assert "filters.3.bias" in sd and "filters.4.bias" not in sd
    sd["filters.3.bias"] = (sd["filters.3.bias"] + np.float32(0.5 - 0.5 * (float(s[k - 1]) + float(s[k])))).astype(np.float32)
    eng = vol_engine(prior, sd, vol)
    above = float((eng.eval_slab(feat, 33, 0, 33) > 0.5).float().mean())
    assert 0.10 <= above <= 0.40, above
    c = SimpleNamespace(prior=prior, eng=eng, feat=feat, feat_np=feat_np, vol=vol, sd=sd, levels=[])
    w = eng._work()
    try:
        w.set_steal(0, 1)
        w.set_reserve_cus(0)
        host = recon(RES, recording(c.levels))
        host.native = False
        c.host_vol = host(**call_args(c))
        c.host_stats = dict(host.last_stats)
        assert c.host_stats["native"] is False
        c.nat0, c.counts, c.pos = eng.adaptive_eval(feat, RES)
        c.nat0 = c.nat0.clone()
    finally:
        w.set_steal(150, 2)
        w.set_reserve_cus(0)
    assert c.host_vol is not None and c.pos, f"{prior}: nothing above 0.5 at the coarsest level"
    assert c.counts[1] > 0 and c.counts[2] > 0, c.counts
    return c


@pytest.fixture(scope="module")
def cases():
    built = {}

    def get(prior):
        if prior not in built:
            built[prior] = make_case(prior)
        return built[prior]
    return get


def pool_regime(counts, res_list, permille, group, reserve, cus):
    """levels of a schedule where launch_fused_f16x3 as it stood before the device-count rule would have pooled (its numbers
    from the bound r^3) while the kernel's device-side per is below steal_static and rem > 0: -> [(res, count, per, rem, static)]"""
    hits = []
    for l in range(1, len(res_list) - 1):
        nt_host = -(-res_list[l] ** 3 // TILE)
        grid = min(nt_host, max(cus - reserve, 1))
        per_host = nt_host // grid
        pool_len = per_host * permille // 1000
        if pool_len <= 0 or nt_host <= grid:
            continue
        per, rem = divmod(-(-counts[l] // TILE), grid)
        if per < per_host - pool_len and rem > 0:
            hits.append((res_list[l], counts[l], per, rem, per_host - pool_len))
    return hits


@pytest.mark.parametrize("steal", STEALS, ids=[f"{p}-{g}-r{r}" for p, g, r in STEALS])
@pytest.mark.parametrize("prior", ["pamir", "pifu"])
def test_native_schedule_equals_host_driven_other_priors(cases, prior, steal):
    """icon_adaptive_eval against the host-driven schedule for the pamir / pifu priors: the same points per level, the same
    volume - under every tile partition, twice (the second launch finds the ticket words as the first left them), and bit for
    bit the all-static native volume"""
    c = cases(prior)
    permille, group, reserve = steal
    w = c.eng._work()
    try:
        w.set_steal(permille, group)
        w.set_reserve_cus(reserve)
        nat = recon(RES)
        for rep in range(2):
            v = nat(**call_args(c))
            # (if native_schedule_reason ever refuses these priors, the comparison would be the host-driven form with itself)
            assert nat.last_stats.get("native") is True, nat.last_stats
            assert nat.last_stats["queries"] == c.host_stats["queries"], (nat.last_stats, c.host_stats)
            d = (v - c.host_vol).abs().max().item()
            print(f"{prior} {steal} rep {rep}: queries {nat.last_stats['queries']}, max |native - host-driven| = {d:.3e}")
            assert d <= 1e-6, f"{prior} {steal} rep {rep}: max |native - host-driven| = {d:.3e}"
            assert torch.equal(bits(v), bits(c.nat0)), (prior, steal, rep)
    finally:
        w.set_steal(150, 2)
        w.set_reserve_cus(0)


@pytest.mark.parametrize("prior", ["pamir", "pifu"])
def test_schedule_levels_reach_the_pool_regime(cases, prior):
    """the comparison above is not vacuous: the boundary band is neither empty nor the whole lattice, and for at least one
    setting of STEALS an examined level has a device-side count whose spans end before the bound's static run (the launch
    that lost `rem` tiles before launches with a device-side count were made static)"""
    c = cases(prior)
    cus = torch.cuda.get_device_properties(dev()).multi_processor_count
    hits = {s: pool_regime(c.counts, RES, *s, cus) for s in STEALS}
    print(f"{prior}: counts {c.counts}, {cus} CUs, regime hits {hits}")
    assert any(hits.values()), (c.counts, cus)
    assert all(0 < c.counts[l] < RES[l] ** 3 for l in (1, 2)), c.counts


@pytest.mark.parametrize("prior", ["pamir", "pifu"])
def test_examined_levels_vs_oracle(cases, prior):
    """the points the host-driven schedule queried at its examined levels, and their results, against the float64 oracle
    (query_vol) on a seeded sample: with the native volume equal to the host-driven one, the native levels are pinned to a
    high-precision reference too"""
    c = cases(prior)
    assert [len(p) for p, _ in c.levels] == c.host_stats["queries"][1:] and len(c.levels) == len(RES) - 2
    mlp = orc.Mlp(c.sd)
    rng = np.random.RandomState(5)
    for lvl, (pts, occ) in enumerate(c.levels, 1):
        idx = rng.choice(len(pts), min(2000, len(pts)), replace=False)
        ref, _ = orc.query_vol(c.feat_np, c.vol, mlp, pts[idx], f64=True)
        err = float(np.abs(occ[idx] - ref).max())
        print(f"{prior} level {RES[lvl]}: {len(pts)} points, max |occ - oracle| = {err:.3e} on {len(idx)}")
        assert err <= OCC_TOL, (prior, RES[lvl], err)


def test_pamir_shipped_schedule_513(cases):
    """the [33 .. 513] schedule (the reference's resolutions) for cfg 4 at the default partition: its 257 level is examined"""
    c = cases("pamir")
    res_list = RES + [513]
    nat, host = recon(res_list), recon(res_list)
    host.native = False
    v1 = nat(**call_args(c))
    assert nat.last_stats.get("native") is True, nat.last_stats
    v2 = host(**call_args(c))
    assert host.last_stats["native"] is False
    assert nat.last_stats["queries"] == host.last_stats["queries"], (nat.last_stats, host.last_stats)
    assert len(nat.last_stats["queries"]) == len(res_list) - 1
    d = (v1 - v2).abs().max().item()
    print(f"pamir 513: queries {nat.last_stats['queries']}, max |native - host-driven| = {d:.3e}")
    assert d <= 1e-6


def test_icon_schedule_launches_stay_static():
    """the icon prior's schedule levels run the SMALL kernel, which never draws from the pool: any setting gives the bits of the
    all-static one"""
    body = assets("body")
    eng = make_engine(body)
    feat = T(body.features)
    w = eng._work()
    try:
        w.set_steal(0, 1)
        want, c0, pos = eng.adaptive_eval(feat, RES)
        want = want.clone()
        assert pos and c0[1] > 0 and c0[2] > 0
        for permille, group in [(40, 1), (1000, 1)]:
            w.set_steal(permille, group)
            v, counts, _ = eng.adaptive_eval(feat, RES)
            assert counts == c0 and torch.equal(bits(v), bits(want)), (permille, group)
    finally:
        w.set_steal(150, 2)


@pytest.mark.parametrize("steal", [(150, 2), (40, 1)])
@pytest.mark.parametrize("prior", ["pamir", "pifu"])
def test_profiled_schedule_level_evaluates_every_tile(cases, prior, steal):
    """icon_work_profile covers the schedule's launches: after [65, 129, 257] the workgroup records are those of the 129 level's
    fused launch (the last one: 257 is interpolated only), and the tiles they evaluated add up to the level's count"""
    c = cases(prior)
    w = c.eng._work()
    try:
        w.set_steal(*steal)
        w.profile(True)
        _, counts, pos = c.eng.adaptive_eval(c.feat, [65, 129, 257])
        rec = w.profile_workgroups()
    finally:
        w.profile(False)
        w.set_steal(150, 2)
    assert pos and counts[1] > 0
    cus = torch.cuda.get_device_properties(dev()).multi_processor_count
    assert rec.shape[0] == min(-(-129 ** 3 // TILE), cus), rec.shape
    tiles = int(rec[:, 4].sum())
    print(f"{prior} {steal}: 129 level {counts[1]} points, {tiles} tiles evaluated by {rec.shape[0]} workgroups")
    assert tiles == -(-counts[1] // TILE), (tiles, counts)

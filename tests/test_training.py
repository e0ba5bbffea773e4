"""The training rows' rule on the CPU: tests/train_oracle.py against a recorded training-mode run of the
reference's own query + get_error (tests/golden/train_step_ref.npz, written by tests/make_train_golden.py), the backward oracle
against torch.autograd in float64, the dispatcher's mode switch with the native calls stubbed, and every refusal by its message.
The device side is tests/test_gpu_training.py."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [p for p in (HERE, ROOT) if p not in sys.path]

import batch_subjects as bs  # noqa: E402
import train_oracle as to  # noqa: E402
from icon_amd import training  # noqa: E402
from icon_amd._lib import IconAmdError  # noqa: E402
from icon_amd.engine import IconQueryEngine, check_regressor  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


ex = sys.modules.get("train_step_example") or _load("train_step_example", os.path.join(ROOT, "examples", "train_step.py"))
mtg = sys.modules.get("make_train_golden") or _load("make_train_golden", os.path.join(HERE, "make_train_golden.py"))

OCC_TOL = 1e-4          # the bar every comparison of the oracle with the reference's own occupancies holds (tests/test_batch_oracle.py)
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = mtg.load()
        S = bs.subjects(mtg.B)
        assert str(_cache["g"]["sha1_subjects"]) == bs.sha1(S["smpl_verts"], S["smpl_vis"], S["smpl_cmap"], S["calibs"])
        assert str(_cache["g"]["sha1_planes"]) == bs.sha1(*[mtg.planes(s) for s in range(mtg.S)])
    return _cache["g"]


def oracle_forward(variant):
    """the forward oracle on the fixture's inputs (shared, left unchanged)"""
    if variant not in _cache:
        g = golden()
        feats, prior = mtg.VARIANTS[variant]
        _cache[variant] = to.forward(bs.subjects(mtg.B), [mtg.planes(s) for s in range(mtg.S)], g["points"].transpose(0, 2, 1),
                                     sdf_clip=float(g["sdf_clip"]), smpl_feats=feats, prior=prior)
    return _cache[variant]


def module(variant, dtype=torch.float32):
    """the fixture's regressor: the synthetic checkpoint in training mode"""
    sd = mtg.state_dict(variant)
    reg = ex.Regressor((sd["filters.0.weight"].shape[1], 512, 256, 128, 1), norm="batch", last_op=torch.nn.Sigmoid())
    missing, unexpected = reg.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all("num_batches_tracked" in m for m in missing)
    return reg.to(dtype).train()


def test_fixture_is_small_and_data_only():
    g = np.load(mtg.OUT, allow_pickle=False)
    assert os.path.getsize(mtg.OUT) < 1 << 20
    assert all(g[k].dtype.kind in "fiU" for k in g.files)


@pytest.mark.parametrize("variant", list(mtg.VARIANTS))
def test_forward_oracle_vs_reference_preds(variant):
    """the reference's module on the ORACLE's rows gives the reference's recorded preds (float32 run and float64 run), stack by stack"""
    g, o = golden(), oracle_forward(variant)
    assert np.array_equal(o["in_cube"] != 0, (np.abs(o["xyz"]) < 1.0).all(2)[:, None, :])
    for dtype, suffix in ((torch.float32, ""), (torch.float64, "64")):
        for s in range(mtg.S):
            with torch.no_grad():
                preds = (torch.from_numpy(o["in_cube"]).to(dtype) * module(variant, dtype)(torch.from_numpy(o["rows"][s]).to(dtype))).numpy()
            err = float(np.abs(preds - g[f"{variant}/preds_{s}{suffix}"]).max())
            print(f"{variant} stack {s} {dtype}: max |preds(oracle rows) - reference preds| = {err:.3e}")
            assert err <= OCC_TOL
    if variant == "full":                   # the batch-global cmap list took part (outliers in both subjects)
        assert o["outlier"].any(1).all() and o["K"] == int(o["outlier"].sum())


@pytest.mark.parametrize("variant", list(mtg.VARIANTS))
def test_tap_statement_is_the_forward_oracles(variant):
    """train_oracle.taps / sample restate the forward oracle's image channels BIT FOR BIT: the backward oracle's weights are the
    forward's"""
    o = oracle_forward(variant)
    feats, prior = mtg.VARIANTS[variant]
    csel = mtg.C // 2 if "vis" in feats else mtg.C
    for s in range(mtg.S):
        assert np.array_equal(to.sample(mtg.planes(s), o["xyz"], o["half"], csel), o["rows"][s][:, :csel])
    if variant == "full":
        assert 0 < o["half"].sum() < o["half"].size                    # both feat_select halves


def _special_points(H, W, rng, n=400):
    """projected x, y: random, outside the image (partly and wholly), on texel centres, on the last row / column"""
    xs = np.linspace(-1.0, 1.0, W).astype(np.float32)
    ys = np.linspace(-1.0, 1.0, H).astype(np.float32)
    pts = [rng.uniform(-1.0, 1.0, (n, 2)), rng.uniform(-1.3, 1.3, (n // 2, 2)), rng.uniform(2.0, 5.0, (8, 2)),
           np.stack([xs[rng.randint(0, W, 40)], ys[rng.randint(0, H, 40)]], 1),                      # texel centres
           np.stack([np.full(20, 1.0), rng.uniform(-1, 1, 20)], 1), np.stack([rng.uniform(-1, 1, 20), np.full(20, 1.0)], 1),
           np.array([[1.0, 1.0], [-1.0, -1.0], [1.0, -1.0], [-1.0, 1.0]]),
           np.array([[-1.0 - 1.0 / (W - 1), 0.1], [0.2, 1.0 + 1.0 / (H - 1)]])]                     # one column / row outside: two taps inside
    return np.concatenate(pts).astype(np.float32)


@pytest.mark.parametrize("n_select", [1, 2])
@pytest.mark.parametrize("H,W", [(8, 8), (5, 9)])
def test_backward_oracle_vs_autograd_f64(n_select, H, W):
    """the backward rule in float64 == torch.autograd of F.grid_sample(align_corners=True) + feat_select's gather, to 1e-12"""
    rng = np.random.RandomState(7 + H + n_select)
    S, B, Cc = 2, 2, 6
    csel = Cc // n_select
    xy = np.stack([_special_points(H, W, rng) for _ in range(B)])
    n = xy.shape[1]
    xyz = np.concatenate([xy, np.zeros((B, n, 1), np.float32)], 2)
    half = rng.randint(0, 2, (B, n)) if n_select == 2 else np.zeros((B, n), np.int64)
    g_rows = rng.normal(size=(S, B, csel + 1, n))
    want = []
    for s in range(S):
        planes = torch.from_numpy(rng.normal(size=(B, Cc, H, W))).requires_grad_(True)
        local = F.grid_sample(planes, torch.from_numpy(xy).double().unsqueeze(2), align_corners=True)[..., 0]   # index(), geometry.py:21-43
        if n_select == 2:               # feat_select, mesh_util.py:266-277 (select = vis = 1 - half)
            idx = (torch.from_numpy(half)[:, None, :] * csel + torch.arange(csel)[None, :, None]).long()
            local = torch.gather(local, 1, idx)
        local.backward(torch.from_numpy(g_rows[s][:, :csel]))
        want.append(planes.grad.numpy())
    want = np.stack(want)
    got, mag, count = to.backward(g_rows, xyz, half, (S, B, Cc, H, W), n_select, with_abs=True, dtype=np.float64)
    assert count.max() > 1 and (count == 0).sum() >= 0
    err = np.abs(got - want)
    assert (err <= 1e-12 * mag + 1e-300).all(), float((err / (mag + 1e-300)).max())
    assert np.abs(want).max() > 0.1


@pytest.mark.parametrize("variant", list(mtg.VARIANTS))
def test_backward_oracle_vs_reference_feat_grad(variant):
    """the backward oracle (float32 weights and products, the device's rule) on d error / d rows == the reference's recorded
    float64 feature gradients.

    d error / d rows comes from torch.autograd through the fixture's module in float64 on the oracle's rows.  The bound, per texel,
    with G = sum over its terms of |g| and M = sum |w g|:
      * the float32 weights: ix = ((x + 1) / 2) * (W - 1) carries at most 2 roundings of values below W, so each factor of a
        weight (x1 - ix, ...; the subtraction itself is exact or one more rounding) is off by at most 3 * 2^-24 * W, and a
        product of two factors <= 1 by at most twice that plus its own rounding: 6 * 2^-24 * W * G + 2^-24 * M;
      * the float32 product w * g and the float32 cast of g: 2 * 2^-24 * M;
      * the recorded float64 run is stored to half a quantisation step of the fixture (scale / 2, an absolute term);
      * the rows fed to the module here are the ORACLE's float32 rows, the reference's float64 run formed its image channels in
        float64 and its SMPL channels with its own float32 leaves (2e-6 apart, the bar of the rows test,
        tests/test_gpu_ties_shell.py:742): d error / d rows of a point moves by an amount that does not scale with that point's
        own gradient.  Allowed: OCC_TOL (the bar the oracle's occupancies are held to against the reference's) times the largest
        |d error / d rows| of the call, per unit of weight: OCC_TOL * gmax * (sum of the texel's weights).  This term dominates
        (the observed distances are some 1e-6 of the largest gradient); the arithmetic itself is pinned to 1e-12 by
        test_backward_oracle_vs_autograd_f64."""
    g, o = golden(), oracle_forward(variant)
    feats, prior = mtg.VARIANTS[variant]
    n_select = 2 if "vis" in feats else 1
    reg = module(variant, torch.float64)
    rows = torch.from_numpy(o["rows"]).double().requires_grad_(True)
    in_cube, labels = torch.from_numpy(o["in_cube"]).double(), torch.from_numpy(g["labels"]).double()
    error = sum(F.mse_loss(in_cube * reg(rows[s]), labels) for s in range(mtg.S)) / mtg.S
    error.backward()
    assert abs(float(error.detach()) - float(g[f"{variant}/error64"][0])) <= OCC_TOL
    shape = (mtg.S, mtg.B, mtg.C, mtg.SIZE, mtg.SIZE)
    got, mag, _ = to.backward(rows.grad.numpy(), o["xyz"], o["half"], shape, n_select, with_abs=True)
    G = _sum_abs_g(np.abs(rows.grad.numpy()), o, shape, n_select)
    gmax = float(np.abs(rows.grad.numpy()).max())
    wsum = to.backward(np.ones_like(o["rows"]), o["xyz"], o["half"], shape, n_select)
    u = 2.0 ** -24
    for s in range(mtg.S):
        want = g[f"{variant}/feat_grad_{s}64"]
        step = float(np.load(mtg.OUT)[f"{variant}/feat_grad_{s}/s64"])
        bound = 6 * u * mtg.SIZE * G[s] + 3 * u * mag[s] + OCC_TOL * gmax * wsum[s] + 0.5 * step
        err = np.abs(got[s] - want)
        print(f"{variant} stack {s}: max |oracle - reference feat_grad64| = {err.max():.3e} (largest gradient {np.abs(want).max():.3e}, "
              f"worst err / bound {float((err / (bound + 1e-300)).max()):.3f})")
        assert (err <= bound).all()
        assert ((want == 0) == (mag[s] == 0)).all() or variant != "full"


def _sum_abs_g(absg, o, shape, n_select):
    """sum over the terms of a texel of |g| (weights of 1 on every tap inside)"""
    S, B, Cc, H, W = shape
    csel = Cc // n_select
    x0, y0, _, inside = to.taps(o["xyz"][..., 0], o["xyz"][..., 1], H, W)
    out = np.zeros(shape)
    for b in range(B):
        for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            p = np.nonzero(inside[k, b])[0]
            for s in range(S):
                for c in range(csel):
                    np.add.at(out[s, b], (o["half"][b][p] * csel + c, y0[b][p] + dy, x0[b][p] + dx), absg[s, b, c, p])
    return out


# ---- the dispatcher -------------------------------------------------------------------------------------------------------------------
def _net(**kw):
    torch.manual_seed(3)
    return ex.StandInNet(**kw)


def _cpu_call(B=2, n=5, C=12, size=8, S=2):
    feats = [torch.randn(B, C, size, size) for _ in range(S)]
    return feats, torch.rand(B, 3, n), torch.eye(4)[None].repeat(B, 1, 1)


@pytest.mark.parametrize("start_mode", ["train", "eval"])
def test_dispatcher_switches_on_the_regressors_mode(monkeypatch, start_mode):
    netG = _net()
    getattr(netG, start_mode)()
    q = training.attach(netG)                                       # neither mode raises at attach time
    assert netG.query is q and isinstance(q.engine, IconQueryEngine) and netG.icon_amd_engine is q.engine
    feats, pts, cal = _cpu_call()
    calls = []

    def fake_rows(engine, features, points, calibs, transforms=None):
        calls.append("train")
        B, n = points.shape[0], points.shape[2]
        return [torch.full((B, 13, n), float(s + 1)) for s in range(len(features))], torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0]).expand(B, 1, n)

    def fake_query(features, points, calibs, transforms=None, regressor=None):
        calls.append("eval")
        return ["engine.query"]

    monkeypatch.setattr(training, "point_features_device", fake_rows)
    monkeypatch.setattr(q.engine, "query", fake_query)
    netG.train()
    preds = netG.query(feats, pts, cal, regressor=netG.if_regressor)
    assert calls == ["train"] and len(preds) == 2 and all(p.shape == (2, 1, 5) for p in preds)
    assert (preds[0][:, :, [1, 4]] == 0).all() and (preds[0][:, :, [0, 2, 3]] > 0).all()          # in_cube * regressor(rows)
    assert preds[0].requires_grad and not torch.equal(preds[0], preds[1])                            # one entry per stack, in order
    netG.eval()
    assert netG.query(feats, pts, cal, regressor=netG.if_regressor) == ["engine.query"] and calls == ["train", "eval"]
    assert netG.query(feats, pts, cal) == ["engine.query"]                                           # the bound regressor, eval mode
    netG.if_regressor.train()                                                                        # the REGRESSOR's mode decides
    netG.query(feats, pts, cal)
    assert calls[-1] == "train"


def test_forward_and_get_error_run_unchanged(monkeypatch):
    netG = _net().train()
    training.attach(netG)
    monkeypatch.setattr(training, "point_features_device",
                        lambda eng, features, points, calibs, transforms=None:
                        ([f[:, :6].mean((2, 3))[:, :, None].expand(-1, -1, points.shape[2]).repeat(1, 3, 1)[:, :13] for f in features],
                         torch.ones(points.shape[0], 1, points.shape[2])))
    batch = dict(image=torch.randn(2, 6, 8, 8), sample=torch.rand(2, 3, 7), calib=torch.eye(4)[None].repeat(2, 1, 1), label=torch.ones(2, 1, 7),
                 smpl_verts=torch.zeros(2, 4, 3), smpl_faces=torch.zeros(2, 2, 3, dtype=torch.long), smpl_vis=torch.zeros(2, 4, 1), smpl_cmap=torch.zeros(2, 4, 3))
    pred, err = netG(batch)
    err.backward()
    assert pred.shape == (2, 1, 7) and netG.F_filter.weight.grad.abs().max() > 0 and netG.if_regressor.filters[0].weight.grad is not None


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _engine(prior="icon"):
    return IconQueryEngine(prior_type=prior)


def test_refusals_by_message(monkeypatch):
    feats, pts, cal = _cpu_call()
    with pytest.raises(IconAmdError, match="prior_type 'pamir' is not trained here"):
        training.point_features_device(_engine("pamir"), feats, pts, cal)
    with pytest.raises(IconAmdError, match="points.requires_grad is set"):
        training.point_features_device(_engine(), feats, pts.clone().requires_grad_(True), cal)
    with pytest.raises(IconAmdError, match="calibs.requires_grad is set"):
        training.point_features_device(_engine(), feats, pts, cal.clone().requires_grad_(True))
    with pytest.raises(IconAmdError, match="transforms is not supported"):
        training.point_features_device(_engine(), feats, pts, cal, transforms=torch.eye(3)[None, :2])
    with pytest.raises(IconAmdError, match="points is a CPU tensor"):
        training.point_features_device(_engine(), feats, pts, cal)
    with pytest.raises(IconAmdError, match="non-empty list"):
        training.point_features_device(_engine(), [], pts, cal)
    # the checks behind the device check, reached with tensors that only claim to be on the device
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with pytest.raises(IconAmdError, match="feature stacks differ in shape"):
        training.point_features_device(_engine(), [feats[0], feats[1][:, :, :4]], pts, cal)
    with pytest.raises(IconAmdError, match=r"points must be \[B,3,N\]"):
        training.point_features_device(_engine(), feats, pts[:, :2], cal)
    with pytest.raises(IconAmdError, match="calibs .* must be"):
        training.point_features_device(_engine(), feats, pts, cal[:1])
    eng = _engine()
    eng.search = "brute"
    with pytest.raises(IconAmdError, match="search='brute'"):
        training.point_features_device(eng, feats, pts, cal)
    eng = _engine()
    eng.tie_rule = ("highest", 2)
    with pytest.raises(IconAmdError, match="tie_rule"):
        training.point_features_device(eng, feats, pts, cal)


def test_maskout_is_refused(monkeypatch):
    netG = _net().train()
    monkeypatch.setattr(sys.modules[type(netG).__module__], "maskout", True, raising=False)
    with pytest.raises(IconAmdError, match="maskout is set"):
        training.attach(netG)
    monkeypatch.setattr(sys.modules[type(netG).__module__], "maskout", False, raising=False)
    q = training.attach(netG)
    monkeypatch.setattr(sys.modules[type(netG).__module__], "maskout", True, raising=False)      # set after attach: refused at the call
    with pytest.raises(IconAmdError, match="maskout is set"):
        q(*_cpu_call())


def test_pamir_training_is_refused_through_the_dispatcher():
    netG = _net(prior_type="pamir").train()
    q = training.attach(netG)
    with pytest.raises(IconAmdError, match="prior_type 'pamir' is not trained here"):
        q(*_cpu_call())


def test_check_regressor_still_refuses_a_training_mode_module():
    reg = ex.Regressor(norm="batch")
    with pytest.raises(IconAmdError, match="if_regressor is in training mode: BatchNorm batch statistics cannot be folded"):
        check_regressor(reg.train())
    check_regressor(reg.eval())
    check_regressor(ex.Regressor(norm="group").train(), "group")           # no batch statistics: nothing to refuse


def test_exports():
    import icon_amd
    assert icon_amd.point_features_device is training.point_features_device and icon_amd.TrainQuery is training.TrainQuery
    from icon_amd import _lib
    assert {"icon_train_rows_bytes", "icon_train_rows_forward", "icon_train_rows_backward"} <= set(_lib.SYMBOLS)

"""The training rows on the device (csrc/train_rows.hip, icon_amd/training.py) against tests/train_oracle.py and the recorded
training step of the reference (tests/golden/train_step_ref.npz).  DESIGN.md 4.22 states the rule.

Shapes: the smallest at which the kernels can go wrong - N = 1001 (no multiple of 64 or 256), B = 3 (tiles straddle subjects),
planes of 8^2 (hundreds of points per texel) and 128^2 (most texels empty), one cell holding 5,000 points, N = 1.  Every call
here searches cooperatively (B * N < 98,304); the packet search the larger calls take is the batched query's own code, reached
through the same function (batch_geometry) and covered by tests/test_gpu_batch_oracle.py.

The backward bound, per element, with M = sum |w g| over the element's terms and K their number: the device forms each weight and
each product in float32 by the oracle's own statement (no difference), sums in float64 in another order (K * 2^-52 * M at most) and
rounds once to float32 (2^-24 * |result| <= 2^-24 * M):  |got - want| <= (2^-24 + K * 2^-52) * M + 1e-30 - a sixth of the
3 * 2^-23 * M the design allowed."""
import importlib.util
import os
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [p for p in (HERE, ROOT) if p not in sys.path]

import batch_subjects as bs  # noqa: E402
import train_oracle as to  # noqa: E402
from batch_oracle import project  # noqa: E402
from icon_amd import training  # noqa: E402
from icon_amd.engine import IconQueryEngine  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SDF_CLIP = 0.05
MESH_KEYS = ("smpl_verts", "smpl_faces", "smpl_cmap", "smpl_vis")
ROWS_TOL = 2e-6                          # the bar of the existing rows test (tests/test_gpu_ties_shell.py:742)
FULL, NOVIS = ("sdf", "norm", "vis", "cmap"), ("sdf", "norm", "cmap")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


ex = sys.modules.get("train_step_example") or _load("train_step_example", os.path.join(ROOT, "examples", "train_step.py"))
mtg = sys.modules.get("make_train_golden") or _load("make_train_golden", os.path.join(HERE, "make_train_golden.py"))


def T(x):
    return torch.from_numpy(np.array(x)).to(DEV)         # a copy: the cached inputs are read-only


def engine(S, prior="icon", feats=FULL, cmap_mode="reference"):
    eng = IconQueryEngine(prior_type=prior, sdf_clip=SDF_CLIP, smpl_feats=feats, cmap_mode=cmap_mode)
    if prior == "icon":
        eng.set_mesh(*(T(S[k]) for k in MESH_KEYS))
    return eng


def bound(mag, count_max):
    return (2.0 ** -24 + count_max * 2.0 ** -52) * mag + 1e-30


# ---------------------------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def fwd_case(prior, feats, size, B=3, n=1001, stacks=2):
    """subjects (subject 0 under the identity calibration, so that coordinates of exactly +-1 can be placed), points, planes and the
    oracle's answer - computed once, read-only"""
    S = {k: v.copy() for k, v in bs.subjects(B).items()}
    S["calibs"][0] = np.eye(4, dtype=np.float32)
    pts = bs.candidate_points(S, n)
    pts[0, :4] = [[1.0, 0.2, 0.1], [0.3, -1.0, 0.2], [0.1, 0.2, 1.0], [-1.0, 1.0, -1.0]]      # exactly on the cube: in_cube = 0
    pts[0, 4] = [0.99999994, 0.2, 0.1]                                                           # the float32 below 1: in_cube = 1
    planes = [bs.planes(B, 12, size, s) for s in range(stacks)]
    o = to.forward(S, planes, pts, SDF_CLIP, smpl_feats=feats, prior=prior)
    for a in (pts, *planes, *[v for v in o.values() if isinstance(v, np.ndarray)]):
        a.setflags(write=False)
    return S, pts, planes, o


FWD = [(prior, feats, size) for size in (8, 128) for prior, feats in (("icon", FULL), ("icon", NOVIS), ("pifu", ()))]


@pytest.mark.parametrize("prior,feats,size", FWD)
def test_forward_rows_vs_oracle(prior, feats, size):
    S, pts, planes, o = fwd_case(prior, feats, size)
    eng = engine(S, prior, feats)
    rows, in_cube = training.point_features_device(eng, [T(p) for p in planes], T(pts.transpose(0, 2, 1)), T(S["calibs"]))
    assert len(rows) == 2 and all(tuple(r.shape) == o["rows"][0].shape for r in rows) and tuple(in_cube.shape) == (3, 1, 1001)
    got = torch.stack(rows).cpu().numpy()
    err = float(np.abs(got - o["rows"]).max())
    print(f"{prior} {feats} {size}^2: max |rows - oracle| = {err:.3e}, K = {o['K']}")
    assert np.isfinite(got).all() and err <= ROWS_TOL
    assert np.array_equal(in_cube.cpu().numpy(), o["in_cube"])
    assert o["in_cube"][0, 0, :5].tolist() == [0, 0, 0, 0, 1]
    csel = 6 if "vis" in feats else 12
    assert np.array_equal(got[0][:, csel:], got[1][:, csel:])                   # the stacks share their SMPL / z channels bit for bit
    assert np.abs(got[0][:, :csel] - got[1][:, :csel]).max() > 0.1
    if prior == "icon":
        # the batch-global list: outliers in more than one subject, and their cmap channels are the list's entries exactly
        assert (o["outlier"].sum(1) > 0).sum() >= 2 and 0.1 < o["K"] / o["outlier"].size < 0.9
        bb, pp = np.nonzero(o["outlier"])
        assert np.array_equal(got[:, bb, csel + 1:csel + 4, pp], o["rows"][:, bb, csel + 1:csel + 4, pp])
        if "vis" in feats:
            assert 0 < o["half"].sum() < o["half"].size


def test_forward_rows_equal_the_single_subject_rows_call():
    """where the batch-global cmap rule does not intervene (cmap_mode 'local'): bit for bit what icon_query_rows gives per subject"""
    S, pts, planes, _ = fwd_case("icon", FULL, 128)
    feats = [T(p) for p in planes]
    rows, _ = training.point_features_device(engine(S, cmap_mode="local"), feats, T(pts.transpose(0, 2, 1)), T(S["calibs"]))
    for b in range(3):
        one = engine({k: S[k][b:b + 1] for k in MESH_KEYS}, cmap_mode="local")
        for s in range(2):
            want = one._rows(feats[s][b:b + 1], points=T(pts[b]), calib12=T(S["calibs"][b, :3, :4]).contiguous())
            assert torch.equal(rows[s][b].t(), want[:, :13]), (b, s)


# ---------------------------------------------------------------------------------------------
# 2. backward
# ---------------------------------------------------------------------------------------------
def native_backward(eng, S_calibs, pts, shape, grad, n_select, mask=None, prefill=float("nan")):
    """forward (for the tap records) + backward on the device -> grad_planes [S,B,C,H,W] numpy; the output starts as NaN"""
    Sn, B, Cc, H, W = shape
    stacks = [torch.zeros((B, Cc, H, W), device=DEV) for _ in range(Sn)]
    calib12 = T(S_calibs[:, :3, :4]).reshape(B, 12).contiguous()
    _, _, taps = training._native_forward(eng, stacks, T(np.ascontiguousarray(pts)), calib12)
    out = torch.full(shape, prefill, dtype=torch.float32, device=DEV)
    training._native_backward(T(np.ascontiguousarray(grad, np.float32)), taps, shape, n_select, (1 << Sn) - 1 if mask is None else mask, out=out)
    return out, taps


def texel_xy(H, W):
    return np.linspace(-1.0, 1.0, W).astype(np.float32), np.linspace(-1.0, 1.0, H).astype(np.float32)


def synth_points(kind, B, n, H, W, rng):
    """projected (x, y) [B,n,2] of the pifu cases (identity calibrations: the points are their own projections)"""
    xs, ys = texel_xy(H, W)
    if kind == "one_cell":                               # every point strictly inside the cell of texel (2, 3)
        x = rng.uniform(xs[3] + 1e-3, xs[4] - 1e-3, (B, n))
        y = rng.uniform(ys[2] + 1e-3, ys[3] - 1e-3, (B, n))
    elif kind == "outside":
        x, y = rng.uniform(1.5, 4.0, (B, n)) * rng.choice([-1, 1], (B, n)), rng.uniform(-3.0, 3.0, (B, n))
    elif kind == "centres":
        x, y = xs[rng.randint(0, W, (B, n))], ys[rng.randint(0, H, (B, n))]
    elif kind == "last":                                 # the last column, the last row, the corner
        x, y = rng.uniform(-1, 1, (B, n)), rng.uniform(-1, 1, (B, n))
        x[:, ::2], y[:, 1::2] = 1.0, 1.0
        x[:, :3], y[:, :3] = 1.0, 1.0
    else:                                                # "random": in and around the image
        x, y = rng.uniform(-1.2, 1.2, (B, n)), rng.uniform(-1.2, 1.2, (B, n))
    return np.stack([x, y], 2).astype(np.float32)


#          name          kind        B  n     S  C   H    W
BWD = [("one_cell",     "one_cell", 1, 5000, 2, 6,  16,  16),      # the long-segment path: 5,000 points in one cell
       ("sparse",       "random",   2, 50,   2, 6,  128, 128),     # most texels get nothing
       ("outside",      "outside",  2, 300,  2, 6,  8,   8),       # no tap inside at all
       ("centres",      "centres",  2, 700,  2, 6,  9,   5),       # weights exactly 0 and 1 (2 / (size - 1) is a power of two)
       ("last",         "last",     2, 700,  2, 6,  8,   9),       # the last row and column; H != W
       ("B1",           "random",   1, 1001, 2, 12, 8,   8),
       ("B5",           "random",   5, 1001, 2, 6,  8,   8),
       ("S1",           "random",   3, 1001, 1, 12, 8,   8),
       ("S3_C7",        "random",   2, 333,  3, 7,  5,   6),       # S * C = 21: a partial second pass of the 16 channel lanes
       ("N1",           "random",   3, 1,    2, 6,  8,   8)]


@pytest.mark.parametrize("name,kind,B,n,S,C,H,W", BWD, ids=[c[0] for c in BWD])
def test_backward_vs_oracle_one_half(name, kind, B, n, S, C, H, W):
    """pifu: no feat_select (one half), points placed in the projected space"""
    rng = np.random.RandomState(len(name) + 13 * B + n)
    xy = synth_points(kind, B, n, H, W, rng)
    pts = np.concatenate([xy, rng.uniform(-0.5, 0.5, (B, n, 1)).astype(np.float32)], 2)
    calibs = np.repeat(np.eye(4, dtype=np.float32)[None], B, 0)
    xyz = np.stack([project(calibs[b], pts[b]) for b in range(B)])
    assert np.array_equal(xyz, pts)
    grad = rng.normal(size=(S, B, C + 1, n)).astype(np.float32)
    shape = (S, B, C, H, W)
    want, mag, count = to.backward(grad, xyz, np.zeros((B, n), np.int64), shape, 1, with_abs=True)
    got, _ = native_backward(engine(None, "pifu", ()), calibs, pts, shape, grad, 1)
    got = got.cpu().numpy()
    assert not np.isnan(got).any()                                   # every element written
    empty = np.broadcast_to((count == 0)[None, :, None], shape)
    assert (got[empty] == 0).all() and np.array_equal(np.signbit(got[empty]), np.zeros(int(empty.sum()), bool))
    err = np.abs(got - want)
    print(f"{name}: worst |got - want| / bound = {float((err / bound(mag, count.max())).max()):.3f}, most terms in a texel {count.max()}, "
          f"empty texels {int((count == 0).sum())} of {count.size}")
    assert (err <= bound(mag, count.max())).all()
    if kind == "one_cell":
        assert count.max() == n and (count > 0).sum() == 4
    if kind == "sparse":
        assert (count == 0).mean() > 0.95
    if kind == "outside":
        assert count.max() == 0
    if kind == "centres":
        x0, y0, w, inside = to.taps(xyz[..., 0], xyz[..., 1], H, W)
        assert set(np.unique(w[inside]).tolist()) <= {0.0, 1.0}
    if kind == "last":
        assert count[:, H - 1, :].sum() > 0 and count[:, :, W - 1].sum() > 0 and count[0, H - 1, W - 1] >= 3


@pytest.mark.parametrize("size", [8, 128])
def test_backward_vs_oracle_both_halves(size):
    """icon with 'vis': the points' feat_select halves come from the search; the subjects and points of the forward test"""
    S, pts, planes, o = fwd_case("icon", FULL, size)
    assert 0 < o["half"].sum() < o["half"].size
    rng = np.random.RandomState(5 + size)
    shape = (2, 3, 12, size, size)
    grad = rng.normal(size=o["rows"].shape).astype(np.float32)
    want, mag, count = to.backward(grad, o["xyz"], o["half"], shape, 2, with_abs=True)
    got, _ = native_backward(engine(S), S["calibs"], pts, shape, grad, 2)
    got = got.cpu().numpy()
    err = np.abs(got - want)
    print(f"both halves {size}^2: worst |got - want| / bound = {float((err / bound(mag, count.max())).max()):.3f}, most terms {count.max()}")
    assert not np.isnan(got).any() and (err <= bound(mag, count.max())).all()
    assert (got[mag == 0] == 0).all() and np.abs(want).max() > 1.0


def test_backward_skips_the_stacks_nobody_asked_for():
    rng = np.random.RandomState(3)
    B, n, shape = 2, 200, (2, 2, 6, 8, 8)
    pts = np.concatenate([synth_points("random", B, n, 8, 8, rng), np.zeros((B, n, 1), np.float32)], 2)
    calibs = np.repeat(np.eye(4, dtype=np.float32)[None], B, 0)
    grad = rng.normal(size=(2, B, 7, n)).astype(np.float32)
    eng = engine(None, "pifu", ())
    both, _ = native_backward(eng, calibs, pts, shape, grad, 1)
    only1, _ = native_backward(eng, calibs, pts, shape, grad, 1, mask=2)
    assert torch.isnan(only1[0]).all() and torch.equal(only1[1], both[1])


# ---------------------------------------------------------------------------------------------
# 3. determinism
# ---------------------------------------------------------------------------------------------
def test_backward_is_deterministic_and_stable_under_permutation():
    """equal bytes from call to call and on a side stream.  Under a permutation of the points of every subject (grad_rows permuted
    alike) the terms of a texel are summed in another order - the order is by point index - so the result is equal within the
    bound of the oracle comparison, not bit for bit."""
    S, pts, planes, o = fwd_case("icon", FULL, 8)
    rng = np.random.RandomState(11)
    shape = (2, 3, 12, 8, 8)
    grad = rng.normal(size=o["rows"].shape).astype(np.float32)
    eng = engine(S)
    a, taps = native_backward(eng, S["calibs"], pts, shape, grad, 2)
    b = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    g = T(grad)
    training._native_backward(g, taps, shape, 2, 3, out=b)
    assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    c = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    with torch.cuda.stream(side):
        training._native_backward(g, taps, shape, 2, 3, out=c)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(a, c)
    perm = np.stack([rng.permutation(1001) for _ in range(3)])
    pts_p = np.stack([pts[b][perm[b]] for b in range(3)])
    grad_p = np.stack([np.stack([grad[s, b][:, perm[b]] for b in range(3)]) for s in range(2)])
    d, _ = native_backward(eng, S["calibs"], pts_p, shape, grad_p, 2)
    _, mag, count = to.backward(grad, o["xyz"], o["half"], shape, 2, with_abs=True)
    err = np.abs(d.cpu().numpy() - a.cpu().numpy())
    assert (err <= 2 * bound(mag, count.max())).all()               # each within the bound of the same exact sum


# ---------------------------------------------------------------------------------------------
# 4. wiring: torch.autograd through the Function against torch's own operators on the device
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior,feats,size", [("icon", FULL, 8), ("icon", NOVIS, 128), ("pifu", (), 8)])
def test_autograd_wiring_vs_torch_operators(prior, feats, size):
    S, pts, planes, o = fwd_case(prior, feats, size)
    rng = np.random.RandomState(17)
    n_select = 2 if "vis" in feats else 1
    csel = 12 // n_select
    g = [T(rng.normal(size=o["rows"][0].shape).astype(np.float32)) for _ in range(2)]
    leaves = [T(p).requires_grad_(True) for p in planes]
    rows, in_cube = training.point_features_device(engine(S, prior, feats), leaves, T(pts.transpose(0, 2, 1)), T(S["calibs"]))
    assert not in_cube.requires_grad
    loss = sum((r * gi).sum() for r, gi in zip(rows, g))
    got = torch.autograd.grad(loss, leaves, retain_graph=True)
    with pytest.raises(RuntimeError):                                 # used once per forward: a double backward raises
        gg = torch.autograd.grad(loss, leaves, create_graph=True)
        torch.autograd.grad(gg[0].sum(), leaves)
    # torch's operators from the same projected points
    uv = T(o["xyz"][..., :2]).unsqueeze(2)
    ref_leaves = [T(p).requires_grad_(True) for p in planes]
    ref_loss = 0
    for s in range(2):
        local = F.grid_sample(ref_leaves[s], uv, align_corners=True)[..., 0]
        if n_select == 2:
            idx = (T(o["half"])[:, None, :] * csel + torch.arange(csel, device=DEV)[None, :, None]).long()
            local = torch.gather(local, 1, idx)
        ref_loss = ref_loss + (local * g[s][:, :csel]).sum()
    want = torch.autograd.grad(ref_loss, ref_leaves)
    grad = np.stack([x.cpu().numpy() for x in g])
    _, mag, count = to.backward(grad, o["xyz"], o["half"], (2, 3, 12, size, size), n_select, with_abs=True)
    K = int(count.max())
    tol = bound(mag, K) + K * 2.0 ** -24 * mag                        # + the float32 accumulation of torch's atomics
    for s in range(2):
        err = np.abs(got[s].cpu().numpy() - want[s].cpu().numpy())
        print(f"{prior} {size}^2 stack {s}: worst |native - torch| / tol = {float((err / tol[s]).max()):.3f} (K = {K})")
        assert (err <= tol[s]).all()
    # a stack that needs no gradient gets none, and no backward call is made when none does
    mixed = [T(planes[0]), T(planes[1]).requires_grad_(True)]
    rows, _ = training.point_features_device(engine(S, prior, feats), mixed, T(pts.transpose(0, 2, 1)), T(S["calibs"]))
    only = torch.autograd.grad(sum((r * gi).sum() for r, gi in zip(rows, g)), mixed[1])[0]
    assert torch.equal(only, got[1])
    rows, _ = training.point_features_device(engine(S, prior, feats), [T(p) for p in planes], T(pts.transpose(0, 2, 1)), T(S["calibs"]))
    assert not rows[0].requires_grad


# ---------------------------------------------------------------------------------------------
# 5. the reference's step
# ---------------------------------------------------------------------------------------------
def _net(variant):
    feats, prior = mtg.VARIANTS[variant]
    netG = ex.StandInNet(prior_type=prior, smpl_feats=feats, channels=mtg.C, num_stack=mtg.S, sdf_clip=float(mtg.SDF_CLIP))
    sd = mtg.state_dict(variant)
    missing, unexpected = netG.if_regressor.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all("num_batches_tracked" in m for m in missing)
    netG.to(DEV)
    S = bs.subjects(mtg.B)
    netG.smpl_feat_dict = {k: T(S[k]) for k in MESH_KEYS}
    return netG, S


@pytest.mark.parametrize("variant", list(mtg.VARIANTS))
def test_training_step_vs_reference(variant):
    """query + get_error + backward of the attached network on the fixture's inputs against the reference's float64 records.  Per
    quantity the distance is max |x - x64|; the yardstick is the same distance of the reference's own float32 run; the device is
    allowed 4 x the yardstick (its GEMMs and reductions order their sums differently from the CPU's), with a floor of
    1e-6 * min(1, max |x64|) - relative to the quantity's size where that is below 1, so that a gradient of 1e-5 is not waved
    through by an absolute 1e-6 - except for the biases in front of a BatchNorm, whose true gradient is 0 (the norm removes the
    mean): there both runs record rounding noise and the floor is the plain 1e-6."""
    g = mtg.load()
    netG, S = _net(variant)
    q = training.attach(netG)
    netG.train()
    leaves = [T(mtg.planes(s)).requires_grad_(True) for s in range(mtg.S)]
    pts, cal, labels = T(g["points"]), T(g["calibs"]), T(g["labels"])
    preds = netG.query(leaves, pts, cal, regressor=netG.if_regressor)
    assert len(preds) == mtg.S and all(tuple(p.shape) == (mtg.B, 1, mtg.N) for p in preds)
    error = netG.get_error(preds, labels)
    error.backward()
    reg = netG.if_regressor
    got = {"error": error.detach().reshape(1), "w0_grad": reg.filters[0].weight.grad}
    for s in range(mtg.S):
        got[f"preds_{s}"], got[f"feat_grad_{s}"] = preds[s].detach(), leaves[s].grad
    for l, f in enumerate(reg.filters):
        got[f"bias_grad_{l}"] = f.bias.grad
    for l, nrm in enumerate(reg.norms):
        got[f"running_mean_{l}"], got[f"running_var_{l}"] = nrm.running_mean, nrm.running_var
    bad = []
    for k, v in got.items():
        ref64, ref32 = g[f"{variant}/{k}64"], g[f"{variant}/{k}"]
        yard = float(np.abs(ref32.astype(np.float64) - ref64).max())
        dist = float(np.abs(v.detach().cpu().numpy().astype(np.float64).reshape(ref64.shape) - ref64).max())
        noise = k.startswith("bias_grad_") and int(k[-1]) < len(reg.norms)
        allowed = max(4.0 * yard, 1e-6 if noise else 1e-6 * min(1.0, float(np.abs(ref64).max())))
        print(f"{variant} {k:16s} reference float32 {yard:.3e}  device {dist:.3e}  allowed {allowed:.3e}  (max |x64| {np.abs(ref64).max():.3e})")
        if not dist <= allowed:
            bad.append(k)
    assert not bad, bad
    # the stacks are in order: stack 0's preds are not stack 1's
    assert not torch.equal(preds[0], preds[1])
    # eval mode: the same object answers with IconQueryEngine.query's bytes
    netG.eval()
    with torch.no_grad():
        ev = netG.query([leaves[-1].detach()], pts, cal, regressor=netG.if_regressor)
        eng = IconQueryEngine(prior_type=netG.prior_type, sdf_clip=netG.sdf_clip, smpl_feats=netG.smpl_feats)
        if netG.prior_type == "icon":
            eng.set_mesh(*(netG.smpl_feat_dict[k] for k in MESH_KEYS))
        want = eng.query([leaves[-1].detach()], pts, cal, regressor=netG.if_regressor)
    assert len(ev) == 1 and torch.equal(ev[0], want[0]) and ev[0].abs().max() > 0


# ---------------------------------------------------------------------------------------------
# 6. a step end to end
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior", ["icon", "pifu"])
def test_two_steps_end_to_end(prior):
    """the example's step function, B = 2, N = 2000: every parameter of the regressor and of the filter moves, and so do the running
    statistics.  (That the native calls wait for nothing is the timing tool's record - tools/train_rows_timing.py counts the
    synchronising API calls with the profiler; no such counter is reachable from here.)"""
    torch.manual_seed(0)
    netG = ex.StandInNet(prior_type=prior).to(DEV)
    training.attach(netG)
    opt = torch.optim.Adam(netG.parameters(), lr=1e-3)
    batch = ex.make_batch(2, 2000, DEV)
    assert 0.2 < float(batch["label"].mean()) < 0.8
    before = {k: v.detach().clone() for k, v in netG.state_dict().items()}
    errs = [float(ex.train_step(netG, opt, batch)) for _ in range(2)]
    assert all(np.isfinite(e) and e > 0 for e in errs)
    after = netG.state_dict()
    same = [k for k in before if torch.equal(before[k], after[k])]
    assert not same, same
    assert all(not torch.equal(before[f"if_regressor.norms.{l}.running_mean"], after[f"if_regressor.norms.{l}.running_mean"]) for l in range(3))
    netG.eval()
    with torch.no_grad():
        pred, _ = netG(batch)
    assert tuple(pred.shape) == (2, 1, 2000) and torch.isfinite(pred).all()

"""The pamir training rows on the device (csrc/train_rows.hip: icon_train_pamir_forward, icon_train_vol_backward; icon_amd/training.py)
against tests/train_pamir_oracle.py and the recorded training step of the reference (tests/golden/train_step_pamir_ref.npz).
DESIGN.md 4.23 states the rule.

Shapes: the smallest at which the kernels can go wrong - N = 1001 (no multiple of 64 or 256), B = 3 (tiles straddle subjects),
volumes of (5,6,7) (many points per voxel, D != H != W, W below the gather's run of 8 voxels) and 32^3 (four runs per row, most
voxels empty), one cell holding 5,000 points, N = 1, S * Cv = 21 channels (a partial second pass of the 16 channel lanes).

The backward bound, per element, is tests/test_gpu_training.py's argument unchanged: with M = sum |w g| over the element's terms
and K the largest number of terms of a voxel, the device forms each weight and each product in float32 by the oracle's own
statement (no difference), sums in float64 in another order (K * 2^-52 * M at most) and rounds once to float32 (2^-24 * M at most):
|got - want| <= (2^-24 + K * 2^-52) * M + 1e-30."""
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

import batch_pamir as bp  # noqa: E402
import batch_subjects as bs  # noqa: E402
import train_oracle as to  # noqa: E402
import train_pamir_oracle as tpo  # noqa: E402
from batch_oracle import project  # noqa: E402
from icon_amd import training  # noqa: E402
from icon_amd.engine import IconQueryEngine  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROWS_TOL = 2e-6                          # the bar of the existing rows tests (tests/test_gpu_training.py)
C_IMG, CV = 12, 7


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


ex = sys.modules.get("train_step_example") or _load("train_step_example", os.path.join(ROOT, "examples", "train_step.py"))


def T(x):
    return torch.from_numpy(np.array(x)).to(DEV)         # a copy: the cached inputs are read-only


def engine():
    return IconQueryEngine(prior_type="pamir")


def bound(mag, count_max):
    return (2.0 ** -24 + count_max * 2.0 ** -52) * mag + 1e-30


def volumes(B, shape, stack):
    """[B,CV,D,H,W] f32 in [-1, 1], another draw per stack"""
    return np.random.RandomState(811 + 17 * stack + shape[0]).uniform(-1.0, 1.0, (B, CV) + tuple(shape)).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def fwd_case(vshape, B=3, n=1001, stacks=2):
    """calibrations (subject 0 under the identity, so that coordinates of exactly +-1 can be placed), points, planes, volumes and
    the oracle's answer - computed once, read-only"""
    calibs = bs.subjects(B)["calibs"].copy()
    calibs[0] = np.eye(4, dtype=np.float32)
    pts = bp.candidate_points({"calibs": calibs}, n)
    pts[0, :4] = [[1.0, 0.2, 0.1], [0.3, -1.0, 0.2], [0.1, 0.2, 1.0], [-1.0, 1.0, -1.0]]      # exactly on the cube: in_cube = 0
    pts[0, 4] = [0.99999994, 0.2, 0.1]                                                           # the float32 below 1: in_cube = 1
    pts[0, 5] = [0.2, 0.1, 0.99999994]
    planes = [bs.planes(B, C_IMG, 8, s) for s in range(stacks)]
    vols = [volumes(B, vshape, s) for s in range(stacks)]
    o = tpo.forward(calibs, planes, vols, pts)
    for a in (calibs, pts, *planes, *vols, *o.values()):
        a.setflags(write=False)
    return calibs, pts, planes, vols, o


def _coords_of(taps, B, n):
    """the device's own projected coordinates from the tap records: x, y, and z in the fourth word"""
    w = taps.cpu().numpy().view(np.float32).reshape(B, n, 4)
    return np.ascontiguousarray(w[..., [0, 1, 3]])


@pytest.mark.parametrize("vshape", [(5, 6, 7), (32, 32, 32)], ids=["5x6x7", "32^3"])
def test_forward_rows_vs_oracle(vshape):
    calibs, pts, planes, vols, o = fwd_case(vshape)
    assert all(np.abs(v).max() <= 1.0 for v in vols)
    feats, vf = [T(p) for p in planes], [T(v) for v in vols]
    rows, in_cube = training.point_features_device(engine(), feats, T(pts.transpose(0, 2, 1)), T(calibs), vol_feats=vf)
    assert len(rows) == 2 and all(tuple(r.shape) == (3, C_IMG + CV, 1001) for r in rows) and tuple(in_cube.shape) == (3, 1, 1001)
    got = torch.stack(rows).cpu().numpy()
    err = float(np.abs(got - o["rows"]).max())
    print(f"pamir {vshape}: max |rows - oracle| = {err:.3e}")
    assert np.isfinite(got).all() and err <= ROWS_TOL
    assert np.array_equal(in_cube.cpu().numpy(), o["in_cube"])
    assert o["in_cube"][0, 0, :6].tolist() == [0, 0, 0, 0, 1, 1]
    # every channel bit for bit the stated float32 rule at the device's own projected coordinates
    calib12 = T(calibs[:, :3, :4]).reshape(3, 12).contiguous()
    rows2, in_cube2, taps = training._native_pamir_forward(feats, vf, T(np.ascontiguousarray(pts)), calib12)
    assert torch.equal(rows2, torch.stack(rows)) and torch.equal(in_cube2, in_cube)
    xyz = _coords_of(taps, 3, 1001)
    assert np.abs(xyz - o["xyz"]).max() <= 1e-6
    for s in range(2):
        assert np.array_equal(got[s][:, :C_IMG], to.sample(planes[s], xyz, np.zeros((3, 1001), np.int64), C_IMG)), s
        assert np.array_equal(got[s][:, C_IMG:], tpo.sample3(vols[s], xyz)), s
    assert np.abs(got[0][:, :C_IMG] - got[1][:, :C_IMG]).max() > 0.1 and np.abs(got[0][:, C_IMG:] - got[1][:, C_IMG:]).max() > 0.1


# ---------------------------------------------------------------------------------------------
# 2. the volumes' backward
# ---------------------------------------------------------------------------------------------
def native_vol_backward(pts, shape, grad, n_planes, mask=None, prefill=float("nan")):
    """forward under identity calibrations (for the tap records) + backward on the device -> grad_vols [S,B,Cv,D,H,W]; the output
    starts as NaN"""
    Sn, B = shape[:2]
    stacks = [torch.zeros((B, n_planes, 4, 4), device=DEV) for _ in range(Sn)]
    vols = [torch.zeros(shape[1:], device=DEV) for _ in range(Sn)]
    calib12 = T(np.repeat(np.eye(4, dtype=np.float32)[None, :3, :4], B, 0)).reshape(B, 12).contiguous()
    _, _, taps = training._native_pamir_forward(stacks, vols, T(np.ascontiguousarray(pts)), calib12)
    out = torch.full(shape, prefill, dtype=torch.float32, device=DEV)
    training._native_vol_backward(T(np.ascontiguousarray(grad, np.float32)), taps, shape, n_planes, (1 << Sn) - 1 if mask is None else mask, out=out)
    return out, taps


def synth_points3(kind, B, n, D, H, W, rng):
    """projected (x, y, z) [B,n,3] (identity calibrations: the points are their own projections)"""
    ax = [np.linspace(-1.0, 1.0, size).astype(np.float32) for size in (W, H, D)]
    if kind == "one_cell":                               # every point strictly inside the cell of voxel (z 1, y 2, x 1)
        p = np.stack([rng.uniform(a[i] + 1e-3, a[i + 1] - 1e-3, (B, n)) for a, i in zip(ax, (1, 2, 1))], 2)
    elif kind == "outside":
        p = rng.uniform(-3.0, 3.0, (B, n, 3))
        p[..., rng.randint(0, 3)] = rng.uniform(1.5, 4.0, (B, n)) * rng.choice([-1, 1], (B, n))
    elif kind == "centres":
        p = np.stack([a[rng.randint(0, len(a), (B, n))] for a in ax], 2)
    elif kind == "last":                                 # the last plane, row, column and the corner
        p = rng.uniform(-1, 1, (B, n, 3))
        p[:, 0::3, 0], p[:, 1::3, 1], p[:, 2::3, 2] = 1.0, 1.0, 1.0
        p[:, :3] = 1.0
    else:                                                # "random": in and around the volume
        p = rng.uniform(-1.2, 1.2, (B, n, 3))
    return p.astype(np.float32)


#          name          kind        B  n     S  Cv  D   H   W
BWD = [("one_cell",     "one_cell", 1, 5000, 2, 7,  4,  4,  4),      # the long-segment path: 5,000 points in one cell
       ("sparse",       "random",   2, 50,   2, 7,  32, 32, 32),     # most voxels get nothing
       ("outside",      "outside",  2, 300,  2, 7,  8,  8,  8),      # no tap inside at all
       ("centres5",     "centres",  2, 700,  2, 7,  5,  5,  5),      # weights exactly 0 and 1 (2 / (size - 1) is a power of two)
       ("centres9x5x3", "centres",  2, 700,  2, 7,  9,  5,  3),
       ("last",         "last",     2, 700,  2, 7,  8,  9,  7),      # the last plane, row, column, corner; D != H != W
       ("B1",           "random",   1, 1001, 2, 7,  6,  5,  9),      # W = 9: a full run of 8 voxels and a run of one
       ("B5",           "random",   5, 1001, 2, 7,  5,  6,  7),
       ("S1",           "random",   3, 1001, 1, 7,  5,  6,  7),
       ("S3_Cv7",       "random",   2, 333,  3, 7,  5,  6,  7),      # S * Cv = 21: a partial second pass of the 16 channel lanes
       ("N1",           "random",   3, 1,    2, 7,  5,  6,  7)]


@pytest.mark.parametrize("name,kind,B,n,S,Cv,D,H,W", BWD, ids=[c[0] for c in BWD])
def test_vol_backward_vs_oracle(name, kind, B, n, S, Cv, D, H, W):
    rng = np.random.RandomState(len(name) + 13 * B + n)
    pts = synth_points3(kind, B, n, D, H, W, rng)
    eye = np.eye(4, dtype=np.float32)
    assert np.array_equal(np.stack([project(eye, pts[b]) for b in range(B)]), pts)
    n_planes = 3
    grad = rng.normal(size=(S, B, n_planes + Cv, n)).astype(np.float32)
    shape = (S, B, Cv, D, H, W)
    want, mag, count = tpo.backward3(grad, pts, shape, n_planes, with_abs=True)
    got, taps = native_vol_backward(pts, shape, grad, n_planes)
    assert np.array_equal(_coords_of(taps, B, n), pts)
    got = got.cpu().numpy()
    assert not np.isnan(got).any()                                   # every element written
    empty = np.broadcast_to((count == 0)[None, :, None], shape)
    assert (got[empty] == 0).all() and not np.signbit(got[empty]).any()
    err = np.abs(got - want)
    print(f"{name}: worst |got - want| / bound = {float((err / bound(mag, count.max())).max()):.3f}, most terms in a voxel {count.max()}, "
          f"empty voxels {int((count == 0).sum())} of {count.size}")
    assert (err <= bound(mag, count.max())).all()
    if kind == "one_cell":
        assert count.max() == n and (count > 0).sum() == 8
    if name == "sparse":
        assert (count == 0).mean() > 0.95 and count.max() >= 1
    if kind == "outside":
        assert count.max() == 0
    if kind == "centres":
        w, inside = tpo.taps3(pts[..., 0], pts[..., 1], pts[..., 2], D, H, W)[3:]
        assert set(np.unique(w[inside]).tolist()) <= {0.0, 1.0} and np.abs(want).max() > 1.0
    if kind == "last":
        assert count[:, D - 1].sum() > 0 and count[:, :, H - 1].sum() > 0 and count[:, :, :, W - 1].sum() > 0 and count[0, D - 1, H - 1, W - 1] >= 3
    if kind == "random" and n >= 333:
        assert np.abs(want).max() > 1.0


def test_vol_backward_skips_the_stacks_nobody_asked_for():
    rng = np.random.RandomState(3)
    B, n, shape = 2, 200, (2, 2, 7, 5, 6, 7)
    pts = synth_points3("random", B, n, 5, 6, 7, rng)
    grad = rng.normal(size=(2, B, 3 + 7, n)).astype(np.float32)
    both, _ = native_vol_backward(pts, shape, grad, 3)
    only1, _ = native_vol_backward(pts, shape, grad, 3, mask=2)
    assert torch.isnan(only1[0]).all() and torch.equal(only1[1], both[1])


# ---------------------------------------------------------------------------------------------
# 3. determinism
# ---------------------------------------------------------------------------------------------
def test_vol_backward_is_deterministic_and_stable_under_permutation():
    """equal bytes from call to call and on a side stream.  Under a permutation of the points of every subject (grad_rows permuted
    alike) the terms of a voxel are summed in another order - the order is by point index - so the result is equal within the
    bound of the oracle comparison, not bit for bit."""
    rng = np.random.RandomState(11)
    B, n, shape = 3, 1001, (2, 3, 7, 5, 6, 7)
    pts = synth_points3("random", B, n, 5, 6, 7, rng)
    grad = rng.normal(size=(2, B, 3 + 7, n)).astype(np.float32)
    a, taps = native_vol_backward(pts, shape, grad, 3)
    g = T(grad)
    b = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    training._native_vol_backward(g, taps, shape, 3, 3, out=b)
    assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    c = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    with torch.cuda.stream(side):
        training._native_vol_backward(g, taps, shape, 3, 3, out=c)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(a, c)
    perm = np.stack([rng.permutation(n) for _ in range(B)])
    pts_p = np.stack([pts[k][perm[k]] for k in range(B)])
    grad_p = np.stack([np.stack([grad[s, k][:, perm[k]] for k in range(B)]) for s in range(2)])
    d, _ = native_vol_backward(pts_p, shape, grad_p, 3)
    _, mag, count = tpo.backward3(grad, pts, shape, 3, with_abs=True)
    err = np.abs(d.cpu().numpy() - a.cpu().numpy())
    assert (err <= 2 * bound(mag, count.max())).all()               # each within the bound of the same exact sum


# ---------------------------------------------------------------------------------------------
# 4. wiring: torch.autograd through the Function against torch's own operators on the device
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vshape", [(5, 6, 7), (32, 32, 32)], ids=["5x6x7", "32^3"])
def test_autograd_wiring_vs_torch_operators(vshape):
    calibs, pts, planes, vols, o = fwd_case(vshape)
    rng = np.random.RandomState(17)
    g = [T(rng.normal(size=o["rows"][0].shape).astype(np.float32)) for _ in range(2)]
    P, cal = T(pts.transpose(0, 2, 1)), T(calibs)

    def run(need_planes, need_vols):
        lp = [T(p).requires_grad_(need_planes[s]) for s, p in enumerate(planes)]
        lv = [T(v).requires_grad_(need_vols[s]) for s, v in enumerate(vols)]
        rows, in_cube = training.point_features_device(engine(), lp, P, cal, vol_feats=lv)
        assert not in_cube.requires_grad
        return lp, lv, rows, sum((r * gi).sum() for r, gi in zip(rows, g))

    lp, lv, rows, loss = run([True, True], [True, True])
    got = torch.autograd.grad(loss, lp + lv, retain_graph=True)
    with pytest.raises(RuntimeError):                                 # used once per forward: a double backward raises
        gg = torch.autograd.grad(loss, lp + lv, create_graph=True)
        torch.autograd.grad(gg[0].sum(), lp)
    # torch's operators from the same projected points: two grid_samples per stack
    xyz = T(o["xyz"])
    rp, rv = [T(p).requires_grad_(True) for p in planes], [T(v).requires_grad_(True) for v in vols]
    ref_loss = 0
    for s in range(2):
        img = F.grid_sample(rp[s], xyz[..., :2].unsqueeze(2), align_corners=True)[..., 0]
        vol = F.grid_sample(rv[s], xyz[:, :, None, None, :], align_corners=True)[:, :, :, 0, 0]
        ref_loss = ref_loss + (torch.cat([img, vol], 1) * g[s]).sum()
    want = torch.autograd.grad(ref_loss, rp + rv)
    grad = np.stack([x.cpu().numpy() for x in g])
    _, mag2, count2 = to.backward(grad, o["xyz"], np.zeros((3, 1001), np.int64), (2, 3, C_IMG, 8, 8), 1, with_abs=True)
    _, mag3, count3 = tpo.backward3(grad, o["xyz"], (2, 3, CV) + tuple(vshape), C_IMG, with_abs=True)
    for name, off, mag, K in (("planes", 0, mag2, int(count2.max())), ("volumes", 2, mag3, int(count3.max()))):
        tol = bound(mag, K) + K * 2.0 ** -24 * mag                    # + the float32 accumulation of torch's atomics
        for s in range(2):
            err = np.abs(got[off + s].cpu().numpy() - want[off + s].cpu().numpy())
            print(f"pamir {vshape} {name} stack {s}: worst |native - torch| / tol = {float((err / tol[s]).max()):.3f} (K = {K})")
            assert (err <= tol[s]).all() and np.abs(want[off + s].cpu().numpy()).max() > 0.1
    # what needs no gradient gets none, and what does gets the same bytes
    lp, lv, _, loss = run([False, True], [True, False])
    loss.backward()
    assert lp[0].grad is None and lv[1].grad is None and torch.equal(lp[1].grad, got[1]) and torch.equal(lv[0].grad, got[2])
    lp, lv, _, loss = run([False, False], [False, True])              # no plane needs one: the planes' backward is not called
    calls = []
    orig_p, orig_v = training._native_backward, training._native_vol_backward
    training._native_backward = lambda *a, **k: calls.append("planes") or orig_p(*a, **k)
    training._native_vol_backward = lambda *a, **k: calls.append("vols") or orig_v(*a, **k)
    try:
        loss.backward()
        assert calls == ["vols"] and torch.equal(lv[1].grad, got[3])
        lp, lv, _, loss = run([True, False], [False, False])
        loss.backward()
        assert calls == ["vols", "planes"] and torch.equal(lp[0].grad, got[0])
    finally:
        training._native_backward, training._native_vol_backward = orig_p, orig_v
    _, _, rows, _ = run([False, False], [False, False])
    assert not rows[0].requires_grad


# ---------------------------------------------------------------------------------------------
# 5. the reference's step
# ---------------------------------------------------------------------------------------------
mtpg = sys.modules.get("make_train_pamir_golden") or _load("make_train_pamir_golden", os.path.join(HERE, "make_train_pamir_golden.py"))


def _net():
    """PamirStandInNet's interface carrying the fixture's regressor and the reference-shaped encoder with the reference's weights;
    ``held`` receives the encoder's outputs of every call, with retain_grad() on them"""
    netG = ex.PamirStandInNet(bp.subjects(mtpg.B)["code"], channels=mtpg.C, vol_channels=mtpg.CV, num_stack=mtpg.S)
    missing, unexpected = netG.if_regressor.load_state_dict({k: torch.from_numpy(v) for k, v in mtpg.regressor_state_dict().items()}, strict=False)
    assert not unexpected and all("num_batches_tracked" in m for m in missing)
    netG.ve = mtpg.encoder()
    netG.to(DEV)
    held = []
    inner = netG.ve.forward

    def forward(x, intermediate_output=True):
        outs = inner(x, intermediate_output=intermediate_output)
        if torch.is_grad_enabled():
            for o in outs:
                o.retain_grad()
            held.extend(outs)
        return outs
    netG.ve.forward = forward
    return netG, held


def _composed_query(netG, vol):
    """HGPIFuNet.query's pamir branch in training mode from torch's own operators on the device: no native code"""
    def query(features, points, calibs, transforms=None, regressor=None):
        xyz = torch.baddbmm(calibs[:, :3, 3:4], calibs[:, :3, :3], points)
        in_cube = ((xyz > -1.0) & (xyz < 1.0)).all(dim=1, keepdim=True).float()
        uv = xyz.transpose(1, 2)
        preds = []
        for im_feat, vol_feat in zip(features, netG.ve(vol, intermediate_output=True)):
            img = F.grid_sample(im_feat, uv[:, :, None, :2], align_corners=True)[..., 0]
            vf = F.grid_sample(vol_feat, uv[:, :, None, None, :], align_corners=True)[:, :, :, 0, 0]
            preds.append(in_cube * regressor(torch.cat([img, vf], 1)))
        return preds
    return query


def _records(netG, held, leaves, preds, error):
    reg = netG.if_regressor
    got = {"error": error.detach().reshape(1), "w0_grad": reg.filters[0].weight.grad}
    idx = torch.from_numpy(mtpg.voxel_sample()).to(DEV)
    for s in range(mtpg.S):
        got[f"preds_{s}"], got[f"feat_grad_{s}"], got[f"vol_grad_{s}"] = preds[s].detach(), leaves[s].grad, held[s].grad.reshape(-1)[idx]
    for l, f in enumerate(reg.filters):
        got[f"bias_grad_{l}"] = f.bias.grad
    for l, nrm in enumerate(reg.norms):
        got[f"running_mean_{l}"], got[f"running_var_{l}"] = nrm.running_mean, nrm.running_var
    for k, p in netG.ve.named_parameters():
        if p.grad is not None:
            got[f"ve_grad.{k}"] = p.grad
    for k, m in netG.ve.named_modules():
        if isinstance(m, torch.nn.BatchNorm3d) and int(m.num_batches_tracked) > 0:
            got[f"ve_stat.{k}.running_mean"], got[f"ve_stat.{k}.running_var"] = m.running_mean, m.running_var
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in got.items()}


def _no_miopen(fn):
    """run the test with torch's own convolution kernels: MIOpen's first use of each 3-D convolution of the encoders (solver search and
    compilation, once per process) costs seconds - 3.4 s forward and 5.4 s backward for the reference-shaped encoder at 128^3 - where
    torch's kernels take a quarter of a second; what is under test is in front of and behind the encoder, not the library under it"""
    import functools

    @functools.wraps(fn)
    def wrapper(*a, **k):
        with torch.backends.cudnn.flags(enabled=False):
            return fn(*a, **k)
    return wrapper


@_no_miopen
def test_training_step_vs_reference():
    """query + get_error + backward of the attached network on the fixture's inputs against the reference's float64 records, the
    semantic volume being the oracle's (the HIP voxeliser's known <= 1e-5 distance from it is pinned elsewhere and not mixed in).
    Per quantity the distance is max |x - x64|; the yardstick is the same distance of the reference's own float32 run; the same
    distance of torch's own operators on this device (grid_sample for both samplers, no native code) is measured here.  Allowed:
    max(4 x yardstick, 2 x composed, floor), the floor being tests/test_gpu_training.py's: 1e-6 * min(1, max |x64|), and the plain
    1e-6 for the gradient of a bias in front of a BatchNorm (the regressor's first three, every Conv3d bias of the encoder), whose
    true value is 0."""
    g = mtpg.load()
    vol = T(mtpg.oracle_volume())
    pts, cal, labels = T(g["points"]), T(g["calibs"]), T(g["labels"])
    runs = {}
    for kind in ("native", "composed"):
        netG, held = _net()
        if kind == "native":
            q = training.attach(netG, voxelizer="hip")
            q.engine._semantic_volume = lambda B=None: vol
            # an eval call first: its encoded volume is cached, and must not survive the training step
            netG.smpl_feat_dict = {k: T(v) for k, v in bp.padded(bp.subjects(mtpg.B)).items()}
            netG.eval()
            with torch.no_grad():
                stale = netG.query([T(mtpg.planes(mtpg.S - 1))], pts, cal, regressor=netG.if_regressor)[0]
            assert q.engine._volb_key is not None
        else:
            netG.query = _composed_query(netG, vol)
        netG.train()
        leaves = [T(mtpg.planes(s)).requires_grad_(True) for s in range(mtpg.S)]
        preds = netG.query(leaves, pts, cal, regressor=netG.if_regressor)
        assert len(preds) == mtpg.S and all(tuple(p.shape) == (mtpg.B, 1, mtpg.N) for p in preds) and len(held) == mtpg.S
        error = netG.get_error(preds, labels)
        error.backward()
        runs[kind] = _records(netG, held, leaves, preds, error)
        if kind == "native":
            assert q.engine._volb_key is None and not torch.equal(preds[0], preds[1])
            # eval mode afterwards: IconQueryEngine.query's bytes, from volumes encoded by the CURRENT weights and statistics
            netG.eval()
            with torch.no_grad():
                ev = netG.query([leaves[-1].detach()], pts, cal, regressor=netG.if_regressor)
                eng = IconQueryEngine(prior_type="pamir")
                eng.set_volume_features(netG.ve(vol, intermediate_output=False)[-1])
                want = eng.query([leaves[-1].detach()], pts, cal, regressor=netG.if_regressor)
            assert len(ev) == 1 and torch.equal(ev[0], want[0]) and ev[0].abs().max() > 0 and not torch.equal(ev[0], stale)
    assert sorted(runs["native"]) == sorted(k[5:] for k in g if k.startswith("step/") and not k.endswith("64"))
    bad = []
    print(f"{'quantity':34s} {'ref float32':>11s} {'composed':>10s} {'native':>10s} {'allowed':>10s} {'max |x64|':>10s}")
    for k, v in runs["native"].items():
        ref64, ref32 = g[f"step/{k}64"], g[f"step/{k}"]
        yard = float(np.abs(ref32.astype(np.float64) - ref64).max())
        dist = float(np.abs(v.reshape(ref64.shape) - ref64).max())
        comp = float(np.abs(runs["composed"][k].reshape(ref64.shape) - ref64).max())
        noise = (k.startswith("bias_grad_") and int(k[-1]) < 3) or (k.startswith("ve_grad.") and "conv" in k and k.endswith(".bias"))
        allowed = max(4.0 * yard, 2.0 * comp, 1e-6 if noise else 1e-6 * min(1.0, float(np.abs(ref64).max())))
        print(f"{k:34s} {yard:11.3e} {comp:10.3e} {dist:10.3e} {allowed:10.3e} {np.abs(ref64).max():10.3e}")
        if not dist <= allowed:
            bad.append(k)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# 6. two steps end to end
# ---------------------------------------------------------------------------------------------
@_no_miopen
def test_two_steps_end_to_end():
    """the example's step function on PamirStandInNet, B = 2, N = 2000, the HIP voxeliser unpatched and called once per step: every
    parameter of the regressor, of the filter and of the volume encoder moves, and so do the running statistics"""
    from icon_amd import engine as engine_mod
    torch.manual_seed(0)
    batch = ex.make_batch(2, 2000, DEV, prior="pamir")
    assert 0.2 < float(batch["label"].mean()) < 0.8 and batch["pad_v_num"].tolist() == [5, 7]
    netG = ex.PamirStandInNet(batch["vertex_code"].cpu().numpy()).to(DEV)
    q = training.attach(netG, voxelizer="hip")
    opt = torch.optim.Adam(netG.parameters(), lr=1e-3)
    before = {k: v.detach().clone() for k, v in netG.state_dict().items()}
    calls = []
    orig = engine_mod.semantic_voxelization_batch
    engine_mod.semantic_voxelization_batch = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        errs = [float(ex.train_step(netG, opt, batch)) for _ in range(2)]
    finally:
        engine_mod.semantic_voxelization_batch = orig
    assert len(calls) == 2 and all(np.isfinite(e) and e > 0 for e in errs)
    after = netG.state_dict()
    same = [k for k in before if torch.equal(before[k], after[k])]
    assert not same, same
    assert any(k.startswith("ve.") and k.endswith("running_mean") for k in before) and any(k.startswith("ve.res.1") for k in before)
    netG.eval()
    with torch.no_grad():
        pred, _ = netG(batch)
    assert tuple(pred.shape) == (2, 1, 2000) and torch.isfinite(pred).all() and q.engine._volb_key is not None

"""The pamir training rows' rule on the CPU: tests/train_pamir_oracle.py against a recorded training-mode step of
the reference's own pamir network (tests/golden/train_step_pamir_ref.npz, written by tests/make_train_pamir_golden.py), the 3-D
tap statement against torch's grid_sample in float32 and its backward in float64, the dispatcher with the native calls stubbed,
every new refusal by its message, the exports and the scratch check of the new backward entry.  The device side is
tests/test_gpu_training_pamir.py."""
import ctypes as C
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

import batch_pamir as bp  # noqa: E402
import batch_subjects as bs  # noqa: E402
import train_pamir_oracle as tpo  # noqa: E402
from icon_amd import _lib, training  # noqa: E402
from icon_amd._lib import IconAmdError  # noqa: E402
from icon_amd.engine import IconQueryEngine  # noqa: E402
from oracle import ref_loader  # noqa: E402
from test_native_call import P, Z, check_scratch_row, i32, i64  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


ex = sys.modules.get("train_step_example") or _load("train_step_example", os.path.join(ROOT, "examples", "train_step.py"))
mtpg = sys.modules.get("make_train_pamir_golden") or _load("make_train_pamir_golden", os.path.join(HERE, "make_train_pamir_golden.py"))

OCC_TOL = 1e-4          # the bar of tests/test_training.py: the oracle's occupancies against the reference's own
needs_reference = pytest.mark.skipif(not ref_loader.available(), reason="reference tree not present")
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = mtpg.load()
    return _cache["g"]


def regressor(dtype=torch.float32):
    """the fixture's regressor: lib/net/MLP.py restated (examples/train_step.py), the recorded checkpoint, training mode"""
    reg = ex.Regressor((mtpg.C + mtpg.CV, 512, 256, 128, 1), norm="batch", last_op=torch.nn.Sigmoid())
    missing, unexpected = reg.load_state_dict({k: torch.from_numpy(v) for k, v in mtpg.regressor_state_dict().items()}, strict=False)
    assert not unexpected and all("num_batches_tracked" in m for m in missing)
    return reg.to(dtype).train()


def test_fixture_is_small_and_data_only():
    g = np.load(mtpg.OUT, allow_pickle=False)
    assert os.path.getsize(mtpg.OUT) < 1 << 20
    assert all(g[k].dtype.kind in "fiU" for k in g.files)


def test_fixture_inputs_are_the_derived_ones():
    g = golden()
    Sj = bp.subjects(mtpg.B)
    assert str(g["sha1_subjects"]) == bs.sha1(Sj["verts"], Sj["tets"], Sj["code"], Sj["calibs"])
    assert str(g["sha1_planes"]) == bs.sha1(*[mtpg.planes(s) for s in range(mtpg.S)])
    assert str(g["sha1_regressor"]) == bs.sha1(*[v for _, v in sorted(mtpg.regressor_state_dict().items())])
    assert str(g["sha1_ve"]) == mtpg.ve_sha1(mtpg.encoder())                 # the replica carries the reference encoder's weights
    assert np.array_equal(g["calibs"], Sj["calibs"]) and np.array_equal(g["voxel_sample"], mtpg.voxel_sample())
    assert g["pad_v_num"].tolist() == list(bp.PAD_V[:2]) and g["pad_v_num"][0] != g["pad_v_num"][1] and g["pad_f_num"][0] != g["pad_f_num"][1]
    assert g["points"].shape == (mtpg.B, 3, mtpg.N) and 0.2 < float(g["labels"].mean()) < 0.8
    assert sum(k.startswith("step/ve_grad.") and not k.endswith("64") for k in g) == 24


@needs_reference
def test_regenerating_the_float64_step_agrees_with_the_fixture():
    """a fresh run of the reference's step reproduces the records.  The float64 run is the one compared (make_train_pamir_golden.agrees
    says why: two float32 runs on the CPU differ with the thread count of the process by far more than either differs from float64)"""
    g = golden()
    Sj, points, labels = mtpg.inputs()
    assert np.array_equal(points, g["points"]) and np.array_equal(labels, g["labels"])
    info = {}
    worst = mtpg.agrees(mtpg.run(Sj, points, labels, torch.float64, info))
    print(f"worst |fresh float64 run - fixture| / allowed = {worst:.3f}")
    assert worst <= 1.0 and info["sha1_ve"] == str(g["sha1_ve"])


@pytest.mark.parametrize("dtype,suffix", [(torch.float32, ""), (torch.float64, "64")], ids=["float32", "float64"])
def test_forward_oracle_vs_reference_preds(dtype, suffix):
    """the reference's regressor on the ORACLE's rows gives the reference's recorded preds, stack by stack.  The vol_feats the rows
    are sampled from are recomputed here: the restated voxeliser leaf, then the reference's encoder (its layer list, its weights)
    in training mode, as the reference's query ran it."""
    g = golden()
    Sj = bp.subjects(mtpg.B)
    with torch.no_grad():
        vol_feats = [v.float().numpy() for v in mtpg.encoder(dtype)(torch.from_numpy(mtpg.oracle_volume()).to(dtype), intermediate_output=True)]
    assert len(vol_feats) == mtpg.S and vol_feats[0].shape == (mtpg.B, mtpg.CV, 32, 32, 32) and np.abs(vol_feats[0] - vol_feats[1]).max() > 0.1
    o = tpo.forward(Sj["calibs"], [mtpg.planes(s) for s in range(mtpg.S)], vol_feats, g["points"].transpose(0, 2, 1))
    assert np.array_equal(o["in_cube"] != 0, (np.abs(o["xyz"]) < 1.0).all(2)[:, None, :]) and 0.5 < o["in_cube"].mean() < 1.0
    for s in range(mtpg.S):
        assert np.array_equal(o["rows"][s][:, mtpg.C:], tpo.sample3(vol_feats[s], o["xyz"]))      # the stated rule IS the oracle's rows
        with torch.no_grad():
            preds = (torch.from_numpy(o["in_cube"]).to(dtype) * regressor(dtype)(torch.from_numpy(o["rows"][s]).to(dtype))).numpy()
        err = float(np.abs(preds - g[f"step/preds_{s}{suffix}"]).max())
        print(f"pamir stack {s} {dtype}: max |preds(oracle rows) - reference preds| = {err:.3e}")
        assert err <= OCC_TOL


def _special_points3(D, H, W, rng, n=400):
    """projected x, y, z: random, outside the volume (partly and wholly), on voxel centres, on the last plane / row / column"""
    ax = [np.linspace(-1.0, 1.0, size).astype(np.float32) for size in (W, H, D)]
    last = []
    for k in range(3):
        p = rng.uniform(-1, 1, (20, 3))
        p[:, k] = 1.0
        last.append(p)
    pts = [rng.uniform(-1.0, 1.0, (n, 3)), rng.uniform(-1.3, 1.3, (n // 2, 3)), rng.uniform(2.0, 5.0, (8, 3)),
           np.stack([a[rng.randint(0, len(a), 40)] for a in ax], 1), *last,
           np.array([[1.0, 1.0, 1.0], [-1.0, -1.0, -1.0], [1.0, -1.0, 1.0], [-1.0, 1.0, 0.3]]),
           np.array([[-1.0 - 1.0 / (W - 1), 0.1, 0.2], [0.2, 1.0 + 1.0 / (H - 1), 0.1], [0.2, 0.1, 1.0 + 1.0 / (D - 1)]])]   # one layer outside
    return np.concatenate(pts).astype(np.float32)


@pytest.mark.parametrize("D,H,W", [(5, 5, 5), (4, 7, 9)])
def test_backward_oracle_vs_autograd_f64(D, H, W):
    """the backward rule in float64 == torch.autograd of the 5-D F.grid_sample(align_corners=True).  The bound is the 2-D oracle's
    own (tests/test_training.py): 1e-12 of the element's magnitude sum M = sum |w g| - both sides form the same float64 weights
    and products and differ in the order of a float64 sum of at most a few hundred terms (K * 2^-53 * M << 1e-12 * M)."""
    rng = np.random.RandomState(7 + D + W)
    S, B, Cv, n_planes = 2, 2, 3, 2
    xyz = np.stack([_special_points3(D, H, W, rng) for _ in range(B)])
    n = xyz.shape[1]
    g_rows = rng.normal(size=(S, B, n_planes + Cv, n))
    want = []
    for s in range(S):
        vol = torch.from_numpy(rng.normal(size=(B, Cv, D, H, W))).requires_grad_(True)
        local = F.grid_sample(vol, torch.from_numpy(xyz).double()[:, :, None, None, :], align_corners=True)[:, :, :, 0, 0]   # index(), geometry.py:21-43
        local.backward(torch.from_numpy(g_rows[s][:, n_planes:]))
        want.append(vol.grad.numpy())
    want = np.stack(want)
    got, mag, count = tpo.backward3(g_rows, xyz, (S, B, Cv, D, H, W), n_planes, with_abs=True, dtype=np.float64)
    assert count.max() > 1
    err = np.abs(got - want)
    assert (err <= 1e-12 * mag + 1e-300).all(), float((err / (mag + 1e-300)).max())
    assert np.abs(want).max() > 0.1


@pytest.mark.parametrize("D,H,W", [(5, 5, 5), (4, 7, 9), (32, 32, 32)])
def test_tap_statement_vs_grid_sample_f32(D, H, W):
    """taps3 / sample3 in float32 against float32 F.grid_sample on the CPU.  Both evaluate ATen's statement; what may differ is
    where a product is contracted into the following addition and how the vectorised kernel orders its work.  Per sample, with
    M = sum |w_k t_k| over the eight corners: a corner's weight takes two roundings after its factors ((x-term * y-term) * z-term),
    the product t_k * w_k one - three roundings, each relative to |w_k t_k|, 3 * 2^-24 * M in all - and the seven additions one
    each, relative to a partial sum of at most M: 7 * 2^-24 * M.  Ten roundings on either side: |got - want| <= 20 * 2^-24 * M."""
    rng = np.random.RandomState(3 + D)
    B, Cv = 2, 3
    xyz = np.stack([_special_points3(D, H, W, rng) for _ in range(B)])
    vol = rng.normal(size=(B, Cv, D, H, W)).astype(np.float32)
    got = tpo.sample3(vol, xyz)
    want = F.grid_sample(torch.from_numpy(vol), torch.from_numpy(xyz)[:, :, None, None, :], align_corners=True)[:, :, :, 0, 0].numpy()
    M = tpo.sample3(np.abs(vol), xyz).astype(np.float64)                  # the weights are >= 0 wherever a corner is inside
    w, inside = tpo.taps3(xyz[..., 0], xyz[..., 1], xyz[..., 2], D, H, W)[3:]
    assert (w[inside] >= 0).all()
    err = np.abs(got.astype(np.float64) - want)
    print(f"{D}x{H}x{W}: worst |sample3 - grid_sample| / bound = {float((err / (20 * 2.0 ** -24 * M + 1e-30)).max()):.3f}")
    assert (err <= 20 * 2.0 ** -24 * M * (1 + 2.0 ** -20) + 1e-30).all()
    assert (got[:, :, 600:608] == 0).all() and np.abs(got).max() > 1.0     # the points far outside: every corner contributes 0


# ---- the dispatcher -------------------------------------------------------------------------------------------------------------------
def _pamir_net():
    torch.manual_seed(3)
    return ex.PamirStandInNet(np.zeros((4, 3), np.float32), volume_res=8)


def _cpu_call(B=2, n=5, C=6, size=8, S=2):
    return [torch.randn(B, C, size, size) for _ in range(S)], torch.rand(B, 3, n), torch.eye(4)[None].repeat(B, 1, 1)


def test_dispatcher_encodes_once_per_training_call_and_never_caches(monkeypatch):
    netG = _pamir_net().train()
    q = training.attach(netG, voxelizer="hip")
    eng = q.engine
    feats, pts, cal = _cpu_call()
    seen, ve_calls, vox_calls = [], [], []

    def fake_rows(engine, features, points, calibs, transforms=None, vol_feats=None):
        seen.append(vol_feats)
        B, n = points.shape[0], points.shape[2]
        return [vf.mean((2, 3, 4))[:, :, None].expand(-1, -1, n).repeat(1, 2, 1)[:, :13] for vf in vol_feats], torch.ones(B, 1, n)

    def fake_volume(B):
        vox_calls.append((B, torch.is_grad_enabled()))
        return torch.rand(B, 3, 8, 8, 8)

    inner = netG.ve.forward
    monkeypatch.setattr(netG.ve, "forward", lambda x, intermediate_output=True: ve_calls.append(intermediate_output) or inner(x, intermediate_output))
    monkeypatch.setattr(training, "point_features_device", fake_rows)
    monkeypatch.setattr(eng, "_semantic_volume", fake_volume)
    eng._vol_key, eng._volb_key, eng._mlp_key = ("stale",), ("stale",), ("stale",)
    preds = netG.query(feats, pts, cal, regressor=netG.if_regressor)
    assert ve_calls == [True] and vox_calls == [(2, False)]                 # one encoder call, intermediate outputs; the voxeliser without a gradient
    assert eng._vol_key is None and eng._volb_key is None                   # an eval call after this step encodes with the new weights
    assert eng._mlp_key is None                                             # and folds the regressor's new running statistics
    assert len(preds) == 2 and all(p.shape == (2, 1, 5) and p.requires_grad for p in preds)
    assert len(seen[0]) == 2 and all(tuple(v.shape) == (2, 7, 2, 2, 2) and v.requires_grad for v in seen[0])
    sum(p.sum() for p in preds).backward()
    assert all(p.grad is not None for p in netG.ve.parameters()) and netG.ve.conv1.weight.grad.abs().max() > 0   # the encoder is reached through the rows
    netG.query(feats, pts, cal, regressor=netG.if_regressor)
    assert ve_calls == [True, True] and len(vox_calls) == 2 and seen[1][0] is not seen[0][0]
    # eval mode: the engine's own query, the dispatcher's pamir half untouched
    monkeypatch.setattr(eng, "query", lambda *a, **k: ["engine.query"])
    netG.eval()
    assert netG.query(feats, pts, cal, regressor=netG.if_regressor) == ["engine.query"] and len(ve_calls) == 2


def test_semantic_volume_is_what_the_eval_path_encodes(monkeypatch):
    """_pamir_volume voxelises through _semantic_volume (both paths call one method) and caches the ENCODED volume as before"""
    netG = _pamir_net().eval()
    eng = IconQueryEngine.attach(netG, voxelizer="hip")
    netG.smpl_feat_dict = dict(voxel_verts=torch.zeros(2, 9, 3), voxel_faces=torch.zeros(2, 6, 4, dtype=torch.long))
    calls = []
    monkeypatch.setattr(eng, "_semantic_volume", lambda B=None: calls.append(B) or torch.rand(2 if B else 1, 3, 8, 8, 8))
    a = eng._pamir_volume(2)
    assert calls == [2] and tuple(a.shape) == (2, 7, 2, 2, 2) and eng._pamir_volume(2) is a and calls == [2]
    eng._volb_key = None                                                   # what a training call does
    assert eng._pamir_volume(2) is not a and calls == [2, 2]
    assert tuple(eng._pamir_volume().shape) == (1, 7, 2, 2, 2) and calls == [2, 2, None]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_message(monkeypatch):
    feats, pts, cal = _cpu_call()
    vols = [torch.zeros(2, 7, 4, 4, 4) for _ in range(2)]
    eng = IconQueryEngine(prior_type="pamir")
    with pytest.raises(IconAmdError, match="prior_type 'pamir' is not trained here without vol_feats"):
        training.point_features_device(eng, feats, pts, cal)
    with pytest.raises(IconAmdError, match="vol_feats belong to prior_type 'pamir'"):
        training.point_features_device(IconQueryEngine(prior_type="pifu"), feats, pts, cal, vol_feats=vols)
    with pytest.raises(IconAmdError, match="points is a CPU tensor"):
        training.point_features_device(eng, feats, pts, cal, vol_feats=vols)
    netG = ex.StandInNet(prior_type="pamir").train()
    with pytest.raises(IconAmdError, match="prior_type 'pamir' is not trained here: netG has no `ve` / `voxelization`"):
        training.attach(netG)(feats, pts, cal)
    # the checks behind the device check: 4-D and 3-D tensors claim to be on the device, the 5-D volumes say where they are
    on_device = [True]
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: self.dim() != 5 or on_device[0]))
    with pytest.raises(IconAmdError, match="vol_feats holds 1 volumes for 2 feature stacks"):
        training.point_features_device(eng, feats, pts, cal, vol_feats=vols[:1])
    with pytest.raises(IconAmdError, match="vol_feats holds 3 volumes for 2 feature stacks"):
        training.point_features_device(eng, feats, pts, cal, vol_feats=vols + vols[:1])
    with pytest.raises(IconAmdError, match=r"vol_feats differ in shape \(\(2, 7, 4, 4, 4\) and \(2, 7, 4, 4, 5\)\)"):
        training.point_features_device(eng, feats, pts, cal, vol_feats=[vols[0], torch.zeros(2, 7, 4, 4, 5)])
    with pytest.raises(IconAmdError, match=r"vol_feats\[1\] \(3, 7, 4, 4, 4\) must be \[2,Cv,D,H,W\]"):
        training.point_features_device(eng, feats, pts, cal, vol_feats=[vols[0], torch.zeros(3, 7, 4, 4, 4)])
    with pytest.raises(IconAmdError, match=r"vol_feats\[0\] \(7, 4, 4, 4\) must be \[2,Cv,D,H,W\]"):
        training.point_features_device(eng, feats, pts, cal, vol_feats=[vols[0][0], vols[1]])
    on_device[0] = False
    with pytest.raises(IconAmdError, match=r"vol_feats\[0\] is a CPU tensor"):
        training.point_features_device(eng, feats, pts, cal, vol_feats=vols)


def test_c_entries_refuse_by_name():
    L = _lib.lib()
    n = C.c_int64(0)

    def err(rc, code):
        assert rc == code, (rc, L.icon_last_error())
        return L.icon_last_error().decode()

    assert "more than 8 feature stacks" in err(L.icon_train_vol_bytes(i32(2), i64(100), i32(9), i32(7), i32(8), i32(8), i32(8), C.byref(n)), 3)
    assert "B * N must be below 2^31" in err(L.icon_train_vol_bytes(i32(2), i64(1 << 30), i32(2), i32(7), i32(8), i32(8), i32(8), C.byref(n)), 1)
    assert "must stay below 2^32 - 1" in err(L.icon_train_vol_bytes(i32(8), i64(100), i32(2), i32(7), i32(1024), i32(1024), i32(1024), C.byref(n)), 3)
    assert "must be positive" in err(L.icon_train_vol_bytes(i32(2), i64(100), i32(2), i32(7), i32(0), i32(8), i32(8), C.byref(n)), 1)
    assert "null argument" in err(L.icon_train_vol_backward(Z, P, i32(2), C.c_uint32(3), i32(2), i32(13), i32(6), i32(7), i32(8), i32(8), i32(8),
                                                            i64(100), P, P, i64(1 << 30), Z), 1)
    assert "fewer channels" in err(L.icon_train_vol_backward(P, P, i32(2), C.c_uint32(3), i32(2), i32(12), i32(6), i32(7), i32(8), i32(8), i32(8),
                                                             i64(100), P, C.c_void_p(8192), i64(1 << 30), Z), 1)
    ptrs, vptrs = (C.c_void_p * 2)(4096, 4096), (C.c_void_p * 2)(4096, 4096)

    def fwd(shapes, vshapes, S=2, N=100, stacks=ptrs, vols=vptrs, taps=P):
        return L.icon_train_pamir_forward(stacks, (C.c_int32 * 8)(*shapes), vols, (C.c_int32 * 10)(*vshapes), i32(S), P, P, i64(N), P, P, taps, Z)

    plane, vol = [2, 6, 8, 8], [2, 7, 4, 4, 4]
    assert "null argument" in err(fwd(plane * 2, vol * 2, taps=Z), 1)
    assert "a volume is null" in err(fwd(plane * 2, vol * 2, vols=(C.c_void_p * 2)(4096, 0)), 1)
    assert "the feature stacks differ in shape" in err(fwd(plane + [2, 6, 8, 9], vol * 2), 1)
    assert "the volumes differ in shape" in err(fwd(plane * 2, vol + [2, 7, 4, 4, 5]), 1)
    assert "another number of subjects than the planes" in err(fwd(plane * 2, [3, 7, 4, 4, 4] * 2), 1)
    assert "B * N must be below 2^31" in err(fwd(plane * 2, vol * 2, N=1 << 30), 1)
    assert "more than 8 feature stacks" in err(L.icon_train_pamir_forward((C.c_void_p * 9)(*[4096] * 9), (C.c_int32 * 36)(*plane * 9), (C.c_void_p * 9)(*[4096] * 9),
                                                                          (C.c_int32 * 45)(*vol * 9), i32(9), P, P, i64(100), P, P, P, Z), 3)
    assert "16-byte aligned" in err(fwd(plane * 2, vol * 2, taps=C.c_void_p(4100)), 1)
    # the planes' forward keeps its refusal of the pamir prior and names the entry that takes its place
    msg = err(L.icon_train_rows_forward(Z, i32(_lib.PRIOR["pamir"]), C.c_float(0.05), i32(0), i32(0), i32(0), i32(0), ptrs, (C.c_int32 * 8)(*plane * 2),
                                        i32(2), P, P, i64(100), P, P, P, i32(0), P, Z), 3)
    assert "the pamir prior is not trained here" in msg and "icon_train_pamir_forward" in msg


# ---- exports, symbols, scratch --------------------------------------------------------------------------------------------------------
def test_exports_and_symbols():
    import icon_amd
    assert icon_amd.point_features_device is training.point_features_device and icon_amd.TrainQuery is training.TrainQuery
    new = {"icon_train_pamir_forward", "icon_train_vol_bytes", "icon_train_vol_backward"}
    assert new <= set(_lib.SYMBOLS)
    L = _lib.lib()
    assert all(hasattr(L, s) for s in new)
    header = open(os.path.join(ROOT, "include", "icon_amd.h")).read()
    assert all(f"int {s}(" in header for s in new)
    assert hasattr(ex, "PamirStandInNet") and "vol_feats" in training.point_features_device.__code__.co_varnames


def _train_vol_backward(L, scratch, nbytes, scan):
    return L.icon_train_vol_backward(P, P, i32(2), C.c_uint32(3), i32(2), i32(13), i32(6), i32(7), i32(8), i32(8), i32(8), i64(100), P,
                                     scratch, i64(nbytes), Z)


def test_scratch_row_of_the_volume_backward():
    check_scratch_row(("icon_train_vol_backward", "icon_train_vol_bytes", (i32(2), i64(100), i32(2), i32(7), i32(8), i32(8), i32(8)),
                       _train_vol_backward, False))

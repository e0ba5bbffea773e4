"""The split-precision MLP on v_mfma_f32_16x16x32_f16: one wave = 32 points = two 16-point blocks, accumulators of one
layer are the B operands of the next through a K permutation the packer applies.  These tests put every block, wave and
workgroup edge, every layer's permutation, the fused kernel against the materialising one and the range net against the
float64 oracle (tolerance 1e-4, the project's bar for the occupancy)."""
import ctypes as C

import numpy as np
import pytest
import torch

from common import assets, oracle_query, orc, rows16, vol_assets
from icon_amd import _lib, synth

pytestmark = pytest.mark.gpu

TOL = 1e-4


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda:0"))


def handle(sd):
    from icon_amd.engine import MlpHandle
    return MlpHandle({k: torch.from_numpy(v) for k, v in sd.items()})


@pytest.fixture(scope="module")
def body():
    return assets("body")


@pytest.fixture(scope="module")
def rows_and_ref(body):
    x = np.random.RandomState(16).normal(0, 1, (600, 13)).astype(np.float32)
    return x, orc.Mlp(body.state_dict).forward(x, f64=True)[:, 0]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 600])
def test_forward_at_block_wave_and_workgroup_edges(body, rows_and_ref, n):
    """16 points = one MFMA block, 32 = one wave, 256 = one workgroup: the first n rows of one batch, each n its own launch"""
    x, ref = rows_and_ref
    rows = rows16(x[:n])
    rows[:, 13:] = 7.0                                  # pad slots and the code word never reach the GEMM
    y = handle(body.state_dict).forward(T(rows), precision="f16x3").cpu().numpy()
    err = np.abs(y - ref[:n]).max()
    print(f"n={n}: max |occ - float64| = {err:.3e}")
    assert y.shape == (n,) and np.isfinite(y).all()
    assert err <= TOL, err


def permutation_layer(l, co, ci):
    """distinct-valued scaled permutation: every input column of the layer is used, every entry has its own value"""
    w = np.zeros((co, ci), np.float32)
    o = np.arange(co)
    if l == 0:                                          # 512 x 13
        w[o, (5 * o + 1) % ci] = 1.0 + o / co
    elif l == 1:                                        # 256 x 512: two hidden columns per row, together all 512
        w[o, (3 * o + 1) % 512] = 1.0 + o / 256.0
        w[o, (3 * o + 1 + 256) % 512] = -(0.5 + o / 512.0)
    elif l == 2:                                        # 128 x (256 + 13): two hidden columns per row (all 256) + one raw input
        w[o, (5 * o + 2) % 256] = 1.0 + o / 128.0
        w[o, (5 * o + 2 + 128) % 256] = -(0.5 + o / 256.0)
        w[o, 256 + o % 13] = 0.25 + o / 1024.0
    else:                                               # 1 x (128 + 13): a weight of its own per channel
        k = np.arange(ci)
        w[0] = 0.01 * (1.0 + k / ci) * np.where(k % 2 == 0, 1.0, -1.0)
    return w[:, :, None]


@pytest.mark.parametrize("layer", [0, 1, 2, 3])
def test_per_layer_permutation_checkpoints(layer):
    """one layer at a time carries a distinct-valued scaled permutation (the others keep the synthetic checkpoint's dense
    weights): a misplaced k-slot or output channel of THAT layer's packed operands routes a wrong, differently scaled channel on"""
    sd = synth.make_mlp_state_dict(seed=31 + layer)
    co, ci = synth.mlp_layer_shapes()[layer]
    sd[f"filters.{layer}.weight"] = permutation_layer(layer, co, ci)
    used = np.abs(sd[f"filters.{layer}.weight"][:, :, 0]).sum(0) > 0
    assert used.all()                                   # no column is left out of the check
    x = np.random.RandomState(layer).normal(0, 1, (1000, 13)).astype(np.float32)
    y = handle(sd).forward(T(rows16(x)), precision="f16x3").cpu().numpy()
    ref = orc.Mlp(sd).forward(x, f64=True)[:, 0]
    d = np.abs(y - ref)
    row = int(d.argmax())
    # every column of this layer carries one output row's weight: name the row of the batch and the input that dominates it
    print(f"layer {layer}: max |occ - float64| = {d.max():.3e} at row {row} (largest input of that row: channel {int(np.abs(x[row]).argmax())}; "
          f"|ref| up to {np.abs(ref).max():.2f})")
    assert d.max() <= TOL, (layer, row, float(d.max()))


def _set_unfused(on):
    _lib.check(_lib.lib().icon_debug_set_unfused(C.c_int(int(on))), "icon_debug_set_unfused")


def both_paths(eng, feat, res):
    out = {}
    for mode in (True, False):
        try:
            _set_unfused(mode)
            out[mode] = eng.eval_slab(feat, res, 0, res).clone()
        finally:
            _set_unfused(False)
    return out[False], out[True]


@pytest.mark.parametrize("cmap_mode", ["reference", "local"])
@pytest.mark.parametrize("res", [9, 17])
def test_fused_volume_equals_materialising_volume(body, cmap_mode, res):
    from icon_amd.engine import IconQueryEngine
    eng = IconQueryEngine(prior_type="icon", sdf_clip=body.sdf_clip, cmap_mode=cmap_mode)
    eng.set_mesh(T(body.smpl_verts), T(body.smpl_faces), T(body.smpl_cmap), T(body.smpl_vis))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in body.state_dict.items()})
    fused, unfused = both_paths(eng, T(body.features), res)
    assert torch.equal(fused, unfused)
    ref, _ = oracle_query(body, synth.lattice_points(res), cmap_local=(cmap_mode == "local"))
    err = np.abs(fused.cpu().numpy().ravel() - ref).max()
    print(f"icon {cmap_mode} res {res}: max |occ - float64| = {err:.3e}")
    assert err <= TOL, err


@pytest.mark.parametrize("prior", ["pamir", "pifu"])
def test_fused_volume_equals_materialising_volume_vol_priors(prior):
    from icon_amd.engine import IconQueryEngine
    feat, vol, sd = vol_assets(prior)
    eng = IconQueryEngine(prior_type=prior)
    eng.set_regressor({k: torch.from_numpy(v) for k, v in sd.items()})
    if vol is not None:
        eng.set_volume_features(T(vol))
    fused, unfused = both_paths(eng, T(feat), 9)
    assert torch.equal(fused, unfused)
    ref, _ = orc.query_vol(feat, vol, orc.Mlp(sd), synth.lattice_points(9))
    err = np.abs(fused.cpu().numpy().ravel() - ref).max()
    print(f"{prior} res 9: max |occ - float64| = {err:.3e}")
    assert err <= TOL, err


def test_hidden_activation_beyond_the_f16_range_is_redone_in_f32(body):
    """one 256-point call; the inputs of one row are inside f16's range, its layer-0 activations - as the kernel splits them,
    times the packer's activation scale - are beyond it: the flag goes up and the row is recomputed in f32"""
    sd = body.state_dict
    x = np.random.RandomState(8).normal(0, 1, (256, 13)).astype(np.float32)
    x[77] *= 9000.0
    assert np.abs(x).max() < 65504.0
    # the folded layer 0 in float64, and the packer's activation scale for it
    W, B = [], []
    for l, (co, ci) in enumerate(synth.mlp_layer_shapes()):
        w, b = sd[f"filters.{l}.weight"][:, :, 0].astype(np.float64), sd[f"filters.{l}.bias"].astype(np.float64)
        if l < 3:
            s = sd[f"norms.{l}.weight"] / np.sqrt(sd[f"norms.{l}.running_var"].astype(np.float64) + 1e-5)
            w, b = w * s[:, None], (b - sd[f"norms.{l}.running_mean"]) * s + sd[f"norms.{l}.bias"]
        W.append(np.ascontiguousarray(w, np.float32)); B.append(np.ascontiguousarray(b, np.float32))
    img = np.zeros(680 * 512, np.uint16); side = np.zeros(1060, np.float32); inv = np.zeros(3, np.float32); scales = np.zeros(5, np.float32)
    pw = (C.c_void_p * 4)(*[w.ctypes.data for w in W]); pb = (C.c_void_p * 4)(*[b.ctypes.data for b in B])
    _lib.check(_lib.lib().icon_debug_mlp_pack_f16x3(C.c_int(13), pw, pb, _lib.ptr(img), _lib.ptr(side), _lib.ptr(inv), _lib.ptr(scales)))
    h0 = W[0].astype(np.float64) @ x.T.astype(np.float64) + B[0][:, None]
    act = np.maximum(h0, 0.01 * h0) * float(scales[3])
    assert np.abs(act[:, 77]).max() > 65504.0 and np.abs(np.delete(act, 77, 1)).max() < 65504.0
    y = handle(sd).forward(T(rows16(x)), precision="f16x3").cpu().numpy()
    ref = orc.Mlp(sd).forward(x, f64=True)[:, 0]
    assert np.isfinite(y).all()
    d = np.abs(y - ref)
    print(f"ordinary rows: max |occ - float64| = {np.delete(d, 77).max():.3e}; row 77: {d[77]:.3e} of |ref| = {abs(ref[77]):.3e}")
    assert np.delete(d, 77).max() <= TOL                   # the 255 ordinary rows: the bar itself
    assert d[77] <= TOL * max(1.0, abs(ref[77]))           # the redone row is f32 arithmetic on a result of that magnitude

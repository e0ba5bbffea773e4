"""SMPL skinning (icon_amd/smpl.py) - CPU side: the oracle (tests/smpl_oracle.py) pinned to the reference's own
lbs() and SMPL class, live where the reference tree is present and through a stored run elsewhere; SmplModel's tables and
refusals; the gaps the GPU bars are taken from; the host contract of the native entries."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import smpl_oracle as so
import smpl_reference as sr
from icon_amd import _lib

needs_reference = pytest.mark.skipif(not sr.available(), reason="reference tree not present")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smpl_lbs_ref.npz")

# float64 rounding (2^-52 = 2.2e-16) times a few hundred terms per sum (217 blend shapes, up to 55 weights) times the chain depth
# (at most 9 in SMPL's tree, 54 in the straight chains): of order 1e-13 in the worst case; the bar leaves a factor of ten
PIN = 1e-12


def _pinned(got, ref, tag):
    for loss in so.LOSSES:
        for k in so.OUTPUTS:
            g = so.gap(got[loss][k], ref[loss][k])
            print(f"{tag} {loss:6s} {k:10s} gap {g:.2e}")
            assert g <= PIN, (tag, loss, k, g)


@needs_reference
@pytest.mark.parametrize("name,B,identity", so.RUNS)
def test_oracle_equals_the_reference_lbs(name, B, identity):
    """outputs and autograd gradients of the float64 oracle against the reference's own lbs(pose2rot=False) in float64"""
    _pinned(so.run(name, B, torch.float64, 0, identity), sr.run(name, B, 0, identity), f"{name} B={B}")


def test_oracle_equals_the_stored_reference_run():
    """tests/golden/smpl_lbs_ref.npz (tools/make_smpl_golden.py): the reference's float64 run, stored - holds where the tree is absent"""
    z = np.load(GOLDEN)
    for name, B in (("chain3", 1), ("tree", 2)):
        got = so.run(name, B)
        ref = {loss: dict(verts=z[f"{name}.B{B}.verts"], joints=z[f"{name}.B{B}.joints"],
                          **{k: z[f"{name}.B{B}.{loss}.{k}"] for k in ("grad_betas", "grad_rot")}) for loss in so.LOSSES}
        _pinned(got, ref, f"{name} B={B}")


def _pose(name, B, seed, pose2rot):
    """(betas [1,NB], body_pose, global_orient, transl [B,3]) float32 tensors: matrices of the case's inputs or axis-angles"""
    V, J, NB, _ = so.CASES[name]
    betas, rot, _, _ = so.inputs(name, B, seed)
    rs = np.random.RandomState(seed)
    if pose2rot:
        aa = (0.4 * rs.randn(B, J, 3)).astype(np.float32)
        orient, body = torch.from_numpy(aa[:, 0]), torch.from_numpy(aa[:, 1:].reshape(B, -1))
    else:
        orient, body = torch.from_numpy(rot[:, :1]), torch.from_numpy(rot[:, 1:])
    return torch.from_numpy(betas[:1]), body, orient, torch.from_numpy(rs.randn(B, 3).astype(np.float32))


@needs_reference
@pytest.mark.parametrize("pose2rot", [True, False])
@pytest.mark.parametrize("with_transl", [True, False])
def test_module_forward_equals_the_reference_smpl_class(pose2rot, with_transl):
    """smpl_oracle.module_forward on the reference's real SMPL module (built from the body case through data_struct) against that
    module's own forward, in float64: betas of batch 1 against poses of batch 2"""
    smpl = sr.smpl_module("body").double()
    betas, body, orient, transl = (t.double() for t in _pose("body", 2, 3, pose2rot))
    kw = dict(betas=betas, body_pose=body, global_orient=orient, transl=transl if with_transl else None, pose2rot=pose2rot,
              return_full_pose=True)
    with torch.no_grad():
        ref, got = smpl(**kw), so.module_forward(smpl, **kw)
    assert got["vertices"].shape == (2, 6890, 3) and got["joints"].shape == ref.joints.shape and ref.joints.shape[1] > 24
    for k in ("vertices", "joints", "full_pose", "global_orient", "betas", "body_pose"):
        g = so.gap(got[k].numpy(), ref[k].numpy())
        print(f"pose2rot={pose2rot} transl={with_transl} {k:13s} gap {g:.2e}")
        assert g <= PIN, (k, g)
    assert got["transl"] is None and ref.transl is None
    if with_transl:                                                        # it was added: the outputs moved by it
        bare = so.module_forward(smpl, **dict(kw, transl=None))
        assert so.gap((got["vertices"] - bare["vertices"]).detach().numpy(), transl[:, None].expand(2, 6890, 3).numpy()) < 1e-12
    assert so.module_forward(smpl, **dict(kw, return_verts=False, return_full_pose=False))["vertices"] is None


@needs_reference
def test_from_module_reads_the_reference_smpl_class():
    from icon_amd.smpl import SmplModel
    c = so.case("body")
    m = SmplModel.from_module(sr.smpl_module("body"))
    assert (m.V, m.J, m.NB, m.K, m.P) == (6890, 24, 10, 4, 207)
    assert np.array_equal(m.v_template.t().numpy(), c["v_template"]) and np.array_equal(m.shapedirs.permute(2, 1, 0).numpy(), c["shapedirs"])
    assert np.array_equal(m.posedirs.permute(0, 2, 1).reshape(207, -1).numpy(), c["posedirs"])
    assert np.array_equal(m.parents.numpy(), c["parents"]) and np.array_equal(m.lbs_weights().numpy(), c["lbs_weights"])


@pytest.mark.parametrize("name", list(so.CASES))
def test_model_tables(name):
    from icon_amd.smpl import SmplModel
    c = so.case(name)
    V, J, NB, per = so.CASES[name]
    m = SmplModel(*(torch.from_numpy(c[k]) for k in so.BUFFERS))
    assert m.device.type == "cpu" and (m.V, m.J, m.NB, m.P) == (V, J, NB, 9 * (J - 1))
    # K is the row maximum; the sparse rows expand back to lbs_weights bit for bit; joints ascend, padding is (0, 0.0)
    count = (c["lbs_weights"] != 0).sum(1)
    assert m.K == count.max() == (J if per == 0 else min(per, J))
    assert m.skin_idx.dtype == torch.int32 and m.skin_w.dtype == torch.float32 and tuple(m.skin_idx.shape) == (V, m.K)
    assert m.lbs_weights().numpy().tobytes() == c["lbs_weights"].tobytes()
    idx, w = m.skin_idx.numpy(), m.skin_w.numpy()
    for v in range(0, V, max(1, V // 50)):
        n = count[v]
        assert (np.diff(idx[v, :n]) > 0).all() and (w[v, :n] != 0).all() and (idx[v, n:] == 0).all() and (w[v, n:] == 0).all()
    # the blend-shape tables: component-major copies
    assert np.array_equal(m.v_template.numpy(), c["v_template"].T) and m.v_template.is_contiguous()
    assert np.array_equal(m.shapedirs.numpy(), c["shapedirs"].transpose(2, 1, 0))
    assert np.array_equal(m.posedirs.numpy(), c["posedirs"].reshape(-1, V, 3).transpose(0, 2, 1))
    # the joint tables: within one float32 ulp of the float64 products
    Jr = c["J_regressor"].astype(np.float64)
    for got, want in ((m.J_template.numpy(), Jr @ c["v_template"].astype(np.float64)),
                      (m.J_shapedirs.numpy(), np.einsum("jv,vcl->jcl", Jr, c["shapedirs"].astype(np.float64)))):
        assert got.dtype == np.float32 and got.shape == want.shape
        assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    moved = m.to("cpu")
    assert moved is not m and moved.skin_w.data_ptr() != m.skin_w.data_ptr() and torch.equal(moved.skin_w, m.skin_w) and moved.K == m.K


def test_model_with_an_unweighted_vertex_and_a_zero_row():
    """a vertex with no weight at all keeps K >= 1 and a row of padding; a row shorter than K is padded"""
    from icon_amd.smpl import SmplModel
    c = {k: v.copy() for k, v in so.case("chain3").items()}
    c["lbs_weights"][2] = 0
    c["lbs_weights"][3] = (0, 1, 0)
    m = SmplModel(*(torch.from_numpy(c[k]) for k in so.BUFFERS))
    assert m.K == 2 and m.skin_idx[2].tolist() == [0, 0] and m.skin_w[2].tolist() == [0, 0]
    assert m.skin_idx[3].tolist() == [1, 0] and m.skin_w[3].tolist() == [1, 0]
    assert m.lbs_weights().numpy().tobytes() == c["lbs_weights"].tobytes()


def test_model_refusals():
    from icon_amd.smpl import IconAmdError, SmplModel
    base = {k: torch.from_numpy(v) for k, v in so.case("chain3").items()}

    def build(**changed):
        return SmplModel(*(changed.get(k, base[k]) for k in so.BUFFERS))

    build()
    with pytest.raises(IconAmdError, match="parents"):
        build(parents=torch.tensor([-1, 2, 0]))                            # out of order: joint 1 hangs on joint 2
    with pytest.raises(IconAmdError, match="parents"):
        build(parents=torch.tensor([-1, 0, 2]))                            # a joint that is its own parent
    with pytest.raises(IconAmdError, match="parents"):
        build(parents=torch.tensor([0, 0, 1]))                             # parents[0] != -1
    with pytest.raises(IconAmdError, match="parents must be an integer"):
        build(parents=torch.tensor([-1.0, 0.0, 1.0]))
    for k, bad in (("shapedirs", base["shapedirs"][:4]), ("posedirs", base["posedirs"][:9]), ("J_regressor", base["J_regressor"][:, :4]),
                   ("parents", base["parents"][:2]), ("lbs_weights", base["lbs_weights"][:, :2]), ("v_template", base["v_template"][:, :2])):
        with pytest.raises(IconAmdError, match="must be"):
            build(**{k: bad})
    for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights"):
        for bad_value in (float("nan"), float("inf")):
            t = base[k].clone()
            t.view(-1)[1] = bad_value
            with pytest.raises(IconAmdError, match="not finite"):
                build(**{k: t})
    J, V = 65, 3                                                           # one joint more than the kernels are built for
    with pytest.raises(IconAmdError, match="J <= 64"):
        SmplModel(torch.zeros(V, 3), torch.zeros(V, 3, 1), torch.zeros(9 * (J - 1), 3 * V), torch.zeros(J, V), torch.arange(-1, J - 1),
                  torch.zeros(V, J))
    with pytest.raises(IconAmdError, match="NB <= 512"):
        SmplModel(torch.zeros(V, 3), torch.zeros(V, 3, 513), torch.zeros(0, 3 * V), torch.zeros(1, V), torch.tensor([-1]), torch.zeros(V, 1))
    with pytest.raises(IconAmdError, match="has no tensor"):
        SmplModel.from_module(torch.nn.Linear(2, 2))


def test_stand_in_module_and_rodrigues():
    """the stand-in's own forward is module_forward; the package's batch_rodrigues is the oracle's formula, and gives rotations"""
    from icon_amd.smpl import batch_rodrigues
    mod = so.StandIn("chain3", batch_size=2, create_transl=True)
    assert [n for n, _ in mod.named_buffers()][:6] == list(so.BUFFERS)
    out = mod(pose2rot=True)
    assert out["vertices"].shape == (2, 5, 3) and out.joints.shape == (2, 3 + 2, 3) and out["full_pose"] is None
    assert torch.equal(out.joints[:, 3:], out.vertices[:, [0, 3]])
    aa = torch.from_numpy(np.random.RandomState(0).randn(7, 3))
    aa[0] = 0                                                              # the + 1e-8 keeps the zero vector finite
    R = batch_rodrigues(aa)
    assert R.dtype == torch.float64 and torch.isfinite(R).all() and so.gap(R.numpy(), so.rodrigues(aa).numpy()) <= 1e-14
    # the 1e-8 under the norm leaves the axis a few 1e-8 off unit length: rotations to 1e-7, not to rounding
    assert (R @ R.transpose(1, 2) - torch.eye(3)).abs().max() < 1e-7 and (R[0] - torch.eye(3)).abs().max() < 1e-7


def test_gaps_are_the_recorded_ones():
    """the GAP constants of tests/test_gpu_smpl.py are what the float32 run of the oracle on the CPU differs from its float64 run
    by - largest over every run of smpl_oracle.RUNS, the three losses and seeds 0..4 - measured here again (on one thread: one
    summation order on every host).  A constant may lie at most 3 % above what is measured here, so that the device bars stay
    at 4 x gap; a constant below the measurement only tightens the bars."""
    import test_gpu_smpl as tg
    worst = so.measure_gaps()
    assert set(worst) == set(tg.GAP) == set(so.OUTPUTS)
    for k, (g, where) in sorted(worst.items()):
        print(f"{k:12s} float32 oracle against float64: {g:.3e} at {where}; recorded {tg.GAP[k]:.3e}")
    for k, (g, where) in worst.items():
        assert tg.GAP[k] <= 1.03 * g, (k, g, where)
        assert tg.BAR[k] == 4 * tg.GAP[k]


def test_smpl_entries_exist_and_refuse():
    """fails on the parent: there is no icon_amd.smpl and the library has no icon_smpl_*"""
    from icon_amd.smpl import IconAmdError, SmplModel, _Tables, attach, detach, smpl_lbs_device
    L = _lib.lib()
    n = C.c_int64(-1)
    assert L.icon_smpl_bytes(C.c_int64(1), C.c_int64(6890), 24, 10, 4, C.byref(n)) == 0
    assert n.value >= 27 * (12 * 24 + 207 + 10) * 8 and n.value % 256 == 0   # 27 workgroups of partials, float64
    for args, code in (((1, 6890, 65, 10, 4), 3), ((1, 6890, 0, 10, 1), 3), ((1, 6890, 24, 513, 4), 3), ((1, 6890, 24, -1, 4), 3),
                       ((1, 6890, 24, 10, 0), 1), ((1, 6890, 24, 10, 25), 1), ((0, 6890, 24, 10, 4), 1), ((1, 0, 24, 10, 4), 1),
                       ((2 ** 20, 2 ** 11, 24, 10, 4), 3)):
        B, V, J, NB, K = args
        assert L.icon_smpl_bytes(C.c_int64(B), C.c_int64(V), J, NB, K, C.byref(n)) == code, args
    assert L.icon_smpl_bytes(C.c_int64(2 ** 20), C.c_int64(2 ** 11 - 1), 1, 0, 1, C.byref(n)) == 0
    # argument checks come before any launch: they fire without a device
    m = SmplModel(*(torch.from_numpy(so.case("chain3")[k]) for k in so.BUFFERS))
    t = m._tables()
    assert isinstance(t, _Tables) and (t.V, t.J, t.NB, t.K, t.P) == (5, 3, 1, 2, 18)
    bad = _Tables.from_buffer_copy(t)
    bad.P = 9
    dummy = C.c_void_p(256)                                                # never dereferenced: every call below is refused first
    assert L.icon_smpl_forward(C.byref(bad), dummy, dummy, C.c_int64(1), dummy, dummy, dummy, None) == 1
    assert b"9 (J - 1)" in L.icon_last_error()
    assert L.icon_smpl_forward(C.byref(t), dummy, dummy, C.c_int64(1), None, dummy, dummy, None) == 1
    assert b"null output" in L.icon_last_error()
    assert L.icon_smpl_backward(C.byref(t), dummy, dummy, C.c_int64(1), dummy, None, None, dummy, dummy, dummy, C.c_int64(0), None) == 1
    assert b"smaller than icon_smpl_bytes" in L.icon_last_error()
    betas, rot, _, _ = (torch.from_numpy(a) for a in so.inputs("chain3"))
    with pytest.raises(IconAmdError, match="float32"):
        smpl_lbs_device(betas.double(), rot, m)
    with pytest.raises(IconAmdError, match="rot_mats must be"):
        smpl_lbs_device(betas, rot[:, :2], m)
    with pytest.raises(IconAmdError, match="betas must be"):
        smpl_lbs_device(betas.repeat(1, 2), rot, m)
    with pytest.raises(IconAmdError, match="SmplModel"):
        smpl_lbs_device(betas, rot, None)
    if not torch.cuda.is_available():
        with pytest.raises(IconAmdError, match="no CPU fallback"):
            smpl_lbs_device(betas, rot, m)
    mod = so.StandIn("chain3")
    own = mod.forward
    attach(mod)
    assert mod.forward is not own and isinstance(mod.icon_amd_smpl, SmplModel)
    with pytest.raises(IconAmdError, match="attached already"):
        attach(mod)
    detach(mod)
    assert mod.forward == own and not hasattr(mod, "icon_amd_smpl")
    with pytest.raises(IconAmdError, match="not attached"):
        detach(mod)

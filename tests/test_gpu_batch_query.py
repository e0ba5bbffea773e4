"""GPU: query() at batch size B > 1 (icon_query_points_batch) - HGPIFuNet.query's batched contract (lib/net/HGPIFuNet.py:268-367).

The reference fixtures (tools/make_golden_batch.py) pin the batch-global outlier cmap list; the other tests pin the batched path
against the B = 1 path bit for bit where the semantics coincide (cmap_mode 'local'), the fused kernel against the materialising
path, the refusals, and the face check of a subject set."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_subjects as bs  # noqa: E402
from common import golden  # noqa: E402
from icon_amd import _lib  # noqa: E402
from icon_amd._lib import IconAmdError  # noqa: E402
from icon_amd.engine import IconQueryEngine  # noqa: E402

pytestmark = pytest.mark.gpu
OCC_TOL = 1e-4
DEV = torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def engine(variant="full", B=bs.B_GOLDEN, cmap_mode="reference", precision="f16x3", S=None):
    feats, C, size, stacks, prior = bs.VARIANTS[variant]
    eng = IconQueryEngine(prior_type=prior, sdf_clip=0.05, smpl_feats=feats or ("sdf", "norm", "vis", "cmap"),
                          cmap_mode=cmap_mode, precision=precision)
    S = S if S is not None else bs.subjects(B)
    if prior == "icon":
        eng.set_mesh(T(S["smpl_verts"]), T(S["smpl_faces"]), T(S["smpl_cmap"]), T(S["smpl_vis"]))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in bs.state_dict(variant).items()})
    feats_t = [T(bs.planes(B, C, size, k)) for k in range(stacks)]
    return eng, S, feats_t


def world_points(S, n, seed=0):
    """[B,3,n] device points"""
    return T(bs.candidate_points(S, n, seed).transpose(0, 2, 1))


@pytest.mark.parametrize("variant", list(bs.VARIANTS))
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_batch_matches_reference_fixture(variant, precision):
    inp, out = golden("query_batch_inputs.npz"), golden("query_batch_outputs.npz")
    S = bs.subjects(bs.B_GOLDEN)
    assert bs.sha1(S["smpl_verts"], S["smpl_vis"], S["smpl_cmap"], S["calibs"]) == str(inp["sha1_subjects"])
    eng, _, feats = engine(variant, S=S, precision=precision)
    occ = eng.query(feats, T(inp["points"]), T(inp["calibs"]))
    stacks = bs.VARIANTS[variant][3]
    assert len(occ) == stacks
    for k in range(stacks):
        got = occ[k].cpu().numpy()
        ref = out[f"occ_{variant}_{k}"]
        assert got.shape == ref.shape == (bs.B_GOLDEN, 1, bs.N_GOLDEN)
        err = float(np.abs(got - ref).max())
        assert err <= OCC_TOL, f"{variant} stack {k} ({precision}): max |occ - reference| = {err}"


@pytest.mark.parametrize("B,n", [(4, 8000), (4, 1001), (3, 40000)])
@pytest.mark.parametrize("variant", ["full", "sdf", "pifu"])
def test_local_mode_equals_single_subject_calls(B, n, variant):
    """cmap_mode 'local' has no cross-subject coupling: subject b of the batch is bit for bit a B = 1 call on subject b (B * n
    above kPacketMinPoints takes the Morton + packet search, the B = 1 calls the cooperative one).  The packet case here has
    n = 40,000 = 625 * 64: no subject's segment is padded, so no wave holds a parked lane - the padding of k_nearest_batch is
    covered by tests/test_gpu_batch_oracle.py (n % 64 != 0)"""
    eng, S, feats = engine(variant, B=B, cmap_mode="local")
    pts = world_points(S, n, seed=5)
    calibs = T(S["calibs"])
    batched = eng.query(feats, pts, calibs)
    for b in range(B):
        one = IconQueryEngine(prior_type=eng.prior_type, sdf_clip=0.05, smpl_feats=eng.smpl_feats, cmap_mode="local")
        if eng.prior_type == "icon":
            one.set_mesh(*(T(S[k][b:b + 1]) for k in ("smpl_verts", "smpl_faces", "smpl_cmap", "smpl_vis")))
        one.set_regressor(eng._regressor)
        single = one.query([f[b:b + 1] for f in feats], pts[b:b + 1].contiguous(), calibs[b:b + 1])
        for k in range(len(feats)):
            assert torch.equal(batched[k][b], single[k][0]), f"subject {b} stack {k}: max diff {(batched[k][b] - single[k][0]).abs().max().item()}"


@pytest.mark.parametrize("cmap_mode", ["reference", "local"])
def test_fused_equals_unfused_batched(cmap_mode):
    eng, S, feats = engine("full", B=4, cmap_mode=cmap_mode)
    pts, calibs = world_points(S, 1001, seed=9), T(S["calibs"])
    fused = eng.query(feats, pts, calibs)
    try:
        _lib.lib().icon_debug_set_unfused(1)
        unfused = eng.query(feats, pts, calibs)
    finally:
        _lib.lib().icon_debug_set_unfused(0)
    for a, b in zip(fused, unfused):
        assert torch.equal(a, b)


def test_reference_mode_couples_subjects():
    """the batch-global outlier list: a batched call differs from B = 1 calls on the subjects (lib/net/HGPIFuNet.py:303-305)"""
    eng, S, feats = engine("full", B=4)
    pts, calibs = world_points(S, 8000, seed=1), T(S["calibs"])
    batched = eng.query(feats, pts, calibs)[0]
    one = IconQueryEngine(prior_type="icon", sdf_clip=0.05)
    one.set_regressor(eng._regressor)
    diff = 0.0
    for b in range(1, 4):
        one.set_mesh(*(T(S[k][b:b + 1]) for k in ("smpl_verts", "smpl_faces", "smpl_cmap", "smpl_vis")))
        single = one.query([feats[0][b:b + 1]], pts[b:b + 1].contiguous(), calibs[b:b + 1])[0]
        diff = max(diff, (batched[b] - single[0]).abs().max().item())
    assert diff > 1e-3


def _good_call(eng, S, feats):
    out = eng.query(feats, world_points(S, 300, seed=2), T(S["calibs"]))
    assert out[0].shape == (S["calibs"].shape[0], 1, 300) and torch.isfinite(out[0]).all()
    return out


def test_refusals_leave_the_engine_usable():
    eng, S, feats = engine("full", B=4)
    B = 4
    pts, calibs = world_points(S, 300, seed=2), T(S["calibs"])
    ref = _good_call(eng, S, feats)
    bad = [
        lambda: eng.query(feats, pts, calibs[:1]),                                   # [1,4,4] calib for 4 subjects
        lambda: eng.query([feats[0][:3]], pts, calibs),                              # features of 3 subjects
        lambda: eng.query(feats, pts[:3].contiguous(), calibs[:3]),                  # SMPL batch of 4, points of 3
        lambda: eng.query([f[:2] for f in feats], torch.zeros(1, 3, 1, device=DEV).expand(2, 3, 2 ** 30), calibs[:2]),   # B * N >= 2^31
    ]
    for fn in bad:
        with pytest.raises(IconAmdError):
            fn()
        assert torch.equal(_good_call(eng, S, feats)[0], ref[0])
    for attr, val in (("search", "brute"), ("tie_rule", ("highest", 0))):
        setattr(eng, attr, val)
        with pytest.raises(IconAmdError):
            eng.query(feats, pts, calibs)
        setattr(eng, attr, IconQueryEngine().__dict__[attr])
        assert torch.equal(_good_call(eng, S, feats)[0], ref[0])
    for name, patch in (("_composed_reason", lambda reg, f: "a layout the fused kernels do not carry"),
                        ("_callnorm_spec", lambda reg: object())):
        setattr(eng, name, patch)
        with pytest.raises(IconAmdError):
            eng.query(feats, pts, calibs)
        delattr(eng, name)
        assert torch.equal(_good_call(eng, S, feats)[0], ref[0])
    pam = IconQueryEngine(prior_type="pamir")
    with pytest.raises(IconAmdError):
        pam.query(feats, pts, calibs)
    # a MeshHandle never merges the subjects of a batch
    from icon_amd.engine import MeshHandle
    with pytest.raises(IconAmdError):
        MeshHandle(*(T(S[k]) for k in ("smpl_verts", "smpl_faces", "smpl_cmap", "smpl_vis")))
    assert B == pts.shape[0]


def test_differing_faces_are_reported_on_the_next_poll():
    eng, S, feats = engine("full", B=3)
    faces = S["smpl_faces"].copy()
    faces[2] = np.roll(faces[2], 1, axis=0)                 # same V and F, other topology
    eng.set_mesh(T(S["smpl_verts"]), T(faces), T(S["smpl_cmap"]), T(S["smpl_vis"]))
    eng.query(feats, world_points(S, 300), T(S["calibs"]))  # enqueued without a synchronisation
    with pytest.raises(IconAmdError, match="faces differ"):
        eng.poll_mesh_status(wait=True)
    # a subject set of one topology works again on the same engine
    eng.set_mesh(T(S["smpl_verts"]), T(S["smpl_faces"]), T(S["smpl_cmap"]), T(S["smpl_vis"]))
    _good_call(eng, S, feats)
    eng.poll_mesh_status(wait=True)


def test_attach_with_batched_smpl_feat_dict():
    S = bs.subjects(4)

    class StandIn(nn.Module):           # the attributes HGPIFuNet.query reads (lib/net/HGPIFuNet.py:63-70,236-240)
        prior_type, sdf_clip, smpl_feats = "icon", 0.05, ["sdf", "norm", "vis", "cmap"]

        def __init__(self):
            super().__init__()
            self.if_regressor = {k: torch.from_numpy(v) for k, v in bs.state_dict("full").items()}
            self.smpl_feat_dict = {k: T(S[k]) for k in ("smpl_verts", "smpl_faces", "smpl_cmap", "smpl_vis")}

    net = StandIn()
    IconQueryEngine.attach(net)
    feats = [T(bs.planes(4, 12, 128, k)) for k in range(2)]
    out = net.query(features=feats, points=world_points(S, 2000), calibs=T(S["calibs"]))
    assert [tuple(o.shape) for o in out] == [(4, 1, 2000)] * 2
    assert all(torch.isfinite(o).all() for o in out)

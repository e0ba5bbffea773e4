"""GPU: query() at batch size B > 1 with the pamir prior - HGPIFuNet.query's batched PaMIR branch (lib/net/HGPIFuNet.py:314-354):
every subject's padding stripped with subject 0's counts, every subject voxelised with subject 0's tetrahedra and the one code table,
ve(vol, intermediate_output=False)[-1] -> [B,Cv,32,32,32], and per point [index(im_feat, xy) | index(vol_feat, xyz)] from the
subject's own planes, volume and calibration.

The reference fixture (tools/make_golden_batch_pamir.py) pins the whole chain; the other tests pin the batched path against B = 1
calls bit for bit (nothing in the pamir path is batch-global), the fused kernel against the materialising path, the batched HIP
voxeliser against the single-subject one, the caching of voxelise + encode, the subject-0 rules and the refusals."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_pamir as bp  # noqa: E402
from common import golden, orc, volume_encoder_replica  # noqa: E402
from icon_amd import _lib, synth  # noqa: E402
from icon_amd._lib import IconAmdError  # noqa: E402
from icon_amd.engine import IconQueryEngine  # noqa: E402

pytestmark = pytest.mark.gpu
OCC_TOL = 1e-4            # the bound of the B = 1 real-encoder test (tests/test_voxelize.py)
DEV = torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _regressor():
    from oracle.query_torch import TorchMLP
    reg = TorchMLP().eval()
    reg.norm, reg.last_op = "batch", None
    reg.load_state_dict({k: torch.from_numpy(v) for k, v in bp.state_dict().items()}, strict=False)
    return reg.to(DEV)


def _feat_dict(d):
    return {k: T(v) for k, v in d.items()}


def attached(precision="f16x3", d=None):
    """a network carrying what HGPIFuNet holds for prior_type='pamir' at B = 4 (the fixture's subjects and encoder), attached with
    the HIP voxeliser"""
    g = golden("query_batch_pamir.npz")
    S = bp.subjects(bp.B_GOLDEN)
    ve = volume_encoder_replica().eval()
    ve.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("ve.")}, strict=False)
    netG = SimpleNamespace(prior_type="pamir", sdf_clip=0.05, smpl_feats=["sdf", "norm", "vis", "cmap"], if_regressor=_regressor(),
                           voxelization=SimpleNamespace(smpl_vertex_code=S["code"], volume_res=bp.VOL_RES, sigma=bp.SIGMA), ve=ve.to(DEV),
                           smpl_feat_dict=_feat_dict(d if d is not None else bp.padded(S)))
    eng = IconQueryEngine.attach(netG, voxelizer="hip", precision=precision)
    return netG, eng, g, S


def run(netG, g, S, B=bp.B_GOLDEN):
    return netG.query(features=[T(bp.planes(B))], points=T(g["points"][:B]), calibs=T(S["calibs"][:B]), regressor=netG.if_regressor)


def standalone(vol, precision="f16x3"):
    eng = IconQueryEngine(prior_type="pamir", precision=precision)
    eng.set_regressor({k: torch.from_numpy(v) for k, v in bp.state_dict().items()})
    eng.set_volume_features(vol)
    return eng


def volumes(B, channels=7, seed=0):
    """[B,Cv,32,32,32] device volumes, one per subject"""
    return T(np.concatenate([synth.make_feature_volume(channels, 32, synth.SEED + 71 * b + seed) for b in range(B)]))


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_batch_matches_reference_fixture(precision):
    netG, eng, g, S = attached(precision)
    assert bp.subjects_sha1(S) == str(g["sha1_subjects"])
    occ = run(netG, g, S)
    assert len(occ) == 1 and tuple(occ[0].shape) == (bp.B_GOLDEN, 1, bp.N_GOLDEN)
    vf = eng._volb_cached
    assert tuple(vf.shape) == (bp.B_GOLDEN, 7, 32, 32, 32)
    dv = float(np.abs(vf[:, :, ::4, ::4, ::4].cpu().numpy() - g["vol_feat_sample"]).max())
    d = float(np.abs(occ[0].cpu().numpy() - g["occ"]).max())
    print(f"pamir B=4 ({precision}): max |vol_feat - reference| = {dv:.2e}, max |occ - reference| = {d:.2e}")
    assert dv <= OCC_TOL and d <= OCC_TOL


@pytest.mark.parametrize("B,n", [(4, 8000), (4, 1001), (3, 40000)])
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_subjects_equal_single_subject_calls(B, n, precision):
    """subject b of a batch is bit for bit a B = 1 call given vol_feat[b:b+1] (n = 1001: tiles straddle subject boundaries)"""
    S = bp.subjects(B)
    vol = volumes(B)
    planes = T(bp.planes(B))
    pts = T(bp.candidate_points(S, n, seed=3).transpose(0, 2, 1))
    calibs = T(S["calibs"])
    batched = standalone(vol, precision).query([planes], pts, calibs)[0]
    assert tuple(batched.shape) == (B, 1, n)
    for b in range(B):
        single = standalone(vol[b:b + 1], precision).query([planes[b:b + 1]], pts[b:b + 1].contiguous(), calibs[b:b + 1])[0]
        assert torch.equal(batched[b], single[0]), f"subject {b}: max diff {(batched[b] - single[0]).abs().max().item()}"


def test_fused_equals_unfused_batched():
    S = bp.subjects(4)
    eng = standalone(volumes(4))
    planes, calibs = [T(bp.planes(4))], T(S["calibs"])
    pts = T(bp.candidate_points(S, 1001, seed=9).transpose(0, 2, 1))
    fused = eng.query(planes, pts, calibs)
    try:
        _lib.lib().icon_debug_set_unfused(1)
        unfused = eng.query(planes, pts, calibs)
    finally:
        _lib.lib().icon_debug_set_unfused(0)
    assert torch.equal(fused[0], unfused[0])


@pytest.mark.parametrize("res", [32, 128])
def test_batched_voxeliser_is_the_single_subject_voxeliser(res):
    from icon_amd.engine import semantic_voxelization, semantic_voxelization_batch
    S = bp.subjects(bp.B_GOLDEN)
    vv = T(S["verts"])
    tets = T(S["tets"])
    vol, occ_dev = semantic_voxelization_batch(vv, tets, S["code"], res=res, sigma=bp.SIGMA, return_occ=True)
    assert tuple(vol.shape) == (bp.B_GOLDEN, 3, res, res, res) and tuple(occ_dev.shape) == (bp.B_GOLDEN, res, res, res)
    for b in range(bp.B_GOLDEN):
        one = semantic_voxelization(vv[b:b + 1], tets[None], S["code"], res=res, sigma=bp.SIGMA)
        assert torch.equal(vol[b], one[0]), f"subject {b}"
        got = vol[b].permute(1, 2, 3, 0).cpu().numpy()
        ref, occ = orc.semantic_voxelize(S["verts"][b], len(S["code"]), S["code"], S["tets"], res=res, sigma=bp.SIGMA, return_occ=True)
        assert np.array_equal(np.abs(got).sum(-1) > 0, occ)
        assert np.array_equal(occ_dev[b].cpu().numpy(), occ.astype(np.uint8))                     # the occupancy itself, not inferred
        assert np.abs(got - ref).max() <= 1e-5


def test_voxelise_and_encode_once_per_batch_of_voxel_tensors():
    netG, eng, g, S = attached()
    ve = netG.ve
    first = run(netG, g, S)[0]
    again = run(netG, g, S)[0]
    assert ve.calls == 1 and torch.equal(first, again)
    netG.smpl_feat_dict["voxel_verts"] = netG.smpl_feat_dict["voxel_verts"].clone()       # next batch: new tensors -> recomputed
    assert torch.equal(run(netG, g, S)[0], first)
    assert ve.calls == 2
    # alternating B = 1 (subject 0 alone) and B = 4 calls: each keeps its own volume
    d4 = netG.smpl_feat_dict
    d1 = _feat_dict(bp.padded({k: (v[:1] if k in ("verts", "calibs", "params") else v) for k, v in S.items()}, bp.PAD_V[:1], bp.PAD_F[:1]))
    for _ in range(2):
        netG.smpl_feat_dict = d1
        one = run(netG, g, S, B=1)[0]
        assert float(np.abs(one[0].cpu().numpy() - g["occ"][0]).max()) <= OCC_TOL
        netG.smpl_feat_dict = d4
        assert torch.equal(run(netG, g, S)[0], first)
    assert ve.calls == 3


def test_subject_0_rules():
    """other pad counts and other tetrahedra for subjects 1.. change nothing, as for the reference
    (tests/test_reference_batch_pamir.py)"""
    netG, _, g, S = attached()
    want = run(netG, g, S)[0]
    d = bp.padded(S)
    d["pad_v_num"][1:] = [1, 2, 6]
    d["pad_f_num"][1:] = [1, 3, 2]
    d["voxel_faces"][1:] = np.random.RandomState(4).randint(0, S["verts"].shape[1], d["voxel_faces"][1:].shape)
    netG2, _, _, _ = attached(d=d)
    assert torch.equal(run(netG2, g, S)[0], want)


def test_refusals_leave_the_engine_usable():
    B = 4
    S = bp.subjects(B)
    vol = volumes(B)
    planes, calibs = T(bp.planes(B)), T(S["calibs"])
    pts = T(bp.candidate_points(S, 500, seed=2).transpose(0, 2, 1))
    eng = standalone(vol)
    want = eng.query([planes], pts, calibs)[0]

    def good():
        eng.set_volume_features(vol)
        assert torch.equal(eng.query([planes], pts, calibs)[0], want)

    eng.set_volume_features(vol[:3].contiguous())                       # a B other than the points'
    with pytest.raises(IconAmdError, match="subjects"):
        eng.query([planes], pts, calibs)
    good()
    with pytest.raises(IconAmdError, match="one feature stack"):       # two stacks: eval's zip evaluates one (HGPIFuNet.py:325,329)
        eng.query([planes, planes.clone()], pts, calibs)
    good()
    eng.set_volume_features(volumes(B, channels=9))                     # Cv > 8
    with pytest.raises(IconAmdError, match="8 volume channels"):
        eng.query([planes], pts, calibs)
    good()
    # the C ABI: a batched feature handle without a volume, and a volume of another batch size
    from icon_amd.engine import FeatBatchHandle, _stream
    from icon_amd._lib import check, ptr
    fh = FeatBatchHandle(planes, 1)
    occ = torch.empty(B * 500, device=DEV)
    calib12 = calibs[:, :3, :4].contiguous()
    p = pts.transpose(1, 2).contiguous()
    with pytest.raises(IconAmdError, match="volume"):
        check(_lib.lib().icon_query_points_batch(C.c_void_p(0), fh.h, eng._mlp_handle().h, C.c_int(_lib.PRIOR["pamir"]), C.c_float(0.05),
                                                 C.c_int(0), ptr(calib12), ptr(p), C.c_int64(500), C.c_int(B), ptr(occ), C.c_int(0),
                                                 C.c_int(1), eng._work().h, _stream()), "icon_query_points_batch")
    v3 = vol[:3].contiguous()
    with pytest.raises(IconAmdError, match="number of subjects"):
        check(_lib.lib().icon_feat_batch_set_volume(fh.h, ptr(v3), C.c_int(3), C.c_int(7), C.c_int(32), C.c_int(32), C.c_int(32), _stream()),
              "icon_feat_batch_set_volume")
    fh.close()
    good()

"""CPU: the reference fixture of the batched query() with the pamir prior (tools/make_golden_batch_pamir.py) and the reference
behaviour it pins - every subject stripped with subject 0's pad counts and voxelised with subject 0's tetrahedra
(lib/net/HGPIFuNet.py:316-324), nothing batch-global.  The tests that run the reference skip without its tree, as
tests/test_reference_batch_query.py does."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from oracle import ref_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_pamir as bp  # noqa: E402
from common import volume_encoder_replica  # noqa: E402

needs_reference = pytest.mark.skipif(not ref_loader.available(), reason="reference tree not present")
FIXTURE = os.path.join(ROOT, "tests", "golden", "query_batch_pamir.npz")


def _reference_occ(d):
    import make_golden_batch_pamir as mgp
    S = bp.subjects(bp.B_GOLDEN)
    points = np.load(FIXTURE)["points"]
    with mgp.reference_net() as (netG, _):
        return mgp.run_reference(netG, S, points, d)[0]


@needs_reference
def test_regenerating_reproduces_the_committed_fixture():
    import make_golden_batch_pamir as mgp
    out = mgp.generate()
    g = np.load(FIXTURE)
    assert sorted(g.files) == sorted(out)
    for k, v in out.items():
        assert np.array_equal(g[k], v), k


def test_fixture_inputs_are_the_derived_subjects():
    g = np.load(FIXTURE)
    S = bp.subjects(bp.B_GOLDEN)
    assert np.array_equal(g["calibs"], S["calibs"]) and np.array_equal(g["params"], S["params"])
    assert str(g["sha1_subjects"]) == bp.subjects_sha1(S)
    assert g["points"].shape == (bp.B_GOLDEN, 3, bp.N_GOLDEN) and g["occ"].shape == (bp.B_GOLDEN, 1, bp.N_GOLDEN)
    assert tuple(g["pad_v_num"]) == bp.PAD_V and tuple(g["pad_f_num"]) == bp.PAD_F
    assert len(set(bp.PAD_V)) > 1 and len(set(bp.PAD_F)) > 1          # rule 1 is only pinned by counts that differ


def test_fixture_is_each_subject_on_its_own():
    """nothing in the pamir path is batch-global: subject b of the reference's batched output is the checker's voxeliser ->
    the fixture's encoder -> query_vol on subject b alone (its vertices, the shared tetrahedra and code table, its planes and
    calibration)"""
    g = np.load(FIXTURE)
    S = bp.subjects(bp.B_GOLDEN)
    ve = volume_encoder_replica().eval()
    ve.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("ve.")}, strict=False)
    planes, mlp = bp.planes(bp.B_GOLDEN), orc.Mlp(bp.state_dict())
    for b in range(bp.B_GOLDEN):
        vol = orc.semantic_voxelize(S["verts"][b], len(S["code"]), S["code"], S["tets"], res=bp.VOL_RES, sigma=bp.SIGMA)
        with torch.no_grad():
            vf = ve(torch.from_numpy(vol).permute(3, 0, 1, 2)[None])[-1][0].numpy()
        assert np.abs(vf[:, ::4, ::4, ::4] - g["vol_feat_sample"][b]).max() <= 1e-5
        occ, _ = orc.query_vol(planes[b], vf, mlp, g["points"][b].T, calib=S["calibs"][b])
        assert np.abs(occ - g["occ"][b, 0]).max() <= 1e-5


@needs_reference
def test_reference_strips_every_subject_with_subject_0s_pad_counts():
    """rule 1: voxel_verts[:, :-pad_v_num[0]] / voxel_faces[:, :-pad_f_num[0]] (lib/net/HGPIFuNet.py:316-319) - the other
    entries are never read"""
    S = bp.subjects(bp.B_GOLDEN)
    d = bp.padded(S)
    d["pad_v_num"] = np.array([bp.PAD_V[0], 1, 2, 6], np.int64)
    d["pad_f_num"] = np.array([bp.PAD_F[0], 1, 3, 2], np.int64)
    assert np.array_equal(_reference_occ(d), np.load(FIXTURE)["occ"])


@needs_reference
def test_reference_voxelises_every_subject_with_subject_0s_tetrahedra():
    """rule 2: update_param(smpl_tetra=voxel_faces[0]) (lib/net/HGPIFuNet.py:321-323) - subjects 1.. of voxel_faces are never read"""
    S = bp.subjects(bp.B_GOLDEN)
    d = bp.padded(S)
    d["voxel_faces"][1:] = 0
    assert np.array_equal(_reference_occ(d), np.load(FIXTURE)["occ"])

"""CPU: the batched float64 oracle (tests/batch_oracle.py) is a reference, not a second opinion: at B = 1 it is
orc.query_icon bit for bit, and on the stored batched run of the reference's own HGPIFuNet.query
(tests/golden/query_batch_*.npz, tools/make_golden_batch.py) it meets the bar the single-subject oracle meets against the
reference in tests/test_oracle_vs_reference.py."""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_oracle as bo  # noqa: E402
import batch_subjects as bs  # noqa: E402
from common import golden  # noqa: E402
from icon_amd import synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402

OCC_TOL = 1e-4
SDF_CLIP = 0.05


@pytest.mark.parametrize("cmap_local", [False, True])
def test_one_subject_is_query_icon_bit_for_bit(cmap_local):
    S = bs.subjects(3)
    S1 = {k: v[2:3] for k, v in S.items()}                   # a subject with a non-identity calibration
    planes = bs.planes(3, 12, 128)[2:3]
    mlp = orc.Mlp(bs.state_dict("full"))
    pts = synth.stratified_points(S1["smpl_verts"][0], S1["smpl_faces"][0], 3000, seed=17)
    ref, _ = orc.query_icon(S1["smpl_verts"][0], S1["smpl_faces"][0], S1["smpl_cmap"][0], S1["smpl_vis"][0], planes[0], mlp, pts,
                            sdf_clip=SDF_CLIP, calib=S1["calibs"][0], f64=True, cmap_local=cmap_local)
    occ, K, counts = bo.batch_query_icon(S1, planes, mlp, pts[None], SDF_CLIP, cmap_local)
    assert occ.shape == (1, 3000) and 0 < K == counts[0] < 3000
    assert np.array_equal(occ[0].view(np.int32), ref.view(np.int32))
    sub = np.random.RandomState(0).permutation(3000)[:500]   # a subset, in no order, gives the same rows
    occ_s, K_s, _ = bo.batch_query_icon(S1, planes, mlp, pts[None], SDF_CLIP, cmap_local, subset=sub)
    assert K_s == K and np.array_equal(occ_s.view(np.int32), ref[sub].view(np.int32))


@lru_cache(maxsize=None)
def _fixture_run(variant, stack):
    inp = golden("query_batch_inputs.npz")
    S = bs.subjects(bs.B_GOLDEN)
    feats, C, size, _, _ = bs.VARIANTS[variant]
    pts = np.ascontiguousarray(inp["points"].transpose(0, 2, 1))
    return bo.batch_query_icon(S, bs.planes(bs.B_GOLDEN, C, size, stack), orc.Mlp(bs.state_dict(variant)), pts, float(inp["sdf_clip"]),
                               False, smpl_feats=feats)


@pytest.mark.parametrize("variant,stack", [("full", 0), ("full", 1), ("sdf", 0), ("nofilter", 0)])
def test_reproduces_the_reference_fixture(variant, stack):
    ref = golden("query_batch_outputs.npz")[f"occ_{variant}_{stack}"]
    occ, K, counts = _fixture_run(variant, stack)
    assert occ.shape == (bs.B_GOLDEN, bs.N_GOLDEN) and K == counts.sum()
    err = float(np.abs(occ - ref[:, 0]).max())
    print(f"{variant} stack {stack}: max |batched oracle - reference| = {err:.3e}, K = {K}, per subject {counts.tolist()}")
    assert err <= OCC_TOL
    # the helper restored the oracle's feature selection
    assert orc.lib().orc_icon_c0(12) == 13


def test_batch_global_list_couples_subjects():
    """as test_batch_global_cmap_tiling_couples_subjects shows for the reference: the batched result is not the concatenation of
    B = 1 results, for every subject behind the first"""
    inp = golden("query_batch_inputs.npz")
    S = bs.subjects(bs.B_GOLDEN)
    mlp = orc.Mlp(bs.state_dict("full"))
    planes = bs.planes(bs.B_GOLDEN, 12, 128)
    pts = np.ascontiguousarray(inp["points"].transpose(0, 2, 1))
    batched, K, counts = _fixture_run("full", 0)
    single = [bo.batch_query_icon({k: v[b:b + 1] for k, v in S.items()}, planes[b:b + 1], mlp, pts[b:b + 1], SDF_CLIP, False)
              for b in range(bs.B_GOLDEN)]
    assert [s[1] for s in single] == counts.tolist()
    for b in range(1, bs.B_GOLDEN):
        assert np.abs(batched[b] - single[b][0][0]).max() > 1e-3, b

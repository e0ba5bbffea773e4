"""CPU: the reference fixtures of the batched query() (tools/make_golden_batch.py) and the reference behaviour they pin.
Needs the reference tree (oracle/ref_loader.py); skips without it, as tests/test_oracle_vs_reference.py does."""
import os
import sys

import numpy as np
import pytest

from oracle import ref_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_subjects as bs  # noqa: E402

needs_reference = pytest.mark.skipif(not ref_loader.available(), reason="reference tree not present")


@needs_reference
def test_regenerating_reproduces_the_committed_fixtures():
    import make_golden_batch as mgb
    inp, out = mgb.generate()
    for name, d in (("query_batch_inputs.npz", inp), ("query_batch_outputs.npz", out)):
        g = np.load(os.path.join(ROOT, "tests", "golden", name))
        assert sorted(g.files) == sorted(d)
        for k, v in d.items():
            assert np.array_equal(g[k], v), (name, k)


@needs_reference
def test_batch_global_cmap_tiling_couples_subjects():
    """smpl_cmap[outlier.repeat(1,1,3)] = smpl_sdf[outlier].repeat(1,1,3) (lib/net/HGPIFuNet.py:303-305) tiles the outliers of
    ALL subjects: the batched reference output is not the concatenation of per-subject B = 1 runs"""
    import make_golden_batch as mgb
    S = bs.subjects(bs.B_GOLDEN)
    points = np.load(os.path.join(ROOT, "tests", "golden", "query_batch_inputs.npz"))["points"]
    with mgb.reference() as ref:
        batched = mgb.run_reference(ref, S, points, "full")[0]
        single = np.concatenate([mgb.run_reference(ref, S, points, "full", subjects=[b])[0] for b in range(bs.B_GOLDEN)])
    assert np.abs(batched[1:] - single[1:]).max() > 1e-3


def test_fixture_inputs_are_the_derived_subjects():
    g = np.load(os.path.join(ROOT, "tests", "golden", "query_batch_inputs.npz"))
    S = bs.subjects(bs.B_GOLDEN)
    assert np.array_equal(g["calibs"], S["calibs"]) and np.array_equal(g["params"], S["params"])
    assert str(g["sha1_subjects"]) == bs.sha1(S["smpl_verts"], S["smpl_vis"], S["smpl_cmap"], S["calibs"])
    assert g["points"].shape == (bs.B_GOLDEN, 3, bs.N_GOLDEN)

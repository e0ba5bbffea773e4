"""The marching-cubes cases of tests/mc_cases.py on the CPU: the HOST implementation (icon_export_mesh) against the independent
classic one (oracle/mc_classic.py) on every small and middle size x {noise, at_level, border} x three levels, and the conditions
every case has to meet - so that the generators and the comparison are known to work, and no GPU test of
tests/test_gpu_mc_sizes.py can pass on a case that holds nothing."""
import numpy as np
import pytest

import mc_cases as mc
from icon_amd.recon import export_mesh_numpy
from oracle import mc_check


@pytest.mark.parametrize("level_id", mc.LEVELS)
@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("res", mc.SIZES_SMALL + mc.SIZES_MID)
def test_host_marching_cubes_vs_classic(res, kind, level_id):
    """export_mesh_numpy == the classic algorithm: same vertex set, same triangles with their winding, nothing flipped, nothing on
    one side only; the float32 vertices within the derived bound (mc_cases.vertex_bound) of the float64 ones.  The checker gets
    the level as the library does (a c_float)."""
    vol, level = mc.case(kind, res, level_id)
    assert vol.dtype == np.float32 and vol.shape == (res, res, res) and np.isfinite(vol).all()
    v, f = export_mesh_numpy(vol, level)
    cv, cf = mc.classic_mesh(vol, level)
    c = mc.compare_with_classic(v.numpy(), f.numpy(), cv, cf, mc.vertex_bound(res))
    mc.assert_same_as_classic(c)
    if not (kind == "border" and res == 3):
        assert len(cf) > 0                                     # (a 2^3 cropped grid is all shell: see the border condition below)
    # the table-free vertex set: every crossed lattice edge, once
    assert len(cv) == len(mc_check.edge_crossings(vol, mc.f32_level(level)))


def test_comparison_sees_a_flip_a_missing_face_and_a_moved_vertex():
    """mc_cases.compare_with_classic on meshes that differ: it has to say so, and how"""
    vol, level = mc.case("at_level", 12, "0.5")
    cv, cf = mc.classic_mesh(vol, level)
    v = cv.astype(np.float32)
    b = mc.vertex_bound(12)
    perm = np.random.RandomState(0).permutation(len(v))
    c = mc.compare_with_classic(v[perm], np.argsort(perm)[cf][::-1][:, [1, 2, 0]], cv, cf, b)     # another order: the same mesh
    mc.assert_same_as_classic(c)
    c = mc.compare_with_classic(v, cf[:, [0, 2, 1]], cv, cf, b)
    assert c["flipped"] > 0.5 * len(cf) and c["only_ours"] == 0 and c["only_theirs"] == 0     # (the rest: two corners in one place)
    nv, nf = mc.classic_mesh(*mc.case("noise", 12, "0.5"))
    c = mc.compare_with_classic(nv.astype(np.float32), nf[:, [0, 2, 1]], nv, nf, b)
    assert c["flipped"] == len(nf) and c["only_ours"] == 0 and c["only_theirs"] == 0
    c = mc.compare_with_classic(v, cf[:-3], cv, cf, b)
    assert c["only_theirs"] == 3 and c["only_ours"] == 0 and c["flipped"] == 0
    moved = v.copy()
    moved[5, 0] += 3 * b
    c = mc.compare_with_classic(moved, cf, cv, cf, b)
    assert not c["same_vertex_set"] and c["max_vertex_diff"] > b
    c = mc.compare_with_classic(np.concatenate([v, v[:1]]), cf, cv, cf, b)
    assert not c["same_vertex_set"]


@pytest.mark.parametrize("level_id", mc.LEVELS)
@pytest.mark.parametrize("res", mc.SIZES_MID + mc.SIZES_SMALL[-2:])
def test_noise_cases_hold_every_configuration(res, level_id):
    """every noise volume with res >= 34 contains all 256 cube configurations (17 and 18: at least every ambiguous face)"""
    vol, level = mc.case("noise", res, level_id)
    idx = mc.config_index(vol, level)
    if res >= 34:
        assert len(np.unique(idx)) == 256
    else:
        assert len(np.unique(idx)) > 200


@pytest.mark.parametrize("level_id", mc.LEVELS)
@pytest.mark.parametrize("res", mc.SIZES_SMALL + mc.SIZES_MID)
def test_at_level_cases_have_a_sample_at_the_level_on_a_crossed_edge(res, level_id):
    vol, level = mc.case("at_level", res, level_id)
    crop = vol[1:, 1:, 1:]
    at = crop == np.float32(level)
    assert at.any()
    hit = 0
    for ax, crossed in mc.crossed_edges(vol, level).items():
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        hit += int((crossed & (at[tuple(lo)] | at[tuple(hi)])).sum())
    assert hit >= 1
    if res >= 8:
        assert hit >= 20                                       # t = 0 and t = 1, on every axis, many times over


@pytest.mark.parametrize("level_id", mc.LEVELS)
@pytest.mark.parametrize("res", mc.SIZES_SMALL + mc.SIZES_MID)
def test_border_cases_cross_into_the_last_row_column_and_plane(res, level_id):
    """crossed edges that END on x = n - 1, on y = n - 1 and on z = n - 1 (n = res - 1 points per axis of the cropped grid):
    the cubes next to the points whose corner strides the classify kernels clamp.  res = 3 is the exception the generator's
    definition forces: its cropped grid is 2^3 points, all of them shell - the case is the EMPTY one (nothing inside, no mesh)."""
    vol, level = mc.case("border", res, level_id)
    n = res - 1
    c = mc.crossed_edges(vol, level)
    if res == 3:
        assert not (vol[1:, 1:, 1:] > np.float32(level)).any() and not any(a.any() for a in c.values())
        return
    assert c[2][:, :, n - 2].any() and c[1][:, n - 2, :].any() and c[0][n - 2, :, :].any()
    # ... and the shell itself holds none: the surface is closed inside the grid
    assert not c[1][:, :, n - 1].any() and not c[0][:, :, n - 1].any()
    assert not c[0][:, n - 1, :].any() and not c[2][:, n - 1, :].any() and not c[1][n - 1, :, :].any() and not c[2][n - 1, :, :].any()


@pytest.mark.parametrize("res", [37, 50] + mc.SIZES_SCAN)
def test_slab_sparse_has_empty_and_full_layer_ranges(res):
    """at least one z range of three or more cell layers without any crossing, and at least one with crossings"""
    per = mc.layer_crossings(mc.slab_sparse(res), 0.5)
    empty = per == 0
    assert empty[:3].all() and empty[-3:].all() and (per > 0).sum() >= 3
    first = int(np.flatnonzero(per > 0)[0])
    assert first >= res // 4                                   # the lower quarter holds nothing: a 4-part cut has an empty part


@pytest.mark.parametrize("res", mc.SIZES_SCAN)
def test_scan_sizes_sit_on_the_switch(res):
    """204: 8,170 blocks of 1,024 cells (one-workgroup scan of the block totals), 205 / 206: more than 8,192 (two-pass scan); the
    closed surfaces there are not small"""
    blocks = -(-((res - 1) ** 3) // 1024)
    assert (blocks <= 8192) == (res == 204) and 8100 < blocks < 8500
    for vol in (mc.ellipsoid(res), mc.slab_sparse(res)):
        idx = mc.config_index(vol, 0.5)
        assert int(((idx > 0) & (idx < 255)).sum()) > 20000

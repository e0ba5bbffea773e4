"""query_color (lib/common/render.py:60-84; apps/infer.py:531) - CPU side: the checker the GPU tests compare with
(tests/color_checker.py) is pinned against the reference's own function run verbatim and against the committed golden, its
sampled branch against float64, and the host contract of the two Python entry points is checked without a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import color_checker as cc
from common import golden
from icon_amd import _lib
from icon_amd.recon import IconAmdError, query_color, query_color_device


@pytest.mark.skipif(not cc.reference_available(), reason="needs the reference tree")
@pytest.mark.parametrize("mesh", ["body", "ico", "ico_offset", "fan"])
def test_checker_equals_the_reference_function_run_verbatim(mesh):
    """both sides run the same torch operators on the same leaves: equality.  Pins the corner swap, the sign of z, the y flip,
    the always-marked last face and the 0..255 scale."""
    v, f = (cc.MESHES.get(mesh) or cc.fan)()
    image = cc.make_image()
    want = cc.reference_query_color()(torch.from_numpy(v), torch.from_numpy(f), image, "cpu")
    got, vis = cc.checker_query_color(v, f, image)
    cc.assert_both_branches(vis)
    assert want.dtype == torch.float32 and want.shape == (len(v), 3) and want.device.type == "cpu"
    assert np.array_equal(got.numpy(), want.numpy())


def test_checker_pins_each_convention_of_the_call():
    """what would go unnoticed if the checker and the code under test shared a mistake: each convention changes the answer"""
    v, f = cc.ico()
    image = cc.make_image()
    col, vis = cc.checker_query_color(v, f, image)
    frac = cc.assert_both_branches(vis)
    assert vis[f[-1]].all()                                                     # faces[-1]: always marked
    # un-swapped corners show the other side; together the two sets cover the sphere
    vis_unswapped = cc.orc.visibility(v[:, :2], v[:, 2], f, 4096)[:, 0]
    assert ((vis != 0) | (vis_unswapped != 0)).mean() > 0.99 and abs((vis_unswapped != 0).mean() - frac) < 0.2
    assert not np.array_equal(vis, vis_unswapped)
    # the visible vertices are the ones that look along +z (z is passed as it is; get_visibility negates it)
    n = cc.orc.vertex_normals(v, f)
    # (a convex mesh: nothing is occluded; only vertices on the silhouette - and faces[-1] - can fall on either side)
    last = np.zeros(len(v), bool); last[f[-1]] = True
    assert (vis[n[:, 2] > 0.5] != 0).all() and (vis[(n[:, 2] < -0.5) & ~last] == 0).all()
    # y is flipped before sampling: sampling at (x, y) gives other colours where the vertex is visible
    unflipped = (torch.nn.functional.grid_sample(image, torch.from_numpy(v[None, :, None, :2].copy()), align_corners=True)[0, :, :, 0].t() + 1) * 0.5 * 255
    assert np.abs(unflipped.numpy() - col.numpy())[vis != 0].max() > 10
    assert np.array_equal(col.numpy()[vis == 0], ((torch.from_numpy(n) + 1.0) * 0.5 * 255.0).numpy()[vis == 0])
    assert 0.0 <= col.min() and col.max() <= 255.0


@pytest.mark.parametrize("mesh", ["body", "ico"])
def test_checker_equals_the_golden(mesh):
    """tests/golden/query_color_ref.npz (tools/make_golden_color.py): the verbatim run, stored - holds where the tree is absent"""
    g = golden("query_color_ref.npz")
    v, f = cc.MESHES[mesh]()
    image = cc.make_image()
    assert np.array_equal(image.numpy(), g["image"])
    col, vis = cc.checker_query_color(v, f, image)
    cc.assert_both_branches(vis)
    assert np.array_equal(vis.astype(np.uint8), g[f"{mesh}_vis"])
    assert np.array_equal(col.numpy(), g[f"{mesh}_colors"])


def test_checker_sampled_branch_vs_float64():
    """the float32 sampled branch (torch's CPU grid_sample) against a float64 numpy restatement on every test mesh.  Measured:
    body 6.07e-4, icosphere 5.00e-4, offset icosphere 5.83e-4, fan 5.12e-4, bumped level-7 icosphere 6.75e-4 colour units;
    color_checker.SAMPLED_F64_FIGURE = 6.8e-4 is that maximum and 4 x it is the bar of the GPU tests."""
    image = cc.make_image()
    worst = 0.0
    for name, fn in list(cc.MESHES.items()) + [("fan", cc.fan), ("bumpy_ico", cc.bumpy_ico)]:
        v, f = fn()
        col, vis = cc.checker_query_color(v, f, image)
        cc.assert_both_branches(vis)
        d = float(np.abs(col.numpy().astype(np.float64) - cc.sampled_branch_f64(v, image))[vis != 0].max())
        print(f"{name}: max |float32 - float64| on the sampled branch = {d:.3e}")
        worst = max(worst, d)
    assert 0.5 * cc.SAMPLED_F64_FIGURE <= worst <= cc.SAMPLED_F64_FIGURE, worst


def test_zero_padding_case_has_visible_vertices_outside_the_image():
    v, f = cc.ico_offset()
    col, vis = cc.checker_query_color(v, f, cc.make_image())
    outside = (np.abs(v[:, :2]) > 1.0 + 2.0 / 63).any(1)                        # more than a pixel (2 / (W - 1)) outside: every tap is padding
    assert (outside & (vis != 0)).sum() >= 10
    assert (col.numpy()[outside & (vis != 0)] == 127.5).all()                   # (0 + 1) * 0.5 * 255


def test_fan_apex_takes_the_normal_branch_and_its_sum_depends_on_the_order():
    v, f = cc.fan()
    _, vis = cc.checker_query_color(v, f, cc.make_image())
    assert vis[0] == 0 and (f == 0).sum() >= 1000
    tri = v[f[(f == 0).any(1)]]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).astype(np.float32)
    fwd, rev = np.zeros(3, np.float32), np.zeros(3, np.float32)
    for a, b in zip(fn, fn[::-1]):
        fwd += a; rev += b
    assert not np.array_equal(fwd, rev)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device behaviour")
def test_fails_loudly_without_device():
    v, f = cc.ico()
    image = cc.make_image()
    with pytest.raises(IconAmdError, match="no CPU fallback"):
        query_color(torch.from_numpy(v), torch.from_numpy(f), image)
    with pytest.raises(IconAmdError, match="no CPU fallback"):
        query_color_device(torch.from_numpy(v), torch.from_numpy(f), image)


def test_bad_arguments_raise():
    v, f = (torch.from_numpy(x) for x in cc.ico())
    image = cc.make_image()
    for fn in (query_color, query_color_device):
        with pytest.raises(IconAmdError, match="batch"):
            fn(v, f, image.repeat(2, 1, 1, 1))
        with pytest.raises(IconAmdError, match="image"):
            fn(v, f, image[0])
        with pytest.raises(IconAmdError, match="image"):
            fn(v, f, image[:, :2])
        with pytest.raises(IconAmdError, match="verts"):
            fn(v[:, :2], f, image)
        with pytest.raises(IconAmdError, match="faces"):
            fn(v, f[:, :2], image)
        with pytest.raises(IconAmdError, match="faces"):
            fn(v, f.float(), image)
    with pytest.raises(IconAmdError, match="out of range"):
        query_color(v, f + len(v), image)
    with pytest.raises(IconAmdError, match="out of range"):
        query_color(v, f - 1, image)


def test_native_entry_refuses_bad_sizes_and_reports_its_scratch():
    lib = _lib.lib()
    n = C.c_int64(0)
    assert lib.icon_query_color_bytes(C.c_int64(275000), C.c_int64(551000), C.c_int(4096), C.byref(n)) == 0
    assert n.value >= 2048 * 2048 * 8 + 551000 * 12                              # the z-buffer and the incidence list at least
    small = C.c_int64(0)
    assert lib.icon_query_color_bytes(C.c_int64(642), C.c_int64(1280), C.c_int(4096), C.byref(small)) == 0 and small.value < n.value
    assert lib.icon_query_color_bytes(C.c_int64(0), C.c_int64(10), C.c_int(4096), C.byref(n)) == 1
    assert lib.icon_query_color_bytes(C.c_int64(10), C.c_int64(10), C.c_int(4095), C.byref(n)) == 1 and b"image_size" in lib.icon_last_error()
    assert lib.icon_query_color_bytes(C.c_int64(10), C.c_int64(10), C.c_int(4096), None) == 1
    assert lib.icon_query_color(None, C.c_int64(3), None, C.c_int64(1), C.c_int(1), None, C.c_int(8), C.c_int(8), C.c_int(4096), None, None,
                                None, C.c_int64(0), None) == 1 and b"null" in lib.icon_last_error()
    assert lib.icon_debug_set_option(b"qc_lanes", C.c_int(7)) == 1 and lib.icon_debug_set_option(b"qc_lanes", C.c_int(0)) == 0


def test_the_two_statements_of_the_s7_set_up_are_the_same_expressions():
    """bilinear_taps (common.h, used by k_qc_shade) restates the set-up that gather_planes (geom_device.h) keeps inline, because
    routing the fused MLP kernel through the helper changes its schedule.  Two copies of a bit-exact rule must
    not drift: the six defining expressions are compared as text, names normalised."""
    import os
    import re
    from common import ROOT
    csrc = os.path.join(ROOT, "icon_amd", "csrc")
    helper = open(os.path.join(csrc, "common.h")).read()
    helper = helper[helper.index("BilinearTaps bilinear_taps("):]
    helper = helper[:helper.index("return t;")]
    inline = open(os.path.join(csrc, "geom_device.h")).read()
    inline = inline[inline.index("void gather_planes("):]
    inline = inline[:inline.index("const float4 *base")]

    def exprs(src):
        src = re.sub(r"\bt\.", "", src)
        out = {}
        for name in ("ix", "iy", "nw", "ne", "sw", "se"):
            m = re.search(r"\b%s = ([^;]+);" % name, src)
            assert m, name
            out[name] = re.sub(r"\s+", "", m.group(1))
        return out
    a, b = exprs(helper), exprs(inline)
    assert a == b, (a, b)
    assert a["ix"] == "((x+1.0f)/2.0f)*(float)(W-1)" and a["nw"] == "((float)x1-ix)*((float)y1-iy)"

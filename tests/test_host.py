"""CPU: host logic and the C-ABI surface (no compute calls - there is no GPU here)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from common import ROOT, chamfer
from icon_amd import _lib, synth
from icon_amd.recon import DenseReconEngine, export_mesh_numpy, lattice_coords, slab_bounds


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "icon_amd.h")).read()
    declared = set(re.findall(r"\b(icon_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    lib = _lib.lib()
    for s in _lib.SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.icon_version() == 100


def test_header_is_plain_c():
    """the boundary is a C ABI: the header must compile as C (no torch / C++ types)"""
    src = '#include "icon_amd.h"\nint main(void){return ICON_OK;}\n'
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


def test_every_object_is_compiled_once_with_its_own_flags():
    """round 4 left an orphan recipe line behind a deleted target: mlp_f16x3.o was compiled twice, the shipped
    object with flags meant for another file.  Every object: one compile command, naming its own source."""
    csrc = os.path.join(ROOT, "icon_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    objs = re.search(r"^OBJS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert len(objs) == len(set(objs)) >= 14
    for o in objs:
        r = subprocess.run(["make", "-n", "-B", "-C", csrc, o], capture_output=True, text=True)
        cmds = [l for l in r.stdout.splitlines() if "hipcc" in l]
        assert len(cmds) == 1, (o, cmds)
        assert re.search(r"-c %s\.(hip|cpp) -o %s$" % (o[:-2], o), cmds[0]), cmds[0]
        assert "-fno-honor-nans" not in cmds[0] and "-ffast-math" not in cmds[0]


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device behaviour")
def test_fails_loudly_without_device():
    from icon_amd.engine import IconAmdError, IconQueryEngine, MlpHandle
    assert _lib.device_count() == 0
    a = synth.make_assets("ico")
    with pytest.raises(IconAmdError, match="no CPU fallback"):
        MlpHandle({k: torch.from_numpy(v) for k, v in a.state_dict.items()})
    eng = IconQueryEngine()
    eng.set_mesh(*(torch.from_numpy(x) for x in (a.smpl_verts, a.smpl_faces, a.smpl_cmap, a.smpl_vis)))
    with pytest.raises(IconAmdError):
        eng.query([torch.from_numpy(a.features)], torch.zeros(1, 3, 4), torch.eye(4)[None])


def test_argument_errors_have_messages():
    import ctypes as C
    lib = _lib.lib()
    h = C.c_void_p(0)
    rc = lib.icon_mesh_create(None, C.c_int64(0), None, C.c_int64(0), None, None, None, C.byref(h))
    assert rc == 1 and b"null" in lib.icon_last_error()
    nv, nf = C.c_int64(0), C.c_int64(0)
    assert lib.icon_export_mesh(None, C.c_int(5), C.c_float(0.5), None, C.byref(nv), None, C.byref(nf)) == 1
    # round 5: the test switches are refused by name / range, a fresh workspace has nothing to report (no device needed for either)
    assert lib.icon_debug_set_option(b"no_such_switch", C.c_int(1)) == 1 and b"unknown key" in lib.icon_last_error()
    assert lib.icon_debug_set_option(b"share_ring", C.c_int(3)) == 1 and lib.icon_debug_set_option(b"share_ring", C.c_int(0)) == 0
    assert lib.icon_debug_set_option(None, C.c_int(1)) == 1
    assert lib.icon_work_status(None) == 1
    w = C.c_void_p(0)
    assert lib.icon_work_create(C.byref(w)) == 0 and lib.icon_work_status(w) == 0 and lib.icon_work_destroy(w) == 0
    out = (C.c_double * 4)()
    assert lib.icon_work_profile_detail(None, out) == 1


def test_product_never_touches_the_oracle():
    bad = []
    for dp, _, fs in os.walk(os.path.join(ROOT, "icon_amd")):
        for f in fs:
            if f.endswith((".py", ".hip", ".cpp", ".h", "Makefile")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                if re.search(r"(from|import)\s+oracle|oracle/|liboracle", txt):
                    bad.append(os.path.join(dp, f))
    assert not bad, bad


@pytest.mark.parametrize("res,world", [(257, 8), (257, 2), (257, 3), (33, 8), (9, 8), (513, 8)])
def test_slab_bounds(res, world):
    cover = []
    for r in range(world):
        z0, z1, per = slab_bounds(res, world, r)
        assert 0 <= z0 <= z1 <= res and z1 - z0 <= per
        cover += list(range(z0, z1))
    assert cover == list(range(res))
    sizes = [slab_bounds(res, world, r)[1] - slab_bounds(res, world, r)[0] for r in range(world)]
    assert max(sizes) - min(sizes) <= 1                     # uniform cost: no short tail slab (257 / 8 = 33 + 7 x 32)
    if (res, world) == (257, 8):
        assert sorted(sizes) == [32] * 7 + [33]


def test_cost_weighted_slab_partition():
    """far-field planes cost more per point (nearest-triangle search) than the planes through the body: the
    weighted cut gives the outer ranks fewer planes, every rank about the same cost"""
    from icon_amd.recon import plane_weights, slab_partition
    res, world = 257, 8
    w = plane_weights(res, -0.25, 0.25)
    parts = slab_partition(res, world, w)
    assert parts[0][0] == 0 and parts[-1][1] == res and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
    cost = [w[a:b].sum() for a, b in parts]
    assert max(cost) / min(cost) < 1.08
    sizes = [b - a for a, b in parts]
    assert sizes[0] <= sizes[world // 2] and sizes[-1] <= sizes[world // 2]
    assert slab_partition(9, 16) == slab_partition(9, 16)   # deterministic; more ranks than planes -> empty slabs allowed
    assert sum(b - a for a, b in slab_partition(9, 16)) == 9


def test_lattice_mapping_matches_reference_formula():
    """batch_eval / create_grid3D conventions: x fastest, y flipped"""
    res = 9
    p = lattice_coords(res, torch.tensor([[[-1.0, 1.0, -1.0]]]), torch.tensor([[[1.0, -1.0, 1.0]]]), True, "cpu")[0].numpy()
    assert np.array_equal(p, synth.lattice_points(res))
    assert np.allclose(p[0], [-1, 1, -1]) and np.allclose(p[1], [-0.75, 1, -1]) and np.allclose(p[res], [-1, 0.75, -1])
    assert np.allclose(p[-1], [1, -1, 1])
    for r in (33, 257, 129):
        q = synth.lattice_points(r, 3, 5)
        assert q.shape == (2 * r * r, 3) and np.isclose(q[0, 2], -1 + 2 * 3 / (r - 1))


def test_dense_recon_engine_is_a_module_with_reference_buffers():
    e = DenseReconEngine(query_func=None, b_min=[[-1.0, 1.0, -1.0]], b_max=[[1.0, -1.0, 1.0]],
                         resolutions=[33, 65, 129, 257], align_corners=True, balance_value=0.5, faster=True,
                         visualize=False, debug=False, use_cuda_impl=False, device="cpu")
    assert isinstance(e, torch.nn.Module)
    assert set(e.state_dict()) == {"b_min", "b_max", "resolutions"}
    assert e.resolutions[-1].tolist() == [257, 257, 257] and e._lattice_fast_path(None)
    assert not e._lattice_fast_path(torch.eye(4)[None])
    with pytest.raises(AssertionError):
        DenseReconEngine(resolutions=[32])


def _closed_manifold(v, f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key, rkey = e[:, 0] * len(v) + e[:, 1], e[:, 1] * len(v) + e[:, 0]
    return len(np.unique(key)) == len(key) and set(key) == set(rkey)


def test_marching_cubes_sphere_and_noise():
    R = 49
    idx = np.arange(R, dtype=np.float32)
    Z, Y, X = np.meshgrid(idx, idx, idx, indexing="ij")
    c, r = np.array([24.3, 25.1, 23.7]), 15.2
    occ = (0.5 + (r - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)) * 0.2).astype(np.float32)
    v, f = export_mesh_numpy(occ, 0.5)
    v, f = v.numpy().astype(np.float64), f.numpy()
    assert _closed_manifold(v, f)
    vol = (np.cross(v[f[:, 0]], v[f[:, 1]]) * v[f[:, 2]]).sum() / 6          # outward normals => positive
    assert abs(vol / (4 / 3 * np.pi * r ** 3) - 1) < 0.01
    # vertices are in the cropped grid's (x,y,z) index space (seg3d_lossless.py:585,594)
    assert np.allclose(v.mean(0), c - 1.0, atol=0.05)
    assert np.abs(np.linalg.norm(v - (c - 1.0), axis=1) - r).max() < 0.05
    # heavy noise exercises every ambiguous configuration: still watertight
    rng = np.random.RandomState(0)
    noisy = occ + (rng.rand(*occ.shape).astype(np.float32) - 0.5) * 0.6
    v2, f2 = export_mesh_numpy(noisy, 0.5)
    assert _closed_manifold(v2.numpy(), f2.numpy())
    # nothing above the level -> empty mesh, no error
    v3, f3 = export_mesh_numpy(np.zeros((9, 9, 9), np.float32), 0.5)
    assert len(v3) == 0 and len(f3) == 0


def test_chamfer_definition():
    v, f = synth.icosphere(3)
    c0, p0 = chamfer(v, f, v, f, n=4000)
    assert c0 < 0.1
    c1, _ = chamfer(v, f, v + np.float32([0.01, 0, 0]), f, n=4000)
    assert 0.3 < c1 < 1.2                         # ~0.01 * 100 * (mean |cos|) per direction


def test_synthetic_assets_are_deterministic():
    a, b = synth.make_assets("body"), synth.make_assets("body")
    assert a.smpl_verts.shape == (1, 6890, 3) and a.smpl_faces.shape == (1, 13776, 3)
    assert a.features.shape == (1, 12, 128, 128) and a.smpl_vis.shape == (1, 6890, 1)
    for k in a.state_dict:
        assert np.array_equal(a.state_dict[k], b.state_dict[k])
    assert [a.state_dict[f"filters.{l}.weight"].shape for l in range(4)] == [(512, 13, 1), (256, 512, 1), (128, 269, 1), (1, 141, 1)]
    import hashlib
    h = hashlib.sha1(a.features.tobytes() + a.state_dict["filters.1.weight"].tobytes()).hexdigest()
    assert h == open(os.path.join(ROOT, "tests", "golden", "synth.sha1")).read().strip()


def test_unsupported_regressors_are_refused():
    """lib/net/MLP.py builds BatchNorm / GroupNorm / InstanceNorm / weight_norm variants: eval-mode BatchNorm1d folds,
    weight_norm is a plain layer, Group / InstanceNorm take the per-call path; what is none of these must raise instead of
    silently mis-evaluating.  last_op: None and nn.Sigmoid (cfg.test_mode False) are evaluated, anything else is refused."""
    import torch.nn as nn
    from icon_amd.engine import check_regressor
    from icon_amd._lib import IconAmdError
    from oracle.query_torch import TorchMLP

    ok = TorchMLP().eval()
    ok.norm, ok.last_op = "batch", None
    check_regressor(ok)
    check_regressor({k: v for k, v in ok.state_dict().items()})
    sig = TorchMLP().eval()
    sig.norm, sig.last_op = "batch", nn.Sigmoid()
    check_regressor(sig)
    from icon_amd.engine import regressor_last_op
    assert regressor_last_op(sig) == "sigmoid" and regressor_last_op(ok) is None
    for attr, val in (("norm", "weight"), ("last_op", nn.Tanh())):      # 'weight' WITH norm layers is not something MLP.py builds
        m = TorchMLP().eval()
        m.norm, m.last_op = "batch", None
        setattr(m, attr, val)
        with pytest.raises(IconAmdError):
            check_regressor(m)
    # 'group' / 'instance' take the per-call path (icon_amd/callnorm.py); a module whose norm layers are not what its `norm` says
    from icon_amd.callnorm import spec_of
    m = TorchMLP().eval()
    m.norm, m.last_op = "group", None
    check_regressor(m)
    with pytest.raises(IconAmdError, match="BatchNorm1d"):
        spec_of(m, None, [512, 256, 128])
    m = TorchMLP()
    m.norm, m.last_op = "batch", None
    m.train()
    with pytest.raises(IconAmdError):
        check_regressor(m)
    gn = {"filters.0.weight": torch.zeros(4, 3, 1), "norms.0.weight": torch.ones(4), "norms.0.bias": torch.zeros(4)}
    with pytest.raises(IconAmdError, match="norm_mlp"):
        check_regressor(gn)
    check_regressor(gn, "group")        # a state_dict cannot say what its norms are: the engine's norm_mlp does


@pytest.mark.parametrize("kind", ["group", "instance"])
def test_call_statistics_fold_like_batchnorm(kind):
    """icon_amd/callnorm.py on CPU tensors: the statistics of a call (f32 GEMM passes, float64 sums; with and without the kept
    pre-norm outputs) put into an eval-mode BatchNorm state_dict give the same MLP as Group / InstanceNorm over the call"""
    from icon_amd import callnorm
    from oracle import oracle as orc
    a = synth.make_assets("ico")
    rs = np.random.RandomState(2)
    sd = {k: v for k, v in a.state_dict.items() if k.startswith("filters.")}
    if kind == "group":
        for l, c in enumerate((512, 256, 128)):
            sd[f"norms.{l}.weight"] = rs.uniform(0.5, 1.5, c).astype(np.float32)
            sd[f"norms.{l}.bias"] = rs.normal(0, 0.1, c).astype(np.float32)
    x = rs.normal(0, 1, (5000, 13)).astype(np.float32)
    x[:, 6] = np.sign(x[:, 6])                                  # a clipped sdf channel: far from Gaussian
    rows = np.zeros((5000, 16), np.float32)
    rows[:, :13] = x
    spec = callnorm.spec_of({k: torch.from_numpy(v) for k, v in sd.items()}, kind, [512, 256, 128])
    W = [torch.from_numpy(sd[f"filters.{l}.weight"][:, :, 0]) for l in range(4)]
    b = [torch.from_numpy(sd[f"filters.{l}.bias"]) for l in range(4)]
    means, variances = callnorm.call_statistics(W, b, [False, False, True, True], spec, torch.from_numpy(rows), 13, chunk=1024)
    m2, v2 = callnorm.call_statistics(W, b, [False, False, True, True], spec, torch.from_numpy(rows), 13, chunk=777, keep_bytes=0)   # recompute branch
    for l in range(3):
        assert torch.allclose(means[l], m2[l], rtol=1e-5, atol=1e-6) and torch.allclose(variances[l], v2[l], rtol=1e-5, atol=1e-8)
    bn = callnorm.batchnorm_equivalent({k: torch.from_numpy(v) for k, v in sd.items()}, spec, means, variances)
    got = orc.Mlp({k: v.numpy() for k, v in bn.items()}).forward(x)[:, 0]
    want = orc.CallNormMlp(sd, kind).forward(x)
    assert np.abs(got - want).max() <= 5e-6 * max(1.0, np.abs(want).max())
    # the statistics themselves: layer 0 against a direct evaluation
    y0 = x.astype(np.float64) @ sd["filters.0.weight"][:, :, 0].astype(np.float64).T + sd["filters.0.bias"]
    g = 32 if kind == "group" else 512
    mu = y0.reshape(5000, g, -1).mean(axis=(0, 2)).repeat(512 // g)
    var = y0.reshape(5000, g, -1).var(axis=(0, 2)).repeat(512 // g)
    assert np.allclose(means[0].numpy(), mu, rtol=1e-6, atol=1e-6) and np.allclose(variances[0].numpy(), var, rtol=1e-5, atol=1e-7)


def test_handle_cache_keys_hold_their_tensors():
    """a cached handle is only valid while the tensors its key was made from are alive (otherwise the
    caching allocator can give the next image's features the same address): the engine keeps strong refs"""
    from icon_amd.engine import IconQueryEngine
    src = open(os.path.join(ROOT, "icon_amd", "engine.py")).read()
    for name in ("_mesh_src", "_feat_src", "_mlp_src", "_vol_src"):
        assert re.search(rf"self\.{name}\s*=|self\._\w+_key, self\.{name} =", src), name
    eng = IconQueryEngine()
    assert eng._feat_src is None and eng.precision == "f16x3"


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` (how the driver calls it) starts two ranks under torch.distributed.run itself; in this
    container they stop at rank setup for want of a HIP device - with that message, not with a launcher usage error"""
    import subprocess
    import sys
    env = dict(os.environ, ICON_AMD_DIST_BACKEND="gloo", OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--res", "17",
                        "--no-cpu-baseline", "--no-extras"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    import torch
    if torch.cuda.is_available():
        assert p.returncode == 0, p.stderr[-2000:]
        line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
        import json
        out = json.loads(line)
        assert out["n_gpus"] == 2 and len(out["config"]["rank_stage_ms"]) == 2
    else:
        assert p.returncode != 0
        assert "needs a HIP device" in p.stderr and "launch multi-GPU runs with" not in p.stderr


def test_hot_kernels_do_not_spill():
    """the register budget of the MFMA body is used to the last register (250 of 256): any change that makes hipcc spill shows
    up as scratch traffic on HBM (20 B/lane = 21 MB per 257^3 launch were once introduced by two scalar constants computed in
    the kernel).  Compile the two hot translation units with the resource remarks and require 0 bytes of scratch for the
    icon instantiations of the fused kernel, the standalone f16x3 MLP and the lattice search, at 8 waves / SIMD for the latter."""
    import re
    import shutil
    import subprocess
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "icon_amd", "csrc")

    def remarks(src, exact):
        with tempfile.TemporaryDirectory() as d:
            cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + (["-ffp-contract=off"] if exact else []) + \
                  ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, src), "-o", os.path.join(d, "x.o")]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
            assert p.returncode == 0, p.stdout[-2000:]
            out, name = {}, None
            for line in p.stdout.splitlines():
                m = re.search(r"Function Name: (\S+)", line)
                if m:
                    name = m.group(1); out[name] = {}
                for key in ("ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs"):
                    m = re.search(re.escape(key) + r": (\d+)", line)
                    if m and name:
                        out[name][key] = int(m.group(1))
            return out
    with ThreadPoolExecutor(3) as ex:
        fused, mlp, query = ex.map(lambda a: remarks(*a), [("fused_f16x3.hip", True), ("mlp_f16x3.hip", False), ("query_kernels.hip", True)])
    # k_fused_f16x3<ICON, Src, SMALL> by mangled name: Src::Lattice = 0, Src::Points = 1, Src::Batch = 2 (common.h)
    def icon_of(src):
        return {k: v for k, v in fused.items() if f"k_fused_f16x3ILi0ELNS_3SrcE{src}ELb" in k}
    icon_fused = {**icon_of(0), **icon_of(1)}
    assert len(icon_of(0)) == 2 and len(icon_of(1)) == 2, list(fused)   # lattice / points x (257^3 kernel, small-call variant)
    # the batched icon instantiations (large / small): the scratch size of the copies of the kernel they replaced
    # (profiles/kernel_resources_before.txt) - 0 bytes
    icon_batch = icon_of(2)
    assert len(icon_batch) == 2, list(fused)
    icon_fused.update(icon_batch)
    assert len(icon_fused) == 6 == sum("k_fused_f16x3ILi0E" in k for k in fused), list(fused)
    print({k[-40:]: v for k, v in icon_fused.items()})
    for k, v in {**icon_fused, **{k: v for k, v in mlp.items() if "k_mlp_f16x3" in k}}.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
    # no timing-only experiment switch (wrong results by construction) is left in the product sources: one stray -D in the
    # compiler flags must not be able to ship a broken library (the round-3 variants live in tools/probes/exp_r03/)
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".h", ".hip", ".cpp")):
            text = open(os.path.join(csrc, name)).read()
            assert "defined(ICON_EXP_" not in text and "ifdef ICON_EXP_" not in text, name
    # k_nearest<LATTICE = true, ALT = false, CLAMP>: the 257^3 kernel (CLAMP) and the same launch for "box_clamp" off
    near = {k: v for k, v in query.items() if "k_nearestILb1ELb0ELb" in k}
    assert len(near) == 2
    for k, v in near.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["Occupancy [waves/SIMD]"] == 8, (k, v)


def test_sign_message_bytes():
    """the size of a rank's sign message (recon.sign_message_bytes): a multiple of 8 - the int64 headers of the gathered buffer
    stay aligned - that holds the header and 2 bits per point, which is what icon_grid_slab_features_msg checks; and, for the
    three sizes _forward_sharded / _forward_sharded_ab derive at res 257 in a world of 8 (a whole slab, its first half, an
    'ab' piece), the value the formula written out at those sites gave"""
    from icon_amd.recon import DenseReconEngine, sign_message_bytes, slab_partition
    for n in (0, 1, 3, 4, 5, 31, 32, 33, 257 * 257 * 33):
        b = sign_message_bytes(n)
        assert b % 8 == 0 and b >= 8 + -(-n // 4), (n, b)
    res, world = 257, 8
    per = max(b - a for a, b in slab_partition(res, world, None))
    per_a = (per + 1) // 2
    pa = DenseReconEngine.ab_pieces(res, world)[0]
    assert (per, per_a, pa) == (33, 17, 17)
    for planes in (per, per_a, pa):
        assert sign_message_bytes(planes * res * res) == 8 + ((planes * res * res + 3) // 4 + 7) // 8 * 8
    assert sign_message_bytes(33 * 257 * 257) == 544920 and sign_message_bytes(17 * 257 * 257) == 280720


@pytest.mark.parametrize("mesh", ["ico", "body", "dup"])
def test_host_mesh_builder_invariants(mesh):
    """the host builder (icon_amd/csrc/mesh_build.cpp, the checker of the device build) through icon_debug_host_mesh_build - pure
    host code, no device: every face sits in exactly one leaf, a child's box lies inside its parent's and contains its
    triangles, the depth stays under the bound the traversal stacks are sized for (mesh_rules.h: depth_bound), the
    permutation and its inverse agree, the ray-bin lists are ascending and cover every triangle's cells"""
    import ctypes as C
    from icon_amd import _lib, synth
    if mesh == "dup":           # 3,000 copies of one triangle + a sphere: zero centroid extents, positional splits
        v, f0 = synth.icosphere(2, radius=0.3)
        f = np.concatenate([np.tile(f0[:1], (3000, 1)), f0])
        vs, cm = synth.make_vis_cmap(v, f)
    else:
        a = synth.make_assets(mesh)
        v, f, cm, vs = a.smpl_verts[0], a.smpl_faces[0], a.smpl_cmap[0], a.smpl_vis[0]
    v = np.ascontiguousarray(v, np.float32); f = np.ascontiguousarray(f, np.int64)
    cm = np.ascontiguousarray(np.asarray(cm, np.float32).reshape(-1, 3)); vs = np.ascontiguousarray(np.asarray(vs, np.float32).reshape(-1))
    V, F = len(v), len(f)
    L = _lib.lib()
    lay = (C.c_int64 * 12)()
    _lib.check(L.icon_debug_mesh_layout(C.c_int64(V), C.c_int64(F), lay))
    lay = list(lay)
    ar = np.zeros(lay[11], np.uint8)
    _lib.check(L.icon_debug_host_mesh_build(_lib.ptr(v), C.c_int64(V), _lib.ptr(f), C.c_int64(F), _lib.ptr(cm), _lib.ptr(vs), _lib.ptr(ar), C.c_int64(len(ar))))
    dyn_i, dyn_f = ar[lay[0]:lay[0] + 128].view(np.int32), ar[lay[0]:lay[0] + 128].view(np.float32)
    root, gy, gz = int(dyn_i[0]), int(dyn_i[1]), int(dyn_i[2])
    n_nodes, n_leaves, depth, entries = (int(x) for x in dyn_i[15:19])
    nodes = ar[lay[2]:lay[2] + 64 * F].view(np.float32).reshape(F, 16)
    refs = nodes.view(np.int32)[:, 12:14]
    order = ar[lay[6]:lay[6] + 4 * F].view(np.int32)
    inv = ar[lay[7]:lay[7] + 4 * F].view(np.int32)
    assert sorted(order.tolist()) == list(range(F)) and np.array_equal(inv[order], np.arange(F))
    tri = v[f]
    tlo, thi = tri.min(1), tri.max(1)
    seen = np.zeros(F, bool)
    stack, maxd, nn, nl = [(root, 0, None)], 0, 0, 0
    while stack:
        ref, d, box = stack.pop()
        maxd = max(maxd, d)
        if ref < 0:
            code = ~ref
            b, cnt = code >> 2, (code & 3) + 1
            assert not seen[b:b + cnt].any()
            seen[b:b + cnt] = True
            nl += 1
            if box is not None:
                fs = order[b:b + cnt]
                assert (tlo[fs] >= box[0]).all() and (thi[fs] <= box[1]).all()
        else:
            nn += 1
            lo, hi = nodes[ref, 0:6].reshape(3, 2), nodes[ref, 6:12].reshape(3, 2)
            for s in (0, 1):
                cb = (lo[:, s], hi[:, s])
                if box is not None:
                    assert (cb[0] >= box[0]).all() and (cb[1] <= box[1]).all()
                stack.append((int(refs[ref, s]), d + 1, cb))
    assert seen.all() and (nn, nl, maxd) == (n_nodes, n_leaves, depth)
    bound = min(48 - 2, int(np.ceil(np.log2(max(F, 2)))) + 10)
    assert depth <= bound
    if gy:                       # ray bins: ascending lists; every triangle listed in the cells its (y,z) box covers
        start = ar[lay[8]:lay[8] + 4 * (gy * gz + 1)].view(np.int32)
        slots = ar[lay[9]:lay[9] + 4 * entries].view(np.int32)
        assert start[0] == 0 and start[-1] == entries and (np.diff(start) >= 0).all()
        for c in np.random.RandomState(0).randint(0, gy * gz, 300):
            lst = slots[start[c]:start[c + 1]]
            assert (np.diff(lst) > 0).all()
        y0, z0, y1, z1, iy, iz = (float(x) for x in dyn_f[3:9])
        rs = np.random.RandomState(1)
        for p in rs.randint(0, F, 200):
            fc = order[p]
            cy = int(np.clip(np.floor((np.float32(0.5) * (tlo[fc, 1] + thi[fc, 1]) - np.float32(y0)) * np.float32(iy)), 0, gy - 1))
            cz = int(np.clip(np.floor((np.float32(0.5) * (tlo[fc, 2] + thi[fc, 2]) - np.float32(z0)) * np.float32(iz)), 0, gz - 1))
            c = cz * gy + cy
            assert p in slots[start[c]:start[c + 1]]


def test_python_sources_bind_every_name_they_load():
    """tools/check_names.py over the package, the tests, bench.py and the tools: a GPU-only test that loads a name bound nowhere in
    its module fails on the GPU box only - after the round (the removal of a precision mode left one behind in round 4)"""
    import glob, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = (glob.glob(os.path.join(root, "tests", "*.py")) + glob.glob(os.path.join(root, "icon_amd", "*.py")) +
             glob.glob(os.path.join(root, "tools", "*.py")) + [os.path.join(root, "bench.py"), os.path.join(root, "__graft_entry__.py")])
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_names.py")] + sorted(files), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout


def test_multiply_high_division_is_exact():
    """csrc/geom_device.h udiv_magic / udiv_fast (the tile decode of k_nearest's per-call record): q = mulhi(n, floor(2^32 / d)) is
    floor(n / d) or one less for EVERY 32-bit n - one compare-and-increment repairs it; d == 1 uses 2^32 - 1.  Checked here in
    exact integer arithmetic over the divisors a lattice can produce and adversarial numerators."""
    rng = np.random.RandomState(5)
    ds = list(range(1, 400)) + [2 ** k for k in range(1, 20)] + [2 ** k - 1 for k in range(2, 20)] + [2 ** k + 1 for k in range(2, 20)] \
        + rng.randint(1, 1 << 20, 300).tolist()
    for d in ds:
        m = (1 << 32) // d if d > 1 else (1 << 32) - 1
        assert m < (1 << 32)
        # (runs of consecutive numerators are capped at 6,000: for the large random divisors the multiples +- 1 below carry the cases)
        ns = np.concatenate([np.arange(0, min(4 * d + 4, 6000)), (1 << 32) - 1 - np.arange(0, min(2 * d + 2, 6000)), rng.randint(0, 1 << 32, 200),
                             (rng.randint(0, (1 << 32) // d + 1, 200) * d), (rng.randint(1, (1 << 32) // d + 1, 200) * d - 1)]).astype(np.int64)
        ns = ns[(ns >= 0) & (ns < (1 << 32))].astype(np.uint64)        # n * m < 2^64: exact in uint64
        q = (ns * np.uint64(m)) >> np.uint64(32)
        want = ns // np.uint64(d)
        assert ((q == want) | (q + np.uint64(1) == want)).all(), d
        q = q + ((ns - q * np.uint64(d)) >= np.uint64(d)).astype(np.uint64)
        assert (q == want).all(), d



def test_adaptive_engine_refuses_the_lossless_schedule():
    """Seg3dLossless(faster=False) - the constructor default upstream (lib/common/seg3d_lossless.py:48) - selects _forward
    (:267-478), which is not implemented here: the engine says so instead of running _forward_faster under that name
    (positional form included: faster is the 11th parameter, :37-51).  The dense engine has no schedule and takes either."""
    from icon_amd.recon import AdaptiveReconEngine, DenseReconEngine
    from icon_amd._lib import IconAmdError
    qf = lambda **kw: None
    for kw in (dict(), dict(faster=False)):
        with pytest.raises(IconAmdError, match=r"faster=True.*_forward \(:267-478"):
            AdaptiveReconEngine(query_func=qf, resolutions=[17, 33], align_corners=True, **kw)
    with pytest.raises(IconAmdError, match="lossless"):
        AdaptiveReconEngine(qf, ((-1.0, 1.0, -1.0),), ((1.0, -1.0, 1.0),), (17, 33), 1, 0.5, True, False, False, False, False)
    AdaptiveReconEngine(qf, ((-1.0, 1.0, -1.0),), ((1.0, -1.0, 1.0),), (17, 33), 1, 0.5, True, False, False, False, True)
    AdaptiveReconEngine(query_func=qf, resolutions=[17, 33], align_corners=True, faster=True)
    DenseReconEngine(query_func=qf, resolutions=[17], align_corners=True)
    DenseReconEngine(query_func=qf, resolutions=[17], align_corners=True, faster=True)


def test_attach_refuses_a_network_module_with_maskout_set():
    """lib/net/HGPIFuNet.py:32 `maskout` is a module constant query() reads (:337-342); attach() looks at the module that
    defines type(netG) and refuses a truthy one"""
    import types
    from types import SimpleNamespace
    from icon_amd.engine import IconQueryEngine
    from icon_amd._lib import IconAmdError
    mod = types.ModuleType("fake_hgpifunet")
    mod.maskout = False
    exec("class Net:\n    pass\n", mod.__dict__)
    sys.modules["fake_hgpifunet"] = mod
    try:
        def net():
            n = mod.Net()
            n.prior_type, n.sdf_clip, n.smpl_feats = "icon", 0.05, ("sdf", "norm", "vis", "cmap")
            n.if_regressor = SimpleNamespace(res_layers=(2, 3, 4))
            return n
        n = net()
        eng = IconQueryEngine.attach(n)
        assert n.query == eng.query
        mod.maskout = True
        with pytest.raises(IconAmdError, match="maskout"):
            IconQueryEngine.attach(net())
    finally:
        del sys.modules["fake_hgpifunet"]


def test_fused_kernel_tile_partition_covers_every_tile_once():
    """The tile partition of k_fused_f16x3 (csrc/fused_f16x3.hip: launch_fused_f16x3 + pool_draw), restated on the host: one
    contiguous span per workgroup; the first steal_static tiles of a span are the workgroup's own run, the rest is cut into
    steal_ngrp groups of steal_grp tiles; list x = the groups of the workgroups x, x + 8, ...; ticket t of list x -> workgroup
    x + 8 (t div ngrp), group t mod ngrp (empty for a span one tile shorter than the longest: drawn again).  For random tile
    counts, grid sizes (not multiples of 8, smaller than 8), pool shares and group sizes, with the workgroups drawing in random
    order from random home XCDs: every tile is evaluated exactly once and every list ends exhausted."""
    rng = np.random.RandomState(11)
    for trial in range(400):
        grid = int(rng.choice([1, 3, 7, 8, 9, 31, 64, 200, 256, 304]))
        ntiles = int(grid + 1 + rng.randint(0, 40 * grid)) if trial % 5 else grid + 1
        permille = int(rng.choice([1, 37, 100, 150, 500, 999, 1000]))
        grp = int(rng.choice([1, 2, 3, 8, 127]))
        per, rem = ntiles // grid, ntiles % grid
        pool_len = per * permille // 1000
        seen = np.zeros(ntiles, np.int32)
        span = lambda b: (b * per + min(b, rem), b * per + min(b, rem) + per + (1 if b < rem else 0))
        if pool_len == 0:                                          # the launcher keeps the launch static
            for b in range(grid):
                seen[span(b)[0]:span(b)[1]] += 1
            assert (seen == 1).all()
            continue
        stat, ngrp = per - pool_len, (pool_len + 1 + grp - 1) // grp
        for b in range(grid):
            seen[span(b)[0]:span(b)[0] + min(stat, per)] += 1
        counters = [0] * 8
        masks = [0] * grid

        def draw(b, xcc):
            for s in range(8):
                x = (xcc + s) & 7
                if (masks[b] >> x) & 1:
                    continue
                nwg = (grid - x + 7) >> 3
                while True:
                    t = counters[x]; counters[x] += 1
                    if t >= nwg * ngrp:
                        masks[b] |= 1 << x
                        break
                    k, g = divmod(t, ngrp)
                    wb = x + 8 * k
                    sb, eb = span(wb)
                    a = sb + stat + g * grp
                    if a < eb:
                        return a, min(grp, eb - a)
            return None
        active = list(range(grid))
        home = {b: int(rng.randint(0, 8)) if trial % 3 == 0 else b % 8 for b in range(grid)}
        while active:
            b = active[int(rng.randint(len(active)))]
            got = draw(b, home[b])
            if got is None:
                active.remove(b)
            else:
                assert got[1] <= 127 and got[0] < (1 << 24)        # the packed word: first tile | tiles << 24
                seen[got[0]:got[0] + got[1]] += 1
        assert (seen == 1).all(), (grid, ntiles, permille, grp, np.flatnonzero(seen != 1)[:8])
        assert all(counters[x] >= ((grid - x + 7) >> 3) * ngrp for x in range(8))


def _launcher_steal(ntiles, grid, permille, grp, small=False, count_on_device=False, pool_on_device_count=False):
    """launch_fused_f16x3's choice of partition, from the HOST tile count (a schedule level's bound r^3): None (static) or
    (steal_static, steal_grp, steal_ngrp).  ``pool_on_device_count``: the rule before the fix (a pool whenever pool_len > 0,
    also when the real count lives on the device)."""
    per = ntiles // grid
    pool_len = per * permille // 1000
    if small or (count_on_device and not pool_on_device_count) or pool_len <= 0 or ntiles <= grid:
        return None
    grp = min(grp, 127)
    return per - pool_len, grp, (pool_len + 1 + grp - 1) // grp


def _kernel_tiles(ntiles, grid, steal, rng):
    """k_fused_f16x3 + pool_draw with the DEVICE tile count: per / rem / spans from ``ntiles``, the launcher's ``steal`` and
    ``grid`` as passed; the workgroups draw in random order from random home XCDs -> evaluations per tile"""
    per, rem = ntiles // grid, ntiles % grid
    seen = np.zeros(ntiles, np.int32)
    span = lambda b: (b * per + min(b, rem), b * per + min(b, rem) + per + (1 if b < rem else 0))
    if steal is None:
        for b in range(grid):
            seen[span(b)[0]:span(b)[1]] += 1
        return seen
    stat, grp, ngrp = steal
    for b in range(grid):
        seen[span(b)[0]:span(b)[0] + min(stat, per)] += 1
    counters, masks = [0] * 8, [0] * grid
    active, home = list(range(grid)), rng.randint(0, 8, grid)
    while active:
        b = active[int(rng.randint(len(active)))]
        got = None
        for s in range(8):
            x = (int(home[b]) + s) & 7
            if (masks[b] >> x) & 1:
                continue
            nwg = (grid - x + 7) >> 3
            while got is None:
                t = counters[x]; counters[x] += 1
                if t >= nwg * ngrp:
                    masks[b] |= 1 << x
                    break
                k, g = divmod(t, ngrp)
                sb, eb = span(x + 8 * k)
                a = sb + stat + g * grp
                if a < eb:
                    got = (a, min(grp, eb - a))
            if got is not None:
                break
        if got is None:
            active.remove(b)
        else:
            seen[got[0]:got[0] + got[1]] += 1
    return seen


def test_fused_kernel_tile_partition_with_device_side_count():
    """A level of the coarse-to-fine schedule (csrc/adaptive.hip) launches the fused kernel with N = r^3, an upper bound: the
    launcher sizes the grid and the partition from it, the kernel cuts its spans from the real count it reads on the device
    (FusedGeom::n_dev).  Restated on the host with two tile counts - the bound for the launcher, a random count <= the bound
    for the kernel: every tile is evaluated exactly once under the launcher's rule (a count that lives on the device is
    static).  Fed the rule before it (a pool whenever pool_len > 0), the restatement finds the tiles that fall between a
    span's end and its first pool group: `rem` of them whenever the device-side `per` is below steal_static."""
    rng = np.random.RandomState(12)
    cus = 256
    # the launcher's numbers of a 256-CU device: the 129^3 / 257^3 levels of the [33 .. 513] schedule, default set_steal(150, 2)
    for bound, npts, permille, grp, lost in [(129 ** 3, 100_000, 150, 2, 135), (129 ** 3, 1_500_000, 150, 2, 228),
                                             (257 ** 3, 2_000_000, 150, 2, 133), (129 ** 3, 1_870_000, 150, 2, 0),
                                             (129 ** 3, 1_870_000, 40, 1, 137)]:
        nt_host, nt_dev = -(-bound // 256), -(-npts // 256)
        grid = min(nt_host, cus)
        for before, want in ((True, lost), (False, 0)):
            steal = _launcher_steal(nt_host, grid, permille, grp, count_on_device=True, pool_on_device_count=before)
            seen = _kernel_tiles(nt_dev, grid, steal, rng)
            assert (seen <= 1).all() and int((seen == 0).sum()) == want, (bound, npts, permille, grp, before)
    found = 0
    for trial in range(600):
        grid = int(rng.choice([1, 3, 7, 8, 9, 31, 64, 200, 240, 256]))
        nt_host = int(grid + 1 + rng.randint(0, 40 * grid))
        nt_dev = int(rng.randint(0, nt_host + 1)) if trial % 4 else nt_host
        permille = int(rng.choice([1, 37, 40, 100, 150, 500, 999, 1000]))
        grp = int(rng.choice([1, 2, 3, 8, 127]))
        small = trial % 7 == 0                       # the icon prior's SMALL launches: static whatever the setting
        seen = _kernel_tiles(nt_dev, grid, _launcher_steal(nt_host, grid, permille, grp, small, count_on_device=True), rng)
        assert (seen == 1).all(), (grid, nt_host, nt_dev, permille, grp, np.flatnonzero(seen != 1)[:8])
        # the rule before the fix: exactly the `rem` extra tiles are lost when the device-side per is below steal_static
        before = _launcher_steal(nt_host, grid, permille, grp, small, count_on_device=True, pool_on_device_count=True)
        seen = _kernel_tiles(nt_dev, grid, before, rng)
        per, rem = nt_dev // grid, nt_dev % grid
        lost = rem if before is not None and before[0] > per else 0
        assert (seen <= 1).all() and int((seen == 0).sum()) == lost, (grid, nt_host, nt_dev, permille, grp)
        found += lost > 0
    assert found > 50                                # the random trials do reach the regime that lost tiles

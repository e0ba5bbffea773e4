"""GPU tests of round 3: parity at the headline sizes against the oracle, tie sensitivity of the nearest-triangle
choice (the unpinned kaolin leaf, lib/dataset/mesh_util.py:374-390), the shell skip (in_cube is strict,
lib/net/HGPIFuNet.py:274-275,363), per-device / per-thread state, clean_mesh connectivity."""
import threading

import numpy as np
import pytest
import torch

from common import assets, oracle_query, orc
from icon_amd import synth
from test_gpu_parity import T, dev, make_engine, OCC_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def body():
    return assets("body")


def stratified_sample(occ_flat: torch.Tensor, res: int, n_each: int, seed: int = 1993) -> np.ndarray:
    """uniform points, points around the 0.5 level set (where the mesh comes from) and shell points"""
    rng = np.random.RandomState(seed)
    n = occ_flat.numel()
    uni = rng.randint(0, n, n_each)
    band = torch.nonzero((occ_flat > 0.2) & (occ_flat < 0.8)).reshape(-1).cpu().numpy()
    lvl = band[rng.randint(0, len(band), min(n_each, len(band)))] if len(band) else uni[:0]
    k = rng.randint(0, res, (n_each // 4, 3))
    k[np.arange(len(k)), rng.randint(0, 3, len(k))] = rng.choice([0, res - 1], len(k))
    shell = (k[:, 2].astype(np.int64) * res + k[:, 1]) * res + k[:, 0]
    return np.unique(np.concatenate([uni, lvl, shell])).astype(np.int64)


# ---------------------------------------------------------------------------------------------
# the headline configurations against the oracle itself (not only through invariants)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,n_each", [(257, 24000), (513, 24000)])
def test_headline_lattice_vs_oracle(body, res, n_each):
    """cfg 2 (257^3) and cfg 5's volume (513^3), cmap_mode=reference, f16x3 - the benchmarked mode: the oracle's
    geometry on the WHOLE lattice (the tiled outlier-cmap rule couples every point to the sign list of the call),
    outlier count K and the sign list bit-exact, occupancy against the float64 MLP on a stratified sample <= 1e-4"""
    feat = T(body.features)
    eng = make_engine(body, cmap_mode="reference", precision="f16x3")
    occ = eng.eval_slab(feat, res, 0, res).reshape(-1)
    idx = stratified_sample(occ, res, n_each)
    assert len(idx) >= 50000
    pts = synth.lattice_points(res)
    ref, _ = orc.query_icon_subset(body.smpl_verts[0], body.smpl_faces[0], body.smpl_cmap[0], body.smpl_vis[0], body.features,
                                   orc.Mlp(body.state_dict), pts, idx, sdf_clip=body.sdf_clip, f64=True)
    got = occ[torch.from_numpy(idx).to(occ.device)].cpu().numpy()
    err = np.abs(got - ref)
    assert err.max() <= OCC_TOL, (err.max(), int((err > OCC_TOL).sum()))
    # K and the sign list: the slab's own list, read back
    signs, count = eng.slab_features(feat, res, 0, res)
    k = int(count.item())
    A = orc.Accel(body.smpl_verts[0], body.smpl_faces[0])
    d2, _ = A.nearest(pts)
    ins = A.check_sign(pts)
    sdf = np.where(ins, 1.0, -1.0).astype(np.float32) * (np.sqrt(d2) / np.sqrt(np.float32(3.0)))
    outl = np.abs(sdf) >= np.float32(body.sdf_clip)
    exp = np.sign(sdf[outl]).astype(np.int8)
    assert k == len(exp)
    assert np.array_equal(signs[:k].cpu().numpy(), exp)


# ---------------------------------------------------------------------------------------------
# tie sensitivity
# ---------------------------------------------------------------------------------------------
def tie_point_sets(a):
    v, f = a.smpl_verts[0], a.smpl_faces[0]
    rng = np.random.RandomState(5)
    nrm = orc.vertex_normals(v, f)
    on_vertex_normals = v[::7] + 0.3 * nrm[::7]                       # the vertex is the nearest feature: its whole fan ties
    tri = v[f[::11]]
    edge_mid_off = 0.5 * (tri[:, 0] + tri[:, 1]) + 0.2 * np.cross(tri[:, 1] - tri[:, 0], rng.randn(len(tri), 3)).astype(np.float32)
    return np.concatenate([synth.lattice_points(33), synth.stratified_points(v, f, 6000, seed=4), on_vertex_normals.astype(np.float32),
                           edge_mid_off.astype(np.float32), v[:500]]).astype(np.float32)


@pytest.mark.parametrize("mesh", ["body", "ico"])
def test_tie_flags_vs_oracle(mesh):
    """winner, runner-up and the ulp gap between their squared distances: HIP == oracle, bit for bit"""
    from icon_amd.engine import MeshHandle
    a = assets(mesh)
    pts = tie_point_sets(a)
    h = MeshHandle(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
    g = {k: v.cpu().numpy() for k, v in h.sdf_query_ties(T(pts)).items()}
    _, idx, idx2, ulps = orc.Accel(a.smpl_verts[0], a.smpl_faces[0]).nearest_ties(pts)
    assert np.array_equal(g["face"], idx.astype(np.int32))
    assert np.array_equal(g["ulps"], ulps)
    near = ulps < 255                                               # beyond the reported range the runner-up is not defined
    assert np.array_equal(g["face2"][near], idx2[near].astype(np.int32))
    # the far field of a closed mesh is dominated by ties: vertices and edges are the nearest features
    assert (ulps <= 1).mean() > 0.3
    # and the winner is what the plain query returns
    assert np.array_equal(h.sdf_query(T(pts))["face"].cpu().numpy(), idx)


@pytest.mark.parametrize("ulps", [0, 1, 4])
def test_alternative_tie_rule_vs_oracle(body, ulps):
    """the whole pipeline under the alternative rule (highest index within `ulps` of the minimum) equals the oracle
    under the same rule; it moves far-field values by much more than 1e-4 but not the level set"""
    res = 33
    feat = T(body.features)
    base = make_engine(body).eval_slab(feat, res, 0, res)
    eng = make_engine(body)
    eng.tie_rule = ("highest", ulps)
    alt = eng.eval_slab(feat, res, 0, res)
    orc.set_tie_rule(1, ulps)
    try:
        ref, _ = oracle_query(body, synth.lattice_points(res))
    finally:
        orc.set_tie_rule(0, 0)
    assert np.abs(alt.cpu().numpy().ravel() - ref).max() <= OCC_TOL
    moved = (alt - base).abs() > 1e-4
    assert moved.any(), "the synthetic body has exact far-field ties: the rule must matter somewhere"
    # ... but the surface hardly notices: a handful of voxels change side of the 0.5 level (bench.py reports the same at
    # 257^3: ~1e-3 of the level-set band, mesh Chamfer ~2 % of a voxel)
    flips = int(((alt > 0.5) != (base > 0.5)).sum().item())
    assert flips <= 0.02 * int((base > 0.5).sum().item()), flips
    # switching the rule back restores the definition on the same engine
    eng.tie_rule = None
    assert torch.equal(eng.eval_slab(feat, res, 0, res), base)
    # the explicit-point API follows the same rule (packets over the Morton order)
    eng.tie_rule = ("highest", ulps)
    pts = synth.lattice_points(res)
    q = eng.query([feat], T(pts.T.copy())[None], torch.eye(4, device=dev())[None])[0][0, 0]
    assert torch.equal(q, alt.reshape(-1))


# ---------------------------------------------------------------------------------------------
# shell skip
# ---------------------------------------------------------------------------------------------
def set_shell_skip(on):
    from icon_amd import _lib
    _lib.check(_lib.lib().icon_debug_set_shell_skip(int(on)))


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("cmap_mode", ["reference", "local"])
@pytest.mark.parametrize("res", [3, 5, 17, 33, 65, 129])
def test_shell_skip_equals_masked_evaluation(body, res, cmap_mode, precision):
    """skipping the in_cube shell (search + MLP over the interior only, shell written as 0) == evaluating and masking
    every point, bit for bit, fused and materialising paths, whole lattice and slabs; the sign list is unchanged"""
    feat = T(body.features)
    try:
        set_shell_skip(0)
        e0 = make_engine(body, cmap_mode=cmap_mode, precision=precision)
        full0 = e0.eval_slab(feat, res, 0, res)
        s0, c0 = e0.slab_features(feat, res, 0, res)
        s0 = s0[: int(c0.item())].clone()
        set_shell_skip(1)
        e1 = make_engine(body, cmap_mode=cmap_mode, precision=precision)
        full1 = e1.eval_slab(feat, res, 0, res, out=torch.full((res, res, res), float("nan"), device=dev()))
        s1, c1 = e1.slab_features(feat, res, 0, res)
        assert torch.equal(full0, full1)
        assert int(c0.item()) == int(c1.item()) and torch.equal(s0, s1[: int(c1.item())])
        for v in (full1,):
            assert (v[0] == 0).all() and (v[-1] == 0).all() and (v[:, 0] == 0).all() and (v[:, -1] == 0).all()
            assert (v[:, :, 0] == 0).all() and (v[:, :, -1] == 0).all()
        if cmap_mode == "local" and res >= 5:      # slabs incl. ones that are all shell / start or end on it
            for z0, z1 in [(0, 1), (0, 2), (res - 1, res), (1, res - 1), (res // 2, res)]:
                out = torch.full((z1 - z0, res, res), float("nan"), device=dev())
                assert torch.equal(e1.eval_slab(feat, res, z0, z1, out=out), full0[z0:z1]), (z0, z1)
    finally:
        set_shell_skip(1)


def test_shell_skip_is_not_taken_when_the_body_reaches_the_boundary(body):
    """a body whose bounding box comes closer to the cube's boundary than the clip band is wide: shell points are not
    all clip-band outliers, the engine must evaluate everything (and still equal the oracle)"""
    import copy
    v = body.smpl_verts.copy()
    v[..., 1] *= 1.0 / np.abs(v[..., 1]).max() * 0.97               # |y| up to 0.97: margin 0.03 < 0.05 * sqrt(3)
    a = copy.copy(body)                                             # shallow: the cached assets stay untouched
    a.smpl_verts = v.astype(np.float32)
    res = 33
    eng = make_engine(a)
    occ = eng.eval_slab(T(a.features), res, 0, res).cpu().numpy().ravel()
    ref, _ = oracle_query(a, synth.lattice_points(res))
    assert np.abs(occ - ref).max() <= OCC_TOL
    o = orc.cal_sdf(a.smpl_verts[0], a.smpl_faces[0], a.smpl_cmap[0], a.smpl_vis[0], synth.lattice_points(res))
    sdf = o["sdf"].reshape(res, res, res)
    shell_not_outlier = (np.abs(sdf[:, [0, -1], :]) < np.float32(a.sdf_clip)).sum()
    assert shell_not_outlier > 0, "the construction must put shell points inside the clip band"


def test_fused_kernel_tile_order_is_free(body):
    """the outlier rank of a point comes from the scan over the LINEAR order + the 64-point ballots, so the MLP tiles
    need not be aligned with that order: pieces cut at arbitrary planes reproduce the whole slab (reference mode)"""
    res = 65
    feat = T(body.features)
    eng = make_engine(body)
    full = eng.eval_slab(feat, res, 0, res)
    for z0, z1, cuts in [(0, res, [0, 1, 2, 31, 64, 65]), (7, 50, [7, 8, 29, 50])]:
        eng.slab_features(feat, res, z0, z1)
        if (z0, z1) != (0, res):
            # a slab that is not the whole call: its own list is the call's list (what eval_slab computes for it)
            want = eng.eval_slab(feat, res, z0, z1)
            eng.slab_features(feat, res, z0, z1)
        else:
            want = full
        out = torch.full((z1 - z0, res, res), float("nan"), device=dev())
        for za, zb in zip(cuts[:-1], cuts[1:]):
            eng.slab_finish_gathered(res, z0, z1, None, 0, 1, 0, out=out, za=za, zb=zb)
        assert torch.equal(out, want), (z0, z1)


# ---------------------------------------------------------------------------------------------
# process-wide state
# ---------------------------------------------------------------------------------------------
def test_two_threads_drive_engines_on_the_same_device(body):
    """engines created and used from two host threads (each with its own workspace and stream-ordered launches):
    both reproduce the single-threaded volume"""
    from icon_amd.recon import export_mesh_device
    res = 65
    feat = T(body.features)
    want = make_engine(body).eval_slab(feat, res, 0, res)
    want_mc = export_mesh_device(want, 0.5)
    results, errors = {}, []

    def worker(k):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                eng = make_engine(body)
                for _ in range(3):
                    occ = eng.eval_slab(feat, res, 0, res)
                v, f = export_mesh_device(occ, 0.5)
                torch.cuda.current_stream().synchronize()
                results[k] = (occ, v.shape[0], f.shape[0])
        except Exception as e:                      # surfaced below
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for k in range(2):
        occ, nv, nf = results[k]
        assert torch.equal(occ, want)
        assert (nv, nf) == (want_mc[0].shape[0], want_mc[1].shape[0])


def test_precision_can_be_changed_after_the_first_query(body):
    """assigning eng.precision takes effect on the next call; an unknown one is refused by name"""
    res = 33
    feat = T(body.features)
    eng = make_engine(body, precision="f16x3")
    a = eng.eval_slab(feat, res, 0, res)
    eng.precision = "f32"
    b = eng.eval_slab(feat, res, 0, res)
    assert torch.equal(b, make_engine(body, precision="f32").eval_slab(feat, res, 0, res))
    assert not torch.equal(a, b) and (a - b).abs().max() <= 1e-4
    from icon_amd.engine import IconAmdError
    eng.precision = "mx6"                                     # (rounds 1-3 had this mode; removed in round 4)
    with pytest.raises(IconAmdError, match="unknown precision"):
        eng.eval_slab(feat, res, 0, res)
    eng.precision = "f16x3"
    assert torch.equal(eng.eval_slab(feat, res, 0, res), a)


# ---------------------------------------------------------------------------------------------
# clean_mesh connectivity (trimesh: faces are connected through shared EDGES)
# ---------------------------------------------------------------------------------------------
def test_clean_mesh_splits_components_that_touch_in_one_vertex():
    from icon_amd.recon import clean_mesh, face_components
    # two tetrahedra sharing exactly one vertex (a marching-cubes pinch), the second with one more (isolated) triangle fan
    a = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    b = np.array([[0, 0, 0], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [-1, -1, -1]], np.float32)
    v = np.concatenate([a, b[1:]])                                 # vertex 0 is shared
    fa = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]], np.int64)
    ib = np.array([0, 4, 5, 6, 7])
    fb_local = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 4], [1, 3, 4], [2, 3, 4]], np.int64)
    fb = ib[fb_local]
    f = np.concatenate([fa, fb])
    lab = face_components(T(f), len(v)).cpu().numpy()
    assert len(set(lab[:4])) == 1 and len(set(lab[4:])) == 1 and lab[0] != lab[4], lab
    cv, cf = clean_mesh(T(v), T(f))
    # the larger component (5 vertices) wins; a vertex union-find would have returned all 8 vertices
    assert cv.shape[0] == 5 and cf.shape[0] == 6
    assert cf.dtype == torch.int32 and cv.dtype == torch.float32
    kept = cv.cpu().numpy()[cf.cpu().numpy().astype(np.int64)]
    assert np.array_equal(kept, v[fb])
    # equal vertex counts: the component met first in face order
    cv2, cf2 = clean_mesh(T(v[:7]), T(np.concatenate([fa, ib[fb_local[:3]]])))
    assert np.array_equal(cv2.cpu().numpy()[cf2.cpu().numpy().astype(np.int64)], v[fa])


@pytest.mark.parametrize("case", ["soup", "fans", "mc_noise", "mc_body", "ties"])
def test_clean_mesh_native_vs_plain_python_checker(case):
    """icon_clean_mesh (edge hash table, union-find over the faces, vertex counts through the same table, order-preserving
    compaction) against oracle/mc_check.py: largest_component_by_faces - trimesh's rules in plain Python: triangle soups (edges used by 1, 2,
    3+ faces, degenerate faces), fans around pinch vertices, marching-cubes surfaces of noise (hundreds of components) and of the
    body, equal-sized components (the one holding the lowest-index face wins)"""
    from oracle.mc_check import largest_component_by_faces as clean_mesh_check
    from icon_amd.recon import clean_mesh, export_mesh_device
    rs = np.random.RandomState(11)
    if case == "soup":
        v = rs.rand(60, 3).astype(np.float32)
        f = rs.randint(0, 60, (400, 3)).astype(np.int64)
        f[::37, 1] = f[::37, 0]                                      # some degenerate faces (a repeated vertex)
    elif case == "fans":                                            # 30 fans of 6 triangles around ONE shared vertex: 30 components of 7 vertices
        n = 30
        v = np.concatenate([np.zeros((1, 3)), rs.rand(n * 6, 3)]).astype(np.float32)
        f = np.array([[0, 1 + 6 * k + j, 1 + 6 * k + (j + 1) % 6] for k in range(n) for j in range(6)], np.int64)
        f = f[rs.permutation(len(f))]
    elif case == "ties":                                            # two tetrahedra of 4 vertices each, a third one listed first
        t = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]], np.int64)
        v = rs.rand(12, 3).astype(np.float32)
        f = np.concatenate([t + 8, t, t + 4])
    else:
        if case == "mc_noise":
            occ = torch.from_numpy(rs.rand(41, 41, 41).astype(np.float32)).to(dev())
        else:
            a = assets("body")
            occ = make_engine(a).eval_slab(T(a.features), 65, 0, 65)
        vt, ft = export_mesh_device(occ, 0.5)
        v, f = vt.cpu().numpy(), ft.cpu().numpy()
    ev, ef = clean_mesh_check(v, f)
    for rep in range(3):                                            # (the table inserts and unions race in a different order every time)
        cv, cf = clean_mesh(T(v), T(f))
        assert cv.dtype == torch.float32 and cf.dtype == torch.int32
        assert np.array_equal(cv.cpu().numpy(), ev) and np.array_equal(cf.cpu().numpy(), ef), (case, rep, cv.shape, ev.shape, cf.shape, ef.shape)
    from icon_amd.engine import IconAmdError
    fb = f.copy(); fb[len(fb) // 2, 2] = len(v)
    with pytest.raises(IconAmdError, match="face index out of range"):
        clean_mesh(T(v), T(fb))


def test_clean_mesh_vertex_scan_enters_a_second_round():
    """V = SCAN_ROUND + 300 vertices, nearly all unreferenced: the scan of the vertices' block counts (8,192 counts of 256 entries
    per round) carries a total into a second round.  A tetrahedron on vertices on both sides of entry SCAN_ROUND beats a lone
    triangle; the result is stated by construction.  No case with F above SCAN_ROUND: the faces' scan is the same code, and
    tests/test_gpu_garment.py: test_both_scans_enter_a_second_round drives it into its second round"""
    from icon_amd.garment import SCAN_ROUND as R
    from icon_amd.recon import clean_mesh
    v = np.random.RandomState(5).rand(R + 300, 3).astype(np.float32)
    tet = np.array([7, R - 1, R, R + 299])
    local = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]], np.int64)
    f = np.concatenate([tet[local], [[100, R + 5, 5000]]])
    cv, cf = clean_mesh(T(v), T(f))
    assert cv.dtype == torch.float32 and cf.dtype == torch.int32
    assert np.array_equal(cv.cpu().numpy(), v[tet]) and np.array_equal(cf.cpu().numpy(), local)


# ---------------------------------------------------------------------------------------------
# attach(): the HIP path behind a network object carrying exactly what the reference's HGPIFuNet carries
# ---------------------------------------------------------------------------------------------
def test_attach_on_a_frozen_replica_of_the_reference_network(body):
    """icon prior: a module with exactly the attributes tests/test_oracle_vs_reference.py verified on the real
    HGPIFuNet (ATTACH_*): attach -> netG.query == oracle; reconEngine(netG=netG) attaches by itself; a second
    filter() (new SMPL tensors) is picked up"""
    from types import SimpleNamespace
    from common import ATTACH_NET_ATTRS, ATTACH_REGRESSOR_ATTRS, ATTACH_SMPL_KEYS
    from icon_amd.engine import IconQueryEngine, query_func
    from icon_amd.recon import DenseReconEngine
    from oracle.query_torch import TorchMLP

    class FrozenHGPIFuNet(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.prior_type, self.sdf_clip, self.smpl_feats = "icon", body.sdf_clip, ["sdf", "norm", "vis", "cmap"]
            self.if_regressor = TorchMLP()
            self.if_regressor.norm, self.if_regressor.last_op = "batch", None
            self.smpl_feat_dict = None

        def query(self, *a, **k):
            raise AssertionError("the reference's torch query must have been replaced")

    netG = FrozenHGPIFuNet().eval()
    netG.if_regressor.load_state_dict({k: torch.from_numpy(v) for k, v in body.state_dict.items()}, strict=False)
    netG.to(dev())
    netG.smpl_feat_dict = {k: T(getattr(body, k)) for k in ATTACH_SMPL_KEYS}
    assert all(hasattr(netG, n) for n in ATTACH_NET_ATTRS) and all(hasattr(netG.if_regressor, n) for n in ATTACH_REGRESSOR_ATTRS)
    eng = IconQueryEngine.attach(netG)
    pts = synth.stratified_points(body.smpl_verts[0], body.smpl_faces[0], 4000, seed=12)
    feats = [T(body.features)]
    occ = query_func(SimpleNamespace(num_views=1), netG, feats, T(pts)[None])[0, 0].cpu().numpy()
    ref, _ = oracle_query(body, pts)
    assert np.abs(occ - ref).max() <= OCC_TOL
    # reconEngine(opt=, netG=, features=, proj_matrix=) finds the attached engine (apps/ICON.py:749-751)
    recon = DenseReconEngine(query_func=query_func, b_min=[[-1.0, 1.0, -1.0]], b_max=[[1.0, -1.0, 1.0]], resolutions=[17, 33],
                             align_corners=True).to(dev())
    vol = recon(opt=SimpleNamespace(num_views=1), netG=netG, features=feats, proj_matrix=None)
    ref33, _ = oracle_query(body, synth.lattice_points(33))
    assert np.abs(vol.cpu().numpy().ravel() - ref33).max() <= OCC_TOL
    # the next image: filter() binds new SMPL tensors (HGPIFuNet.py:236-240); the engine must notice
    ico = assets("ico")
    netG.smpl_feat_dict = {k: T(getattr(ico, k)) for k in ATTACH_SMPL_KEYS}
    occ2 = query_func(SimpleNamespace(num_views=1), netG, feats, T(pts)[None])[0, 0].cpu().numpy()
    ref2, _ = orc.query_icon(ico.smpl_verts[0], ico.smpl_faces[0], ico.smpl_cmap[0], ico.smpl_vis[0], body.features,
                             orc.Mlp(body.state_dict), pts, sdf_clip=body.sdf_clip)
    assert np.abs(occ2 - ref2).max() <= OCC_TOL
    assert eng is netG.icon_amd_engine


def test_bench_self_launch_two_ranks_on_one_gpu():
    """`python bench.py --gpus 2` as the driver calls it: the script starts its own ranks; under
    ICON_AMD_DIST_BACKEND=gloo two ranks share this one GPU (control flow only) and rank 0 prints the JSON line;
    with RCCL it stops at rank setup with a message that says how many devices are needed"""
    import json
    import os
    import subprocess
    import sys
    from common import ROOT
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--res", "65",
            "--no-cpu-baseline", "--no-extras"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(base, env=dict(env, ICON_AMD_DIST_BACKEND="gloo"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert out["n_gpus"] == 2 and len(out["config"]["rank_stage_ms"]) == 2 and out["config"]["parallelism"] == "zslab2"
    # default: the 'ab' layout - two Z-slabs per rank, in lattice order A_0, A_1, B_0, B_1; no assembly copies
    assert out["config"]["slab_layout"] == "ab" and out["config"]["assembly_copies"] == 0 and out["config"]["gather_to"] is None
    pc = out["config"]["pieces"]
    order = [pc[0][0], pc[1][0], pc[0][1], pc[1][1]]
    assert order[0][0] == 0 and order[-1][1] == 65 and all(a[1] == b[0] for a, b in zip(order[:-1], order[1:])), pc
    # the round-5 layout on request: one contiguous slab per rank
    p = subprocess.run(base + ["--slab-layout", "contiguous"], env=dict(env, ICON_AMD_DIST_BACKEND="gloo"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert out["config"]["slab_layout"] == "contiguous"
    planes = [r["planes"] for r in out["config"]["rank_stage_ms"]]
    assert planes[0][0] == 0 and planes[0][1] == planes[1][0] and planes[1][1] == 65
    # ... and only rank 0 receiving the volume
    p = subprocess.run(base + ["--gather-to", "0"], env=dict(env, ICON_AMD_DIST_BACKEND="gloo"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert out["config"]["gather_to"] == 0 and out["config"]["slab_layout"] == "ab"
    # BASELINE.json configs[4]: one image per GPU, whole volumes, no data-path collective
    p = subprocess.run(base + ["--replicas"], env=dict(env, ICON_AMD_DIST_BACKEND="gloo"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert rep["n_gpus"] == 2 and rep["scaling"] == "weak" and rep["config"]["parallelism"] == "replicas2"
    assert rep["config"]["points_per_step"] == 2 * 65 ** 3 and [r["planes"] for r in rep["config"]["rank_stage_ms"]] == [[0, 65], [0, 65]]
    assert abs(rep["value"] - 2 * 65 ** 3 / (rep["ms_per_step"] * 1e-3)) <= 1e-6 * rep["value"]
    if torch.cuda.device_count() < 2:
        p = subprocess.run(base, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert p.returncode != 0 and "need 2 HIP devices" in p.stderr


@pytest.mark.parametrize("world", [2, 3, 4])
def test_real_ranks_on_one_gpu_run_the_hip_slab_kernels(world):
    """SURVEY.md section 8e under REAL ranks: `world` processes (torch.distributed.run, gloo - they share this box's one GPU) each
    run the HIP kernels of their Z-slab through the sharded protocol of DenseReconEngine (packed 2-bit sign messages, one
    all_gather, the slab finished in two pieces, gathered volume), both cmap modes, 65^3 and 129^3, with and without the
    overlap / cost-balanced cut / reserved CUs, in the 'ab' layout (two slabs per rank, gathers straight into the result; also with
    gather_to = the last rank) and the contiguous one; rank 0 asserts the assembled volume == the single-process volume, bit for
    bit (tests/dist_gpu_worker.py).  The gloo tests of tests/test_dist_gloo.py prove the host protocol with a checker
    backend; this one puts the real kernels behind it."""
    import os
    import socket
    import subprocess
    import sys
    from common import ROOT
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "dist_gpu_worker.py")]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0 and f"DIST_GPU_OK world={world} checked=16" in p.stdout, p.stdout[-4000:]


@pytest.mark.parametrize("world", [2, 3])
def test_real_ranks_exchange_meshes_instead_of_the_volume(world):
    """DenseReconEngine.forward_mesh under REAL ranks (gloo, one GPU): every rank triangulates the cell layers of its own Z-slab
    (icon_mc_count_range / icon_mc_emit_keyed; only the neighbour's first plane of the volume travels), keyed vertices and faces
    are gathered and merged by key - the same vertices and faces IN THE SAME ORDER as marching cubes on the single-process
    volume, 33^3 .. 129^3, both cmap modes, equal and cost-balanced cuts; None where forward() returns None
    (tests/dist_gpu_mesh_worker.py)"""
    import os
    import socket
    import subprocess
    import sys
    from common import ROOT
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "dist_gpu_mesh_worker.py")]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0 and f"DIST_MESH_OK world={world} checked=12" in p.stdout, p.stdout[-4000:]


# ---------------------------------------------------------------------------------------------
# randomised sweep over lattice sizes, slabs, pieces, clip bands and bodies (tile mapping, shell, ranks)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_random_lattices_slabs_and_pieces_vs_oracle(seed):
    """whole lattice == oracle (<= 1e-4) and arbitrary slabs finished in arbitrary pieces == the whole-lattice volume of
    the same sign source, for random resolutions (tile counts below / above the grid size, interiors that are not a
    multiple of the tile), clip bands, bodies that do or do not reach the cube's boundary, both cmap modes"""
    import copy
    rng = np.random.RandomState(1000 + seed)
    a = copy.copy(assets("body" if seed % 3 else "ico"))
    v = a.smpl_verts.copy()
    v *= rng.uniform(0.6, 1.04)                                             # up to the cube's boundary (0.93 * 1.04 = 0.97)
    v += rng.uniform(-0.02, 0.02, 3).astype(np.float32)
    a.smpl_verts = v.astype(np.float32)
    a.sdf_clip = float(rng.choice([0.02, 0.05, 0.11]))
    res = int(rng.choice([5, 7, 9, 13, 19, 27, 33, 41, 49]))
    cmap_mode = "reference" if seed % 2 else "local"
    feat = T(a.features)
    eng = make_engine(a, cmap_mode=cmap_mode)
    full = eng.eval_slab(feat, res, 0, res, out=torch.full((res, res, res), float("nan"), device=dev()))
    ref, _ = orc.query_icon(a.smpl_verts[0], a.smpl_faces[0], a.smpl_cmap[0], a.smpl_vis[0], a.features, orc.Mlp(a.state_dict),
                            synth.lattice_points(res), sdf_clip=a.sdf_clip, cmap_local=(cmap_mode == "local"))
    assert np.abs(full.cpu().numpy().ravel() - ref).max() <= OCC_TOL
    if cmap_mode == "local":
        # any slab, cut into any pieces, reproduces its planes of the whole volume (no coupling between points)
        z0 = int(rng.randint(0, res - 1)); z1 = int(rng.randint(z0 + 1, res + 1))
        cuts = sorted(set([z0, z1] + [int(c) for c in rng.randint(z0, z1 + 1, 3)]))
        eng.slab_features(feat, res, z0, z1)
        out = torch.full((z1 - z0, res, res), float("nan"), device=dev())
        for za, zb in zip(cuts[:-1], cuts[1:]):
            eng.slab_finish_gathered(res, z0, z1, None, 0, 1, 0, out=out, za=za, zb=zb)
        assert torch.equal(out, full[z0:z1]), (res, z0, z1, cuts)
    else:
        # reference mode: "ranks" with their own slabs exchanging packed messages, pieces per rank
        world = int(rng.randint(2, 5))
        bounds = sorted(set([0, res] + [int(c) for c in rng.randint(0, res + 1, world - 1)]))
        parts = list(zip(bounds[:-1], bounds[1:]))
        per = max(b - x for x, b in parts)
        stride = 8 + ((per * res * res + 3) // 4 + 7) // 8 * 8
        engines = [make_engine(a, cmap_mode=cmap_mode) for _ in parts]
        msgs = []
        for (x, b), e in zip(parts, engines):
            m = torch.full((stride,), 0x55, dtype=torch.int8, device=dev()); m[:8] = 0
            e.slab_features(feat, res, x, b, msg=m)
            msgs.append(m)
        gathered = torch.cat(msgs).contiguous()
        outs = []
        for r, ((x, b), e) in enumerate(zip(parts, engines)):
            out = torch.full((b - x, res, res), float("nan"), device=dev())
            cuts = sorted(set([x, b] + [int(c) for c in rng.randint(x, b + 1, 2)]))
            for za, zb in zip(cuts[:-1], cuts[1:]):
                e.slab_finish_gathered(res, x, b, gathered, stride, len(parts), r, out=out, za=za, zb=zb)
            outs.append(out)
        assert torch.equal(torch.cat(outs), full), (res, parts)


def test_per_axis_resolutions(body):
    """resolutions given as (W, H, D) triples (lib/common/seg3d_lossless.py:66-71): one query over the materialised lattice,
    volume [D, H, W]; equals the oracle on the same points; export_mesh pads to a cube without moving a vertex"""
    from types import SimpleNamespace
    from icon_amd.recon import DenseReconEngine, lattice_coords
    from icon_amd.engine import query_func
    eng = make_engine(body)
    W, H, D = 33, 65, 17
    recon = DenseReconEngine(query_func=query_func, b_min=[[-1.0, 1.0, -1.0]], b_max=[[1.0, -1.0, 1.0]],
                             resolutions=[(9, 17, 5), (W, H, D)], align_corners=True, balance_value=0.5).to(dev())
    vol = recon(opt=SimpleNamespace(num_views=1), netG=eng, features=[T(body.features)], proj_matrix=None)
    assert vol.shape == (D, H, W)
    pts = lattice_coords((W, H, D), recon.b_min.cpu(), recon.b_max.cpu(), True, "cpu")[0].numpy()
    # the mapping is batch_eval's: x fastest, y flipped
    assert np.allclose(pts[0], [-1, 1, -1]) and np.allclose(pts[-1], [1, -1, 1]) and np.allclose(pts[1], [-1 + 2 / (W - 1), 1, -1])
    ref, _ = oracle_query(body, pts)
    assert np.abs(vol.cpu().numpy().ravel() - ref).max() <= OCC_TOL
    verts, faces = recon.export_mesh(vol)
    assert len(faces) > 50 and verts[:, 0].max() <= W - 1 and verts[:, 1].max() <= H - 1 and verts[:, 2].max() <= D - 1
    # a cubic lattice through the same generic path equals the fast path
    recon_c = DenseReconEngine(query_func=query_func, b_min=[[-1.0, 1.0, -1.0]], b_max=[[1.0, -1.0, 1.0]],
                               resolutions=[(33, 33, 33)], align_corners=True).to(dev())
    fast = recon_c(opt=SimpleNamespace(num_views=1), netG=eng, features=[T(body.features)], proj_matrix=None)
    assert torch.equal(fast, eng.eval_slab(T(body.features), 33, 0, 33))


def test_explicit_points_at_scale_equal_the_lattice_path(body):
    """(257, 257, 129): 8.5 M explicit points through query() (Morton packets, fused kernel in point mode) - every second
    plane of the 257^3 lattice, so in the per-point cmap mode the volume must be bit for bit the lattice path's
    (the same check passes at (513, 513, 257) = 67.6 M points, 71 ms)"""
    from types import SimpleNamespace
    from icon_amd.recon import DenseReconEngine
    from icon_amd.engine import query_func
    eng = make_engine(body, cmap_mode="local")
    full = eng.eval_slab(T(body.features), 257, 0, 257)
    recon = DenseReconEngine(query_func=query_func, b_min=[[-1.0, 1.0, -1.0]], b_max=[[1.0, -1.0, 1.0]], resolutions=[(257, 257, 129)],
                             align_corners=True, engine=eng).to(dev())
    vol = recon(opt=SimpleNamespace(num_views=1), netG=eng, features=[T(body.features)], proj_matrix=None)
    assert vol.shape == (129, 257, 257) and torch.equal(vol, full[::2])


# ---------------------------------------------------------------------------------------------
# last_op = Sigmoid (cfg.test_mode False, lib/net/HGPIFuNet.py:133; lib/net/MLP.py:68-70)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_sigmoid_last_op_vs_oracle(body, precision):
    """a regressor built with last_op = nn.Sigmoid(): sigmoid(MLP) then the in_cube mask, every precision, explicit points,
    lattice and the standalone MLP.forward; the module's own last_op is picked up by attach-style binding"""
    import warnings
    from icon_amd.engine import MlpHandle
    from oracle.query_torch import TorchMLP
    reg = TorchMLP().eval()
    reg.norm, reg.last_op = "batch", torch.nn.Sigmoid()
    reg.load_state_dict({k: torch.from_numpy(v) for k, v in body.state_dict.items()}, strict=False)
    eng = make_engine(body, precision=precision)
    eng.set_regressor(reg.to(dev()))
    omlp = orc.Mlp(body.state_dict, last_op="sigmoid")
    pts = synth.stratified_points(body.smpl_verts[0], body.smpl_faces[0], 3000, seed=21)
    pts = np.concatenate([pts, np.array([[1.0, 0.2, 0.1], [0.3, -1.0, 0.0], [1.2, 0.0, 0.0]], np.float32)])   # on / outside the cube
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        occ = eng.query([T(body.features)], T(pts.T.copy())[None], torch.eye(4, device=dev())[None])[0][0, 0].cpu().numpy()
        vol = eng.eval_slab(T(body.features), 33, 0, 33).cpu().numpy().ravel()
    ref, _ = orc.query_icon(body.smpl_verts[0], body.smpl_faces[0], body.smpl_cmap[0], body.smpl_vis[0], body.features, omlp, pts,
                            sdf_clip=body.sdf_clip)
    tol = OCC_TOL
    assert np.abs(occ - ref).max() <= tol
    assert (occ[-3:] == 0).all() and occ.min() >= 0.0 and occ.max() <= 1.0                # in_cube * sigmoid(.)
    inside = (np.abs(pts) < 1.0).all(1)
    assert ((occ[inside] > 0.0) & (occ[inside] < 1.0)).all() and (occ[~inside] == 0).all()
    ref33, _ = orc.query_icon(body.smpl_verts[0], body.smpl_faces[0], body.smpl_cmap[0], body.smpl_vis[0], body.features, omlp,
                              synth.lattice_points(33), sdf_clip=body.sdf_clip)
    assert np.abs(vol - ref33).max() <= tol
    x = np.random.RandomState(1).normal(0, 1, (777, 13)).astype(np.float32)
    from common import rows16
    h = MlpHandle({k: torch.from_numpy(v) for k, v in body.state_dict.items()}, last_op="sigmoid")
    got = h.forward(T(rows16(x)), precision).cpu().numpy()
    assert np.abs(got - omlp.forward(x)[:, 0]).max() <= OCC_TOL
    # the same weights without last_op differ (the flag is part of the handle key)
    reg.last_op = None
    plain = eng.eval_slab(T(body.features), 33, 0, 33).cpu().numpy().ravel()
    assert np.abs(plain - vol).max() > 0.1


# ---------------------------------------------------------------------------------------------
# norm_mlp: 'weight' (lib/net/MLP.py:42-45): weight_norm layers, no norm layers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_weight_norm_regressor_vs_oracle(body, precision):
    """a state_dict with filters.l.weight_g / weight_v and no norms.*: the library receives v * (g / ||v||) and runs the layers
    without normalisation (the oracle's reading of the same dict is pinned against the reference's MLP(norm='weight') in
    tests/test_oracle_vs_reference.py)"""
    from icon_amd.engine import MlpHandle
    from common import rows16
    from common import weight_norm_state_dict
    rs = np.random.RandomState(12)
    sd = weight_norm_state_dict(body.state_dict)
    omlp = orc.Mlp(sd)
    x = rs.normal(0, 1, (2000, 13)).astype(np.float32)
    h = MlpHandle({k: torch.from_numpy(v) for k, v in sd.items()})
    got = h.forward(T(rows16(x)), precision).cpu().numpy()
    want = omlp.forward(x, f64=True)[:, 0]
    assert np.abs(got - want).max() <= OCC_TOL * max(1.0, np.abs(want).max())
    eng = make_engine(body, precision=precision)
    eng.set_regressor({k: torch.from_numpy(v) for k, v in sd.items()})
    pts = synth.stratified_points(body.smpl_verts[0], body.smpl_faces[0], 3000, seed=22)
    occ = eng.query([T(body.features)], T(pts.T.copy())[None], torch.eye(4, device=dev())[None])[0][0, 0].cpu().numpy()
    ref, _ = orc.query_icon(body.smpl_verts[0], body.smpl_faces[0], body.smpl_cmap[0], body.smpl_vis[0], body.features, omlp, pts,
                            sdf_clip=body.sdf_clip)
    assert np.abs(occ - ref).max() <= OCC_TOL * max(1.0, np.abs(ref).max())
    vol = eng.eval_slab(T(body.features), 33, 0, 33).cpu().numpy().ravel()
    ref33, _ = orc.query_icon(body.smpl_verts[0], body.smpl_faces[0], body.smpl_cmap[0], body.smpl_vis[0], body.features, omlp,
                              synth.lattice_points(33), sdf_clip=body.sdf_clip)
    assert np.abs(vol - ref33).max() <= OCC_TOL * max(1.0, np.abs(ref33).max())


# ---------------------------------------------------------------------------------------------
# norm_mlp 'group' / 'instance' (lib/net/MLP.py:35-41): statistics over the points of the call (icon_amd/callnorm.py)
# ---------------------------------------------------------------------------------------------
def _callnorm_state_dict(body, kind):
    from common import callnorm_state_dict
    return callnorm_state_dict(body.state_dict, kind)


class _CallNormMLP(torch.nn.Module):
    """the attribute surface of lib/net/MLP.py for norm = 'group' / 'instance' (the reference class itself does not travel)"""

    def __init__(self, sd, kind):
        super().__init__()
        dims = [13, 512, 256, 128, 1]
        self.norm, self.last_op, self.res_layers = kind, None, [2, 3, 4]
        self.filters = torch.nn.ModuleList([torch.nn.Conv1d(dims[l] + (13 if l in (2, 3) else 0), dims[l + 1], 1) for l in range(4)])
        self.norms = torch.nn.ModuleList([torch.nn.GroupNorm(32, c) if kind == "group" else torch.nn.InstanceNorm1d(c) for c in dims[1:-1]])
        self.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("kind", ["group", "instance"])
def test_call_normalised_regressors_vs_oracle(body, kind, precision):
    """Group / InstanceNorm regressors: explicit points (whole call and a half of it - different statistics), the 33^3 lattice
    as one call (shell included in the statistics), module and state_dict binding; the oracle's restatement is pinned against
    the reference's MLP(norm=...) through its own query() in tests/test_oracle_vs_reference.py"""
    from icon_amd.engine import IconAmdError
    sd = _callnorm_state_dict(body, kind)
    omlp = orc.CallNormMlp(sd, kind)
    args = (body.smpl_verts[0], body.smpl_faces[0], body.smpl_cmap[0], body.smpl_vis[0], body.features, omlp)
    pts = synth.stratified_points(body.smpl_verts[0], body.smpl_faces[0], 4000, seed=23)
    pts = np.concatenate([pts, np.array([[1.0, 0.2, 0.1], [1.2, 0.0, 0.0]], np.float32)])      # on / outside the cube: in the statistics, masked after
    eye = torch.eye(4, device=dev())[None]
    for cmap_mode in ("reference", "local"):
        eng = make_engine(body, precision=precision, cmap_mode=cmap_mode)
        eng.set_regressor(_CallNormMLP(sd, kind).eval().to(dev()))
        occ = eng.query([T(body.features)], T(pts.T.copy())[None], eye)[0][0, 0].cpu().numpy()
        ref, _ = orc.query_icon_callnorm(*args, pts, sdf_clip=body.sdf_clip, cmap_local=(cmap_mode == "local"))
        scale = max(1.0, float(np.abs(ref).max()))
        assert np.abs(occ - ref).max() <= OCC_TOL * scale, (kind, cmap_mode)
        assert (occ[-2:] == 0).all()
        half = eng.query([T(body.features)], T(pts[:2000].T.copy())[None], eye)[0][0, 0].cpu().numpy()
        ref_half, _ = orc.query_icon_callnorm(*args, pts[:2000], sdf_clip=body.sdf_clip, cmap_local=(cmap_mode == "local"))
        assert np.abs(half - ref_half).max() <= OCC_TOL * scale
        assert np.abs(half - occ[:2000]).max() > 1e-3                    # the population of the call matters
        vol = eng.eval_slab(T(body.features), 33, 0, 33).cpu().numpy().ravel()
        ref33, _ = orc.query_icon_callnorm(*args, synth.lattice_points(33), sdf_clip=body.sdf_clip, cmap_local=(cmap_mode == "local"))
        assert np.abs(vol - ref33).max() <= OCC_TOL * max(1.0, float(np.abs(ref33).max())), (kind, cmap_mode)
    # a state_dict does not say what its norms are
    eng = make_engine(body, precision=precision)
    eng.set_regressor({k: torch.from_numpy(v) for k, v in sd.items()})
    if kind == "group":
        with pytest.raises(IconAmdError, match="norm_mlp"):
            eng.query([T(body.features)], T(pts.T.copy())[None], eye)
    eng.norm_mlp = kind
    occ = eng.query([T(body.features)], T(pts.T.copy())[None], eye)[0][0, 0].cpu().numpy()
    ref, _ = orc.query_icon_callnorm(*args, pts, sdf_clip=body.sdf_clip)
    assert np.abs(occ - ref).max() <= OCC_TOL * max(1.0, float(np.abs(ref).max()))
    # the split slab protocol (the multi-GPU driver's) has no whole-call statistics: refused by name
    with pytest.raises(IconAmdError, match="split slab protocol"):
        eng.slab_finish_gathered(33, 0, 33, None, 0, 1, 0, device=dev())


def test_rows_entry_points_vs_oracle(body):
    """icon_query_rows / icon_grid_rows: the MLP input rows [N,16] of a call = the oracle's X (reference channel order),
    slot 15 the in_cube bit; the lattice version includes the shell (no skip)"""
    eng = make_engine(body)
    omlp = orc.Mlp(body.state_dict)
    pts = synth.stratified_points(body.smpl_verts[0], body.smpl_faces[0], 3000, seed=24)
    pts = np.concatenate([pts, np.array([[1.0, 0.2, 0.1]], np.float32)])
    rows = eng._rows(T(body.features), points=T(pts), calib12=np.eye(4, dtype=np.float32)[:3].copy()).cpu().numpy()
    _, X = orc.query_icon(body.smpl_verts[0], body.smpl_faces[0], body.smpl_cmap[0], body.smpl_vis[0], body.features, omlp, pts, sdf_clip=body.sdf_clip)
    assert np.abs(rows[:, :13] - X).max() <= 2e-6 and (rows[:, 13:15] == 0).all()
    code = rows[:, 15].view(np.int32)
    assert ((code & 8) != 0).tolist() == ((np.abs(pts) < 1.0).all(1)).tolist()
    rows33 = eng._rows(T(body.features), lattice=(33, 0, 33)).cpu().numpy()
    _, X33 = orc.query_icon(body.smpl_verts[0], body.smpl_faces[0], body.smpl_cmap[0], body.smpl_vis[0], body.features, omlp,
                            synth.lattice_points(33), sdf_clip=body.sdf_clip)
    assert np.abs(rows33[:, :13] - X33).max() <= 2e-6
    shell = ~(np.abs(synth.lattice_points(33)) < 1.0).all(1)
    assert np.abs(rows33[shell, :13]).max() > 0.5 and ((rows33[:, 15].view(np.int32) & 8) != 0).tolist() == (~shell).tolist()


@pytest.mark.parametrize("mesh", ["body", "ico"])
@pytest.mark.parametrize("res", [17, 33, 65])
def test_shared_walk_lattice_rows_equal_point_rows(mesh, res):
    """the lattices of few packets (<= 65^3) search with ONE packet per workgroup, the walk shared by 8 / 16 wavefronts through an
    LDS queue (geom_device.h: nearest_shared); explicit points go through the one-wave-per-point / one-wave-per-packet
    searches.  Same points -> the same nearest faces -> the same feature rows, BIT FOR BIT (sdf, cmap, normals, vis, code).
    Repeated: the sharing is timing dependent, the answer must not be."""
    a = assets(mesh)
    eng = make_engine(a)
    feat = T(a.features)
    pts = synth.lattice_points(res)
    want = eng._rows(feat, points=T(pts), calib12=np.eye(4, dtype=np.float32)[:3].copy()).cpu().numpy()
    for rep in range(4):
        got = eng._rows(feat, lattice=(res, 0, res)).cpu().numpy()
        bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
        assert len(bad) == 0, f"{mesh} {res}^3 pass {rep}: {len(bad)} rows differ, first {bad[:5]}"


# ---------------------------------------------------------------------------------------------
# the reference's own answers for the configurations outside configs/*.yaml (tests/golden/variants.npz)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("name", ["mvp_sdf", "novis_full", "vis_sdf", "weight", "group", "instance", "sigmoid"])
def test_variants_golden_reference(body, name, precision):
    """HIP path vs the fixture tools/make_golden.py (section i) wrote by running the reference's HGPIFuNet.query with its own MLP
    class: smpl_feats with / without 'vis' (icon-mvp), norm_mlp 'weight' / 'group' / 'instance', last_op Sigmoid"""
    from common import VARIANTS, variant_state_dict, golden
    from icon_amd.engine import IconQueryEngine
    g = golden("variants.npz")
    planes, feats, norm, last_op = VARIANTS[name]
    c0, sd = variant_state_dict(name, body)
    eng = IconQueryEngine(prior_type="icon", sdf_clip=body.sdf_clip, smpl_feats=feats, precision=precision)
    eng.set_mesh(T(body.smpl_verts), T(body.smpl_faces), T(body.smpl_cmap), T(body.smpl_vis))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in sd.items()})
    eng.last_op = last_op
    eng.norm_mlp = norm if norm in ("group", "instance") else None
    pts = g["points"]
    occ = eng.query([T(np.ascontiguousarray(body.features[:, :planes]))], T(pts.T.copy())[None], torch.eye(4, device=dev())[None])[0][0, 0].cpu().numpy()
    want = g["occ_" + name]
    assert np.abs(occ - want).max() <= OCC_TOL * max(1.0, float(np.abs(want).max())), name
    assert (occ[-2:] == 0).all()


# ---------------------------------------------------------------------------------------------
# cfg.net.smpl_feats subsets (lib/net/HGPIFuNet.py:301-311)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("feats,planes", [(["sdf", "vis"], 12), (["sdf", "norm", "vis"], 12), (["sdf", "cmap", "vis"], 12),
                                          (["sdf"], 6), (["sdf"], 12), (["sdf", "norm", "cmap"], 6), (["sdf", "cmap"], 6)])
def test_smpl_feats_subsets_vs_oracle(body, feats, planes, precision):
    """the MLP input [img | sdf | cmap? | norm?] for subsets of cfg.net.smpl_feats (the oracle's layout is pinned against the
    reference's query() in tests/test_oracle_vs_reference.py); without 'vis' (configs/train/icon-mvp.yaml:40) img is EVERY
    feature channel (HGPIFuNet.py:345-346), with it the half smpl_vis selects"""
    from icon_amd.engine import IconQueryEngine, IconAmdError
    img = planes // 2 if "vis" in feats else planes
    c0 = img + 1 + (3 if "cmap" in feats else 0) + (3 if "norm" in feats else 0)
    sd = synth.make_mlp_state_dict(synth.SEED + 5, dims=(c0, 512, 256, 128, 1))
    omlp = orc.Mlp(sd)
    pts = synth.stratified_points(body.smpl_verts[0], body.smpl_faces[0], 3000, seed=31)
    features = np.ascontiguousarray(body.features[:, :planes])
    feat = T(features)
    try:
        orc.set_smpl_feats("cmap" in feats, "norm" in feats, "vis" in feats)
        for cmap_mode in ("reference", "local"):
            eng = IconQueryEngine(prior_type="icon", sdf_clip=body.sdf_clip, smpl_feats=feats, cmap_mode=cmap_mode, precision=precision)
            eng.set_mesh(T(body.smpl_verts), T(body.smpl_faces), T(body.smpl_cmap), T(body.smpl_vis))
            eng.set_regressor({k: torch.from_numpy(v) for k, v in sd.items()})
            occ = eng.query([feat], T(pts.T.copy())[None], torch.eye(4, device=dev())[None])[0][0, 0].cpu().numpy()
            ref, _ = orc.query_icon(body.smpl_verts[0], body.smpl_faces[0], body.smpl_cmap[0], body.smpl_vis[0], features, omlp, pts,
                                    sdf_clip=body.sdf_clip, cmap_local=(cmap_mode == "local"))
            assert np.abs(occ - ref).max() <= OCC_TOL, (feats, cmap_mode)
            vol = eng.eval_slab(feat, 33, 0, 33).cpu().numpy().ravel()
            ref33, _ = orc.query_icon(body.smpl_verts[0], body.smpl_faces[0], body.smpl_cmap[0], body.smpl_vis[0], features, omlp,
                                      synth.lattice_points(33), sdf_clip=body.sdf_clip, cmap_local=(cmap_mode == "local"))
            assert np.abs(vol - ref33).max() <= OCC_TOL, (feats, cmap_mode)
    finally:
        orc.set_smpl_feats(True, True, True)
    # a regressor whose input width does not match the selected features is refused by the library
    eng = IconQueryEngine(prior_type="icon", sdf_clip=body.sdf_clip, smpl_feats=feats)
    eng.set_mesh(T(body.smpl_verts), T(body.smpl_faces), T(body.smpl_cmap), T(body.smpl_vis))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in synth.make_mlp_state_dict(synth.SEED + 6, dims=(c0 + 1, 512, 256, 128, 1)).items()})
    with pytest.raises(IconAmdError, match="input width"):
        eng.query([feat], T(pts.T.copy())[None], torch.eye(4, device=dev())[None])


def test_smpl_feats_wider_than_the_kernels_is_refused(body):
    """twelve feature planes without 'vis' plus cmap: 12 + 1 + 3 = 16 input channels, one more than the kernels carry"""
    from icon_amd.engine import IconQueryEngine, IconAmdError
    eng = IconQueryEngine(prior_type="icon", sdf_clip=body.sdf_clip, smpl_feats=["sdf", "cmap"])
    eng.set_mesh(T(body.smpl_verts), T(body.smpl_faces), T(body.smpl_cmap), T(body.smpl_vis))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in body.state_dict.items()})
    with pytest.raises(IconAmdError, match="15 MLP input channels"):
        eng.query([T(body.features)], torch.zeros(1, 3, 8, device=dev()), torch.eye(4, device=dev())[None])
    with pytest.raises(IconAmdError, match="15 MLP input channels"):
        eng.eval_slab(T(body.features), 17, 0, 17)


# ---------------------------------------------------------------------------------------------
# meshes with more than 32,768 triangle slots (the 16-bit slot hand-over carries a byte of higher bits for them)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_mesh_with_more_slots_than_15_bits(body, precision):
    """81,920 faces: every consumer of the nearest-triangle hand-over (k_sign, the fused feature phase, k_features) must
    see the full slot index; lattice and explicit points against the oracle"""
    import copy
    from icon_amd.engine import MeshHandle
    v, f = synth.icosphere(6, radius=0.62, center=(0.03, -0.05, 0.02))
    v = (v * np.array([0.7, 1.25, 0.45])).astype(np.float32)              # an ellipsoid: not every face equidistant from anything
    f = f.astype(np.int64)
    vis, cm = synth.make_vis_cmap(v, f)
    a = copy.copy(body)
    a.smpl_verts, a.smpl_faces = v[None], f[None]
    a.smpl_cmap = np.asarray(cm, np.float32).reshape(1, -1, 3)
    a.smpl_vis = np.asarray(vis, np.float32).reshape(1, -1, 1)
    h = MeshHandle(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
    assert h.stats()["slots"] > 32768
    eng = make_engine(a, precision=precision)
    res = 33
    occ = eng.eval_slab(T(a.features), res, 0, res).cpu().numpy().ravel()
    ref, _ = oracle_query(a, synth.lattice_points(res))
    assert np.abs(occ - ref).max() <= OCC_TOL
    pts = synth.stratified_points(v, f, 5000, seed=8)
    q = eng.query([T(a.features)], T(pts.T.copy())[None], torch.eye(4, device=dev())[None])[0][0, 0].cpu().numpy()
    refq, _ = oracle_query(a, pts)
    assert np.abs(q - refq).max() <= OCC_TOL
    faces_hit = h.sdf_query(T(pts))["face"].cpu().numpy()
    assert faces_hit.max() > 40000          # the sample does reach triangles stored beyond slot 32,768
    if precision == "f16x3":                # the native schedule (shared-walk block search, 4-lane sign kernel) carries the high byte too
        from types import SimpleNamespace
        from icon_amd.engine import query_func
        from icon_amd.recon import AdaptiveReconEngine
        kw = dict(query_func=query_func, b_min=[[-1.0, 1.0, -1.0]], b_max=[[1.0, -1.0, 1.0]], resolutions=[17, 33, 65], align_corners=True, faster=True)
        call = dict(opt=SimpleNamespace(num_views=1), netG=eng, features=[T(a.features)], proj_matrix=None)
        nat, host = AdaptiveReconEngine(**kw).to(dev()), AdaptiveReconEngine(**kw).to(dev())
        host.native = False
        v1, v2 = nat(**call), host(**call)
        assert nat.last_stats.get("native") is True and nat.last_stats["queries"] == host.last_stats["queries"]
        assert (v1 - v2).abs().max().item() <= 1e-6


# ---------------------------------------------------------------------------------------------
# the sharded path on the REAL collective backend (RCCL), world size 1
# ---------------------------------------------------------------------------------------------
_NCCL_WORLD1 = r'''
import os, sys
sys.path.insert(0, os.environ["ICON_ROOT"]); sys.path.insert(0, os.path.join(os.environ["ICON_ROOT"], "tests"))
import numpy as np, torch, torch.distributed as dist
from types import SimpleNamespace
from icon_amd import synth
from icon_amd.engine import IconQueryEngine, query_func
from icon_amd.recon import DenseReconEngine
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
a = synth.make_assets("body")
T = lambda x: torch.from_numpy(x).to(dev)
out = {}
for cmap_mode in ("reference", "local"):
    for overlap, layout, gather_to in ((True, "ab", None), (True, "ab", 0), (True, "contiguous", None), (False, "ab", None)):
        eng = IconQueryEngine(prior_type="icon", sdf_clip=a.sdf_clip, cmap_mode=cmap_mode)
        eng.set_mesh(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
        eng.set_regressor({k: torch.from_numpy(v) for k, v in a.state_dict.items()})
        rec = DenseReconEngine(query_func=query_func, resolutions=[17, 65], align_corners=True, engine=eng, overlap_gather=overlap,
                               slab_layout=layout, gather_to=gather_to).to(dev)
        want = eng.eval_slab(T(a.features), 65, 0, 65)
        got = rec._forward_sharded(eng, T(a.features), 65, dist, 1, 0)          # the N > 1 code path, one rank: RCCL broadcast / all_gather / gather / async handles
        assert torch.equal(got, want), (cmap_mode, overlap, layout, gather_to)
        assert rec.last_stats["slabs"] == [(0, 65)]
        ab = overlap and layout == "ab"
        assert rec.last_stats.get("layout", "contiguous") == ("ab" if ab else "contiguous")
        if ab:      # two slabs of the one rank, two sign gathers into one buffer, two volume gathers (all_gather or gather) into one result
            assert rec.last_stats["pieces"] == [((0, 33), (33, 65))] and rec.last_stats["assembly_copies"] == 0 and got.storage_offset() == 0
dist.barrier(); dist.destroy_process_group()
print("NCCL-WORLD1-OK")
'''


def test_sharded_path_on_rccl_world_size_one():
    """every collective call of the Z-slab path (cut broadcast, int8 message all_gather, the two asynchronous volume gathers
    and their handles; round 6: the 'ab' layout's gathers into views of one result buffer, `dist.gather` for gather_to) issued on the real backend - "nccl" = RCCL - with one rank: API and dtype compatibility that the gloo
    tests cannot vouch for; the volume must equal the unsharded one bit for bit"""
    import os
    import socket
    import subprocess
    import sys
    from common import ROOT
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    env = dict(os.environ, ICON_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-c", _NCCL_WORLD1], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "NCCL-WORLD1-OK" in p.stdout, p.stdout[-3000:]


# ---------------------------------------------------------------------------------------------
# regressors outside what the fused kernels carry: icon_amd/composed.py (HIP geometry leaf + PyTorch-ROCm operators)
# ---------------------------------------------------------------------------------------------
class _AnyMLP(torch.nn.Module):
    """lib/net/MLP.py's attribute surface and forward for arbitrary filter_channels / res_layers / last_op, eval-mode BatchNorm"""

    def __init__(self, dims, res_layers, last_op=None, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.norm, self.last_op, self.res_layers = "batch", last_op, list(res_layers)
        self.filters = torch.nn.ModuleList([torch.nn.Conv1d(dims[l] + (dims[0] if l in res_layers else 0), dims[l + 1], 1) for l in range(len(dims) - 1)])
        self.norms = torch.nn.ModuleList([torch.nn.BatchNorm1d(c) for c in dims[1:-1]])
        with torch.no_grad():
            for m in self.norms:
                m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5); m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.1)

    def forward(self, x):
        y = x
        for i, f in enumerate(self.filters):
            y = f(torch.cat([y, x], 1) if i in self.res_layers else y)
            if i != len(self.filters) - 1:
                y = torch.nn.functional.leaky_relu(self.norms[i](y), 0.01)
        return self.last_op(y) if self.last_op is not None else y


@pytest.mark.parametrize("case", ["pifu_size_mlp", "nineteen_inputs", "tanh"])
def test_composed_path_on_the_gpu(body, case):
    """what the fused kernels do not carry goes through icon_amd/composed.py with a warning that says why: the same code on the
    CPU with the checker's geometry leaf (that pairing is pinned against the reference's query() in
    tests/test_oracle_vs_reference.py) gives the same occupancies; explicit points and a lattice"""
    import warnings
    from types import SimpleNamespace
    from icon_amd import composed
    from icon_amd.engine import IconQueryEngine
    feats, dims, last_op = ["sdf", "norm", "vis", "cmap"], [13, 512, 256, 128, 1], None
    if case == "pifu_size_mlp":
        dims = [13, 1024, 512, 256, 128, 1]
    elif case == "nineteen_inputs":
        feats, dims = ["sdf", "norm", "cmap"], [19, 512, 256, 128, 1]
    else:
        last_op = torch.nn.Tanh()
    mlp = _AnyMLP(dims, [2, 3, 4], last_op, seed=3).eval()
    pts = synth.stratified_points(body.smpl_verts[0], body.smpl_faces[0], 3000, seed=52)
    pts = np.concatenate([pts, np.array([[1.0, 0.2, 0.1], [1.2, 0.0, 0.0]], np.float32)])

    def checker_leaf(p):
        o = orc.cal_sdf(body.smpl_verts[0], body.smpl_faces[0], body.smpl_cmap[0], body.smpl_vis[0], p.numpy())
        return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in o.items() if k in ("sdf", "norm", "cmap", "vis")}
    cpu = SimpleNamespace(prior_type="icon", smpl_feats=tuple(feats), sdf_clip=body.sdf_clip, cmap_mode="reference", res_layers=(2, 3, 4),
                          norm_mlp=None, last_op=None)
    Tc = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    want = composed.query_composed(cpu, [Tc(body.features)], Tc(pts.T.copy())[None], torch.eye(4)[None], mlp, sdf_query=checker_leaf)[0][0, 0].numpy()
    want33 = composed.query_composed(cpu, [Tc(body.features)], Tc(synth.lattice_points(33).T.copy())[None], torch.eye(4)[None], mlp,
                                     sdf_query=checker_leaf)[0][0, 0].numpy()
    eng = IconQueryEngine(prior_type="icon", sdf_clip=body.sdf_clip, smpl_feats=feats)
    eng.set_mesh(T(body.smpl_verts), T(body.smpl_faces), T(body.smpl_cmap), T(body.smpl_vis))
    eng.set_regressor(mlp.to(dev()))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        import icon_amd.engine as E
        E._WARNED_COMPOSED.clear()
        occ = eng.query([T(body.features)], T(pts.T.copy())[None], torch.eye(4, device=dev())[None])[0][0, 0].cpu().numpy()
        vol = eng.eval_slab(T(body.features), 33, 0, 33).cpu().numpy().ravel()
    assert sum("composed path" in str(w.message) for w in rec) == 1           # announced once, with the reason
    scale = max(1.0, float(np.abs(want).max()))
    assert np.abs(occ - want).max() <= 2e-5 * scale and (occ[-2:] == 0).all()
    assert np.abs(vol - want33).max() <= 2e-5 * max(1.0, float(np.abs(want33).max()))
    if case == "tanh":
        # more points than one chunk (129^3 = 2.15 M > 2^21; MIOpen's batch norm refuses such inputs - ATen's kernels run): in the
        # per-point cmap mode a sample of the volume equals the same points asked for on their own
        eng.cmap_mode, cpu.cmap_mode = "local", "local"
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            big = eng.eval_slab(T(body.features), 129, 0, 129).cpu().numpy().ravel()
        idx = np.random.RandomState(0).choice(129 ** 3, 3000, replace=False)
        p = synth.lattice_points(129)[idx]
        sub = composed.query_composed(cpu, [Tc(body.features)], Tc(p.T.copy())[None], torch.eye(4)[None], mlp.cpu(), sdf_query=checker_leaf)[0][0, 0].numpy()
        assert np.isfinite(big).all() and np.abs(big[idx] - sub).max() <= 2e-5

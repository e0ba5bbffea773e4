"""GPU: the batched query() (icon_query_points_batch) against the batched float64 oracle (tests/batch_oracle.py, pinned on
the CPU by tests/test_batch_oracle.py) on the branches tests/test_gpu_batch_query.py does not reach: the packet search with
padding lanes (n no multiple of 64), B > 4 (Morton keys that give low bits to the subject index), the reference cmap mode over
the packet search, meshes with more than 32,768 triangle slots in a batch, one engine across calls of changing B and n, clip
bands that empty or fill the batch-global outlier list, and the [B,3,4] calibration layout.

Every comparison with the oracle holds to OCC_TOL = 1e-4, the bar of the B = 1 comparisons in tests/test_gpu_parity.py for
both precisions.  Largest observed max |device - oracle| on an MI355X over all cases of this module: 1.55e-6 with f16x3 (the
unlike subjects; 6.0e-7 over the other cases) and 6.0e-7 with f32.

The guards on the outlier list are computed from the ORACLE's values: in every general 'reference' case every subject
contributes both outliers and non-outliers and 0.1 <= K / (B n) <= 0.9.  Three kinds of case state their own list instead,
because the general guard contradicts what they are built for: n = 1 (one point is an outlier or it is not: the BATCH must
hold both kinds), the empty / full lists (K = 0, K = B n), and the unlike subjects (one subject nearly all outliers, one with
none)."""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_oracle as bo  # noqa: E402
import batch_subjects as bs  # noqa: E402
from icon_amd import synth  # noqa: E402
from icon_amd.engine import IconQueryEngine, MeshHandle  # noqa: E402
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
OCC_TOL = 1e-4
SDF_CLIP = 0.05
DEV = torch.device("cuda:0")
MESH_KEYS = ("smpl_verts", "smpl_faces", "smpl_cmap", "smpl_vis")
PACKET_MIN = 98304                       # kPacketMinPoints (icon_amd/csrc/geom_device.h): B * n at which the search turns to packets


def T(x):
    return torch.from_numpy(np.array(x)).to(DEV)         # a copy: the cached inputs are read-only


@lru_cache(maxsize=None)
def planes(B):
    return bs.planes(B, 12, 128, 0)


@lru_cache(maxsize=None)
def oracle_mlp():
    return orc.Mlp(bs.state_dict("full"))


def engine(S, feat, cmap_mode="reference", precision="f16x3", sdf_clip=SDF_CLIP):
    """variant 'full', stack 0, over the subjects S with the feature planes feat [B,12,128,128]"""
    eng = IconQueryEngine(prior_type="icon", sdf_clip=sdf_clip, smpl_feats=("sdf", "norm", "vis", "cmap"), cmap_mode=cmap_mode, precision=precision)
    eng.set_mesh(*(T(S[k]) for k in MESH_KEYS))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in bs.state_dict("full").items()})
    return eng, [T(feat)]


def device_query(eng, feats, pts, calibs):
    """pts [B,n,3] numpy world points -> [B,n] float32"""
    out = eng.query(feats, T(pts.transpose(0, 2, 1)), T(calibs))
    assert len(out) == 1 and tuple(out[0].shape) == (pts.shape[0], 1, pts.shape[1])
    return out[0][:, 0]


def single_calls(S, feats, pts, precision="f16x3"):
    """B = 1 calls (cmap_mode 'local') on every subject -> list of [n] device tensors"""
    out = []
    for b in range(pts.shape[0]):
        one, _ = engine({k: S[k][b:b + 1] for k in MESH_KEYS}, np.zeros(0, np.float32), "local", precision)
        out.append(device_query(one, [feats[0][b:b + 1]], pts[b:b + 1], S["calibs"][b:b + 1])[0])
    return out


def edge_subset(B, n, seed=0):
    """the first and last 128 call positions of every subject - where tiles that take one point per lane straddle two subjects -
    plus 3,000 random positions"""
    edge = np.concatenate([b * n + np.r_[0:128, n - 128:n] for b in range(B)])
    return np.unique(np.concatenate([edge, np.random.RandomState(seed + 77).choice(B * n, 3000, replace=False)]))


def points(S, n, seed=0):
    """[B,n,3] world points.  A draw of ONE point per subject is the far-field point for every subject and seed (K = B): the
    n = 1 cases take the first point of the 63-point draw instead, which mixes outliers and others for B = 2, 5 and 8"""
    return bs.candidate_points(S, 63, seed)[:, :1].copy() if n == 1 else bs.candidate_points(S, n, seed)


def guards(K, counts, B, n):
    assert K == counts.sum()
    if n > 1:
        assert (counts > 0).all() and (counts < n).all(), f"outliers per subject {counts.tolist()} of {n}"
    assert 0.1 <= K / (B * n) <= 0.9, f"K = {K} of {B * n}"


@lru_cache(maxsize=None)
def std_case(B, n, cmap_local, subset=False):
    """subjects, points and the oracle's answer (read-only) of a case over bs.subjects(B)"""
    S = bs.subjects(B)
    pts = points(S, n)
    sub = edge_subset(B, n) if subset else None
    occ, K, counts = bo.batch_query_icon(S, planes(B), oracle_mlp(), pts, SDF_CLIP, cmap_local, subset=sub)
    for a in (pts, occ, counts):
        a.setflags(write=False)
    return S, pts, sub, occ, K, counts


def compare(got, occ, sub, what):
    """got: [B,n] device tensor; occ: the oracle's [B,n], or [len(sub)] at the call positions sub"""
    got = got.cpu().numpy()
    err = float(np.abs(got - occ).max()) if sub is None else float(np.abs(got.reshape(-1)[sub] - occ).max())
    print(f"{what}: max |device - oracle| = {err:.3e}")
    assert np.isfinite(got).all() and err <= OCC_TOL, f"{what}: max |device - oracle| = {err}"


# ---------------------------------------------------------------------------------------------
# cooperative search, every point
# ---------------------------------------------------------------------------------------------
COOP = [(B, n) for B in (2, 5, 8) for n in (1, 63, 1001)]


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("cmap_mode", ["reference", "local"])
@pytest.mark.parametrize("B,n", COOP)
def test_cooperative_path_vs_oracle(B, n, cmap_mode, precision):
    S, pts, _, occ, K, counts = std_case(B, n, cmap_mode == "local")
    if cmap_mode == "reference":
        guards(K, counts, B, n)
    eng, feats = engine(S, planes(B), cmap_mode, precision)
    compare(device_query(eng, feats, pts, S["calibs"]), occ, None, f"coop B={B} n={n} {cmap_mode} {precision} K={K}")


def test_outlier_lists_wrap_out_of_phase():
    """over the reference cases above the tiling olist[(3j + k) % K] wraps in both phases K % 3 = 1 and K % 3 = 2"""
    phases = {std_case(B, n, False)[4] % 3 for B, n in COOP}
    assert {1, 2} <= phases, phases


# ---------------------------------------------------------------------------------------------
# packet search: padding lanes (n % 64 != 0) and every key layout (subject bits 1, 2, 3, 3 over 30, 30, 29, 29 Morton bits)
# ---------------------------------------------------------------------------------------------
PACKETS = [(2, 49153), (3, 32769), (5, 19663), (8, 12289)]


@pytest.mark.parametrize("B,n", PACKETS)
def test_packet_search_equals_cooperative_search_point_for_point(B, n):
    """cmap_mode 'local': subject b of the batch (packets: B n >= 98,304, the segment of every subject padded to whole wavefronts)
    is bit for bit the B = 1 call on subject b (n < 98,304: the cooperative search), for ALL points"""
    assert B * n >= PACKET_MIN > n and n % 64 != 0
    S = bs.subjects(B)
    pts = points(S, n)
    eng, feats = engine(S, planes(B), "local")
    batched = device_query(eng, feats, pts, S["calibs"])
    for b, single in enumerate(single_calls(S, feats, pts)):
        diff = (batched[b] != single).nonzero().flatten()
        assert diff.numel() == 0, (f"subject {b}: {diff.numel()} of {n} points differ, first call positions {diff[:8].tolist()}, "
                                   f"max diff {(batched[b] - single).abs().max().item()}")


@pytest.mark.parametrize("B,n,precision", [(B, n, "f16x3") for B, n in PACKETS] + [(5, 19663, "f32")])
def test_packet_search_reference_mode_vs_oracle(B, n, precision):
    assert B * n >= PACKET_MIN and n % 64 != 0
    S, pts, sub, occ, K, counts = std_case(B, n, False, subset=True)
    guards(K, counts, B, n)
    eng, feats = engine(S, planes(B), "reference", precision)
    compare(device_query(eng, feats, pts, S["calibs"]), occ, sub, f"packets B={B} n={n} reference {precision} K={K} K%3={K % 3}")


@pytest.mark.parametrize("n", [32767, 32768])
def test_the_switch_between_the_searches(n):
    """B = 3: 98,301 points take the cooperative search, 98,304 the packets"""
    B = 3
    assert (B * n >= PACKET_MIN) == (n == 32768)
    S, pts, sub, occ, K, counts = std_case(B, n, False, subset=True)
    guards(K, counts, B, n)
    eng, feats = engine(S, planes(B), "reference")
    compare(device_query(eng, feats, pts, S["calibs"]), occ, sub, f"switch B={B} n={n} K={K}")


# ---------------------------------------------------------------------------------------------
# empty and full outlier lists
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [0.0, 10.0])
def test_empty_and_full_outlier_lists(clip):
    B, n = 5, 1001
    S = bs.subjects(B)
    pts = bs.candidate_points(S, n, 3)
    occ, K, counts = bo.batch_query_icon(S, planes(B), oracle_mlp(), pts, clip, False)
    assert K == (B * n if clip == 0.0 else 0)
    eng, feats = engine(S, planes(B), "reference", sdf_clip=clip)
    compare(device_query(eng, feats, pts, S["calibs"]), occ, None, f"clip {clip} K={K}")


# ---------------------------------------------------------------------------------------------
# more than 32,768 triangle slots in a batch
# ---------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def big_subjects():
    """the 81,920-face ellipsoid of test_mesh_with_more_slots_than_15_bits and a rotated, rescaled copy with the same faces"""
    v, f = synth.icosphere(6, radius=0.62, center=(0.03, -0.05, 0.02))
    v0 = (v * np.array([0.7, 1.25, 0.45])).astype(np.float32)
    f = f.astype(np.int64)
    c = v0.astype(np.float64).mean(0)
    v1 = (((v0.astype(np.float64) - c) @ (bs._rot(2, 0.5) @ bs._rot(0, -0.3)).T) * 0.8 + c + np.array([0.05, 0.02, -0.04])).astype(np.float32)
    verts, vis, cmap = [], [], []
    for vb in (v0, v1):
        vs, cm = synth.make_vis_cmap(vb, f)
        verts.append(vb); vis.append(np.asarray(vs, np.float32).reshape(-1, 1)); cmap.append(np.asarray(cm, np.float32).reshape(-1, 3))
    S = dict(smpl_verts=np.stack(verts), smpl_faces=np.stack([f, f]), smpl_cmap=np.stack(cmap), smpl_vis=np.stack(vis),
             calibs=bs.subjects(2)["calibs"])
    for a in S.values():
        a.setflags(write=False)
    return S


@lru_cache(maxsize=None)
def big_case():
    S = big_subjects()
    pts = bs.candidate_points(S, 3000, 4)
    occ, K, counts = bo.batch_query_icon(S, planes(2), oracle_mlp(), pts, SDF_CLIP, False)
    return S, pts, occ, K, counts


def assert_high_slots_reached(S, pts):
    for b in range(2):
        h = MeshHandle(*(T(S[k][b:b + 1]) for k in MESH_KEYS))
        assert h.stats()["slots"] > 32768
        faces_hit = h.sdf_query(T(bo.project(S["calibs"][b], pts[b])))["face"].cpu().numpy()
        assert faces_hit.max() > 40000, b            # as test_mesh_with_more_slots_than_15_bits: triangles stored beyond slot 32,768


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_big_meshes_in_a_batch_vs_oracle(precision):
    """every batched consumer of the nearest-triangle hand-over reads the byte of higher slot bits: k_sign_wide<true>, the fused
    feature phase (f16x3) and k_features<..., Src::Batch> (f32)"""
    S, pts, occ, K, counts = big_case()
    guards(K, counts, 2, 3000)
    assert_high_slots_reached(S, pts)
    eng, feats = engine(S, planes(2), "reference", precision)
    compare(device_query(eng, feats, pts, S["calibs"]), occ, None, f"big meshes n=3000 reference {precision} K={K}")


def test_big_meshes_packet_search_equals_single_subject_calls():
    S, n = big_subjects(), 49153
    assert 2 * n >= PACKET_MIN and n % 64 != 0
    pts = bs.candidate_points(S, n, 6)
    assert_high_slots_reached(S, pts)
    eng, feats = engine(S, planes(2), "local")
    batched = device_query(eng, feats, pts, S["calibs"])
    for b, single in enumerate(single_calls(S, feats, pts)):
        diff = (batched[b] != single).nonzero().flatten()
        assert diff.numel() == 0, f"subject {b}: {diff.numel()} of {n} points differ, first call positions {diff[:8].tolist()}"


# ---------------------------------------------------------------------------------------------
# unlike subjects
# ---------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def unlike_case():
    """subject 1 shrunk to 0.3x and shifted under points drawn around its former surface: nearly all outliers; subject 2 with
    points inside the band only: no outlier"""
    B, n = 4, 1001
    S = {k: v.copy() for k, v in bs.subjects(B).items()}
    pts = bs.candidate_points(S, n, 2).copy()
    v = S["smpl_verts"][1].astype(np.float64)
    c = 0.5 * (v.min(0) + v.max(0))
    S["smpl_verts"][1] = ((v - c) * 0.3 + c + np.array([0.0, 0.0, 0.2])).astype(np.float32)
    vs, cm = synth.make_vis_cmap(S["smpl_verts"][1], S["smpl_faces"][1])
    S["smpl_vis"][1], S["smpl_cmap"][1] = np.asarray(vs, np.float32).reshape(-1, 1), np.asarray(cm, np.float32).reshape(-1, 3)
    rng = np.random.RandomState(12)
    K2 = S["calibs"][2].astype(np.float64)
    near = S["smpl_verts"][2][rng.randint(0, S["smpl_verts"].shape[1], n)].astype(np.float64) + rng.uniform(-0.01, 0.01, (n, 3))
    pts[2] = ((near - K2[:3, 3]) @ np.linalg.inv(K2[:3, :3]).T).astype(np.float32)
    occ, K, counts = bo.batch_query_icon(S, planes(B), oracle_mlp(), pts, SDF_CLIP, False)
    return S, pts, occ, K, counts


def test_unlike_subjects_vs_oracle():
    """the batch-global list is far from an even mix of the subjects"""
    S, pts, occ, K, counts = unlike_case()
    B, n = pts.shape[:2]
    assert 0.95 * n <= counts[1] < n and counts[2] == 0, counts.tolist()
    assert 0 < counts[0] < n and 0 < counts[3] < n and 0.1 <= K / (B * n) <= 0.9
    eng, feats = engine(S, planes(B), "reference")
    compare(device_query(eng, feats, pts, S["calibs"]), occ, None, f"unlike subjects, outliers per subject {counts.tolist()}")


# ---------------------------------------------------------------------------------------------
# one engine across calls of changing B and n; the [B,3,4] calibration layout
# ---------------------------------------------------------------------------------------------
def test_one_engine_across_changing_shapes():
    shapes = [(5, 1001), (2, 50001), (5, 1001), (8, 300)]
    assert 2 * 50001 >= PACKET_MIN

    def call(eng, B, n):
        S = bs.subjects(B)
        eng.set_mesh(*(T(S[k]) for k in MESH_KEYS))
        return eng.query([T(planes(B))], T(bs.candidate_points(S, n, 8).transpose(0, 2, 1)), T(S["calibs"]))[0]

    one, _ = engine(bs.subjects(5), planes(5))
    got = []
    for B, n in shapes:
        got.append(call(one, B, n).clone())
        if B * n >= PACKET_MIN:
            assert torch.equal(call(one, B, n), got[-1]), "two runs of the packet call differ"
    assert torch.equal(got[2], got[0]), "(5, 1001) after the packet call differs from (5, 1001) before it"
    for (B, n), g in zip(shapes, got):
        fresh, _ = engine(bs.subjects(B), planes(B))
        assert torch.equal(call(fresh, B, n), g), f"({B}, {n}) on the reused engine differs from a fresh engine"


def test_calibrations_of_three_rows():
    B, n = 5, 1001
    S = bs.subjects(B)
    eng, feats = engine(S, planes(B))
    pts = T(bs.candidate_points(S, n, 1).transpose(0, 2, 1))
    full = eng.query(feats, pts, T(S["calibs"]))[0]
    rows3 = eng.query(feats, pts, T(S["calibs"][:, :3, :]))[0]
    assert tuple(T(S["calibs"][:, :3, :]).shape) == (B, 3, 4) and torch.equal(full, rows3)

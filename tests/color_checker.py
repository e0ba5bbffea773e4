"""CPU checker of query_color (lib/common/render.py:60-84) and the meshes its tests run on.

The checker composes three leaves that already have checkers of their own - oracle.visibility (the z-buffer rule),
oracle.vertex_normals (S1) and torch's CPU grid_sample - with the same float32 torch operators the reference applies around
them, so it can be compared for equality with the reference's own function where that tree is present
(reference_query_color below runs it verbatim) and with the HIP call everywhere else."""
import ast
import os

import numpy as np
import torch

from common import assets, orc, synth

IMAGE_SEED = 531                       # apps/infer.py:531, the call site
IMAGE_SIZE = 64


def make_image(size=IMAGE_SIZE, seed=IMAGE_SEED):
    """[1,3,size,size] float32 in [-1,1]: smooth but non-constant (a wrong tap or a flipped axis shows), seeded"""
    x = synth.make_feature_planes(3, size, seed)[0]
    return torch.from_numpy(np.tanh(x).astype(np.float32))[None].contiguous()


def checker_query_color(verts, faces, image):
    """-> (colors [V,3] float32 tensor, vis [V] float32 numpy) - render.py:72-84 with the leaves bound to the oracle"""
    verts = torch.as_tensor(verts).float()
    faces = torch.as_tensor(faces).long()
    (xy, z) = verts.split([2, 1], dim=1)
    vis = orc.visibility(xy.numpy(), z.numpy(), faces[:, [0, 2, 1]].numpy(), 4096)[:, 0]
    visibility = torch.from_numpy(vis)
    uv = xy.unsqueeze(0).unsqueeze(2)
    uv = uv * torch.tensor([1.0, -1.0]).type_as(uv)
    colors = (torch.nn.functional.grid_sample(image, uv, align_corners=True)[0, :, :, 0].permute(1, 0) + 1.0) * 0.5 * 255.0
    normals = torch.from_numpy(orc.vertex_normals(verts.numpy(), faces.numpy()))
    colors[visibility == 0.0] = ((normals + 1.0) * 0.5 * 255.0)[visibility == 0.0]
    return colors.detach(), vis


def assert_both_branches(vis, least=0.2):
    """a mesh whose vertices (nearly) all take one branch would let a test pass with the other branch broken"""
    frac = float((np.asarray(vis) != 0).mean())
    assert least <= frac <= 1.0 - least, f"visible fraction {frac:.3f}: each branch needs at least {least:.0%} of the vertices"
    return frac


def sampled_branch_f64(verts, image):
    """((grid_sample + 1) * 0.5) * 255 in float64 numpy from the float32 inputs: bilinear, zeros padding, align_corners=True"""
    v = np.asarray(verts, np.float64)
    img = image[0].numpy().astype(np.float64)
    _, H, W = img.shape
    ix, iy = (v[:, 0] + 1) / 2 * (W - 1), (-v[:, 1] + 1) / 2 * (H - 1)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    out = np.zeros((len(v), 3))
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            w = (1 - np.abs(ix - xi)) * (1 - np.abs(iy - yi))
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            tap = img[:, np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)].T
            out += np.where(ok[:, None], tap, 0.0) * w[:, None]
    return (out + 1.0) * 0.5 * 255.0


# ---------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------
def body():
    a = assets("body")
    return a.smpl_verts[0].astype(np.float32), a.smpl_faces[0].astype(np.int64)


def ico():
    v, f = synth.icosphere(3, radius=0.55, center=(0.05, -0.1, 0.02))
    return v.astype(np.float32), f.astype(np.int64)


def ico_offset():
    """the level-3 icosphere pushed over the right and upper borders of the image: part of it samples the zero padding"""
    v, f = synth.icosphere(3, radius=0.55, center=(0.75, -0.8, 0.02))
    return v.astype(np.float32), f.astype(np.int64)


def bumpy_ico():
    """level-7 icosphere (163,842 vertices, 327,680 faces) with a radial bump field deep enough to occlude itself"""
    v, f = synth.icosphere(7, radius=1.0, center=(0.0, 0.0, 0.0))
    v = v.astype(np.float64)
    d = v / np.linalg.norm(v, axis=1, keepdims=True)
    bump = 1.0 + 0.18 * np.sin(9.0 * d[:, 0] + 1.0) * np.sin(7.0 * d[:, 1]) * np.cos(8.0 * d[:, 2])
    return (v * bump[:, None] * 0.62 + np.array([0.03, -0.02, 0.01])).astype(np.float32), f.astype(np.int64)


def fan(n=1500):
    """a cone of n triangles around ONE apex vertex (valence n) with an irregular rim, hidden behind a cap: a flat m x m grid
    that faces the camera and covers the whole fan (query_color passes z as it is and get_visibility negates it: the largest z
    is nearest).  The rim's radii and heights are random, so the apex normal is a long sum of unlike terms - its float32
    value depends on the order of the additions.  The cap's vertices are the visible branch (over 20 % of the mesh)."""
    rng = np.random.RandomState(4)
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = rng.uniform(0.12, 0.3, n)
    rim = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-0.1, 0.1, n)], 1)
    apex = np.array([[0.005, -0.01, 0.175]])
    k = np.arange(n)
    fan_f = np.stack([np.zeros(n, np.int64), 1 + k, 1 + (k + 1) % n], 1)
    m = 24
    g = np.linspace(-0.45, 0.45, m)
    gx, gy = np.meshgrid(g, g)
    ca, sa = np.cos(0.0371), np.sin(0.0371)                         # slightly rotated: no cap edge runs through a row of pixel centres
    cap = np.stack([ca * gx.ravel() - sa * gy.ravel() + 1.3e-4, sa * gx.ravel() + ca * gy.ravel() - 2.9e-4, np.full(m * m, 0.3)], 1)
    c0 = 1 + n
    i, j = np.meshgrid(np.arange(m - 1), np.arange(m - 1))
    q = (c0 + j * m + i).ravel()                                    # counter-clockwise in xy: the normal points at the camera
    cap_f = np.concatenate([np.stack([q, q + 1, q + m + 1], 1), np.stack([q, q + m + 1, q + m], 1)])
    v = np.concatenate([apex, rim, cap]).astype(np.float32)
    return v, np.concatenate([fan_f, cap_f]).astype(np.int64)


MESHES = {"body": body, "ico": ico, "ico_offset": ico_offset}


# ---------------------------------------------------------------------------------------------
# the reference's own function, verbatim
# ---------------------------------------------------------------------------------------------
def reference_available():
    from oracle import ref_loader
    return ref_loader.available()


def reference_query_color():
    """``query_color`` of lib/common/render.py, compiled from that file's own AST node into a namespace whose two leaves are
    bound to the oracle: get_visibility -> oracle.visibility, Meshes -> the loader's stand-in (oracle.vertex_normals).  The
    module itself cannot be imported: it pulls pytorch3d's renderer in at module level."""
    import sys
    from oracle import ref_loader
    ref_loader.load()
    path = os.path.join(ref_loader.REFERENCE_ROOT, "lib", "common", "render.py")
    tree = ast.parse(open(path).read(), path)
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "query_color")

    def get_visibility(xy, z, faces):
        return torch.from_numpy(orc.visibility(xy.cpu().numpy(), z.cpu().numpy(), faces.cpu().numpy(), 4096))

    ns = {"torch": torch, "np": np, "get_visibility": get_visibility, "Meshes": sys.modules["pytorch3d.structures"].Meshes}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns["query_color"]


# ---------------------------------------------------------------------------------------------
# tolerances
# ---------------------------------------------------------------------------------------------
# Largest |checker - float64 restatement| of the sampled branch over the test meshes, in colour units (0..255), measured by
# tests/test_query_color.py::test_checker_sampled_branch_vs_float64 (body 6.07e-4, icosphere 5.00e-4, offset icosphere
# 5.83e-4, fan 5.12e-4, bumped level-7 icosphere 6.75e-4): float32 rounding of the pixel coordinate (|ix| <= 63, half an ulp
# = 1.9e-6) times the image's slope (up to ~1 per pixel) times 127.5, plus the rounding of the result itself (ulp(255)/2 = 7.6e-6).
SAMPLED_F64_FIGURE = 6.8e-4
# the HIP call's sampled branch against the checker: 4 x that figure - room for another, equally valid float32 ordering
SAMPLED_GPU_BAR = 4 * SAMPLED_F64_FIGURE

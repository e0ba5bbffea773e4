"""The soft silhouette (icon_amd.render.silhouette_device) stated in torch - PARITY UNPINNED: the rule is
restated from pytorch3d's published pipeline (MeshRasterizer with blur_radius = log(1/1e-4 - 1) * 5e-5, cull_backfaces=True,
SoftSilhouetteShader with sigma = 1e-4), not held against the package.

Brute force: every pixel centre of a chunk of rows against every face that can reach the chunk.  dtype-generic: run in float64
it is the reference statement, run in float32 on the CPU it is the yardstick the device's tolerances are taken from.  Camera and
projection are render_checker.look_at_f64 / ortho_matrix_f64 (the matrices, cast to the dtype); the winning edge is chosen with
explicit ``where`` selections (the first minimum in the order (v0,v1), (v0,v2), (v1,v2)); gradients are torch autograd's.
The candidate set and the culling are piecewise constant: they are computed without gradient and applied as masks."""
import numpy as np
import torch

import color_checker as cc
import render_checker as rc

SIGMA = 1e-4                                            # BlendParams().sigma
BLUR_SIL = float(np.log(1.0 / 1e-4 - 1.0) * 5e-5)       # RasterizationSettings.blur_radius of the silhouette renderer: 4.60512e-4
EPS = 1e-8                                              # pytorch3d's kEpsilon
EXCL_BLUR_REL = 1e-4                                    # |m - BLUR_SIL| <= this * BLUR_SIL: candidate status may flip in float32
EXCL_AREA = 1e-6                                        # a face of |area| <= this that reaches the pixel: the cull may flip
EXCLUDED_BAR = 0.0102                                   # one flipped pair moves alpha by at most sigmoid(-BLUR_SIL / sigma) = 0.0099
EXCLUDED_CAP = 0.02                                     # excluded pixels <= 2 % of the pixels with alpha > 0


def sliver():
    """face 0: a triangle whose grown box lies half outside the image (two borders cut it in both views); face 1: a long thin
    triangle; face 2: in the plane x + z = const and wound so that its projected area is negative for BOTH requested cameras
    (0 and 1: a face cannot turn its back on cameras 0 and 2 at once) - nothing may be drawn for it, and it is the only face in its
    part of the image.  Both front-facing triangles face the bisector of the two cameras too."""
    v = np.array([[0.62, 0.71, 0.75], [1.18, 0.83, 0.30], [0.80, 1.21, 0.66],
                  [-0.10, -0.52, 0.50], [0.45, -0.47, -0.30], [-0.08, -0.44, 0.49],
                  [-0.50, 0.10, -0.40], [-0.50, 0.50, -0.40], [-0.288, 0.10, -0.612]], np.float32)
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int64)
    return v, f


def fan():
    """render_checker's fan, 1.6 times as large.  As it stands 62 of its 1,226 silhouette pixels (5.1 %) lie within reach of one of
    the 14 fan faces whose projected |area| is <= 1e-6 - above the 2 % cap on excluded pixels; the count of such faces falls with
    the square of the scale, the silhouette grows with it"""
    v, f = cc.fan()
    return (v * np.float32(1.6)).astype(np.float32), f


def body():
    """render_checker's body, 2.5 times as large about (0, 0.1, 0): a torso that leaves the image on all four sides.
    As it stands 622 of its 5,716 silhouette pixels at 128^2 (11.2 %) lie within reach of a face seen edge-on (|area| <= 1e-6: the
    rim of every limb) - above the 2 % cap; the share falls with the fourth power of the scale"""
    v, f = rc.body()
    c = np.array([0.0, 0.1, 0.0], np.float32)
    return ((v - c) * np.float32(2.5) + c).astype(np.float32), f


# name -> (builder, image size, cameras): render_checker's seven, with their sizes and cameras (fan and body rescaled to meet
# the cap on excluded pixels), and one of our own
CASES = dict(rc.CASES)
CASES["fan"] = (fan,) + rc.CASES["fan"][1:]
CASES["body"] = (body,) + rc.CASES["body"][1:]
CASES["sliver"] = (sliver, 48, (0, 1))


def project(verts, cam, dtype):
    """-> NDC X (+X is left), NDC Y (+Y is up), view depth D as [V] tensors of `dtype` (differentiable in verts)"""
    R, T = rc.look_at_f64(rc.CAM_EYES[cam])
    K = rc.ortho_matrix_f64()
    view = verts @ torch.as_tensor(R, dtype=dtype) + torch.as_tensor(T, dtype=dtype)
    ndc = torch.cat([view, torch.ones_like(view[:, :1])], 1) @ torch.as_tensor(K.T, dtype=dtype)
    return ndc[:, 0], ndc[:, 1], view[:, 2]


def _centre(i, S, dtype):
    return -1.0 + (2 * i + 1).to(dtype) / torch.tensor(float(S), dtype=dtype)


def _ef(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def _seg(px, py, ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    deg = l2 <= EPS
    t = (dx * (px - ax) + dy * (py - ay)) / torch.where(deg, torch.ones_like(l2), l2)
    tt = torch.clamp(t, 0.0, 1.0)
    qx = torch.where(deg, bx + 0 * px, ax + tt * dx)
    qy = torch.where(deg, by + 0 * py, ay + tt * dy)
    ex, ey = px - qx, py - qy
    return ex * ex + ey * ey


def silhouette(verts, faces, cam_ids, S, dtype=torch.float64, faces_per_pixel=None, flip=None, grad_alpha=None, zero_excluded=False,
               tile=(8, 16)):
    """-> dict: ``alpha`` [n,S,S], ``count`` [n,S,S] (candidates per pixel, before any truncation), ``excl_blur`` / ``excl_area``
    [n,S,S] bool (the two exclusion conditions, evaluated in `dtype`: meant to be read from the float64 run), all numpy, in the
    orientation of the output (camera 2 mirrored left-right when `flip`; default: exactly two views); with ``grad_alpha``
    [n,S,S] also ``grad_verts`` [V,3]: the gradient of sum(alpha * grad_alpha), grad_alpha taken as 0 on this run's excluded pixels with ``zero_excluded``
    (``grad_alpha`` may be a function (view, rows, columns, alpha there) -> values: a loss's own derivative, in one pass).
    ``faces_per_pixel``: None takes all candidates (the native rule); a number keeps that many per pixel, nearest first by (depth, face id) as render_blend_f64 ranks them."""
    v = torch.tensor(np.asarray(verts, np.float64), dtype=dtype, requires_grad=grad_alpha is not None)
    f_all = np.asarray(faces, np.int64)
    f_all = f_all[rc.good_faces(f_all, len(v))]
    n = len(cam_ids)
    flip = (n == 2) if flip is None else flip
    alpha = np.zeros((n, S, S))
    count = np.zeros((n, S, S), np.int64)
    excl_blur = np.zeros((n, S, S), bool)
    excl_area = np.zeros((n, S, S), bool)
    reach = float(np.sqrt(BLUR_SIL)) * 1.01 + 2.0 / S
    repeats = (f_all[:, 0] == f_all[:, 1]) | (f_all[:, 1] == f_all[:, 2]) | (f_all[:, 0] == f_all[:, 2])
    ft = torch.from_numpy(f_all)
    for k, cam in enumerate(cam_ids):
        with torch.no_grad():
            X, Y, _ = project(v, cam, dtype)
            area_all = _ef(X[ft[:, 2]], Y[ft[:, 2]], X[ft[:, 0]], Y[ft[:, 0]], X[ft[:, 1]], Y[ft[:, 1]])
            # a face that is neither drawn nor close to the cull's thresholds has no say anywhere.  (A face that repeats a vertex
            # has area exactly 0 in every precision: its cull cannot flip, and it excludes nothing.)
            tiny_all = (area_all.abs() <= EXCL_AREA) & ~torch.from_numpy(repeats)
            matters = ((area_all.abs() > EPS) & ~(area_all < 0)) | tiny_all
            xlo, xhi = X[ft].min(1).values - reach, X[ft].max(1).values + reach
            ylo, yhi = Y[ft].min(1).values - reach, Y[ft].max(1).values + reach
        mirror = flip and cam == 2
        for r0, c0 in ((r, c) for r in range(0, S, tile[0]) for c in range(0, S, tile[1])):
            rows, cols = torch.arange(r0, min(S, r0 + tile[0])), torch.arange(c0, min(S, c0 + tile[1]))
            py_rows, px_cols = _centre(S - 1 - rows, S, dtype), _centre(S - 1 - cols, S, dtype)
            keep = torch.nonzero(matters & (ylo <= py_rows.max()) & (yhi >= py_rows.min()) &
                                 (xlo <= px_cols.max()) & (xhi >= px_cols.min())).ravel()
            if not len(keep):
                continue
            px = px_cols.repeat(len(rows))[:, None]                                    # [P,1]
            py = py_rows.repeat_interleave(len(cols))[:, None]
            X, Y, D = project(v, cam, dtype)
            fk = ft[keep]
            x0, x1, x2 = X[fk[:, 0]][None], X[fk[:, 1]][None], X[fk[:, 2]][None]         # [1,F']
            y0, y1, y2 = Y[fk[:, 0]][None], Y[fk[:, 1]][None], Y[fk[:, 2]][None]
            area = area_all[keep][None]
            live = (area.abs() > EPS) & ~(area < 0)
            den = area + EPS
            s01, s02, s12 = _seg(px, py, x0, y0, x1, y1), _seg(px, py, x0, y0, x2, y2), _seg(px, py, x1, y1, x2, y2)
            m = torch.where(s02 < s01, s02, s01)                                       # the first minimum wins
            m = torch.where(s12 < m, s12, m)
            with torch.no_grad():
                w0, w1, w2 = _ef(px, py, x1, y1, x2, y2) / den, _ef(px, py, x2, y2, x0, y0) / den, _ef(px, py, x0, y0, x1, y1) / den
                inside = (w0 > 0) & (w1 > 0) & (w2 > 0)
                c_0, c_1, c_2 = (torch.clamp(w, 0.0, 1.0) for w in (w0, w1, w2))
                s = torch.clamp((c_0 + c_1) + c_2, min=1e-5)
                pz = ((c_0 / s) * D[fk[:, 0]][None] + (c_1 / s) * D[fk[:, 1]][None]) + (c_2 / s) * D[fk[:, 2]][None]
                cand = live & (inside | (m < BLUR_SIL)) & ~(pz < 0)
                cnt = cand.sum(1)
                eb = (live & ((m - BLUR_SIL).abs() <= EXCL_BLUR_REL * BLUR_SIL)).any(1)
                ea = (tiny_all[keep][None] & (m < BLUR_SIL)).any(1)
                if faces_per_pixel is not None:
                    key = torch.where(cand, pz, torch.full_like(pz, float("inf")))
                    order = torch.argsort(key, dim=1, stable=True)                     # ties: ascending face id (keep is ascending)
                    rank = torch.empty_like(order)
                    rank.scatter_(1, order, torch.arange(order.shape[1]).expand_as(order).contiguous())
                    cand = cand & (rank < faces_per_pixel)
            d = torch.where(cand, torch.where(inside, -m, m), torch.zeros_like(m))      # non-candidates: no exp of a huge number
            prob = torch.where(cand, 1.0 / (1.0 + torch.exp(d / SIGMA)), torch.zeros_like(d))
            a = 1.0 - torch.prod(1.0 - prob, dim=1)                                     # [P]
            r_out = rows.repeat_interleave(len(cols)).numpy()
            c_out = cols.repeat(len(rows)).numpy()
            if mirror:
                c_out = S - 1 - c_out
            if grad_alpha is not None:
                ga = grad_alpha(k, r_out, c_out, a.detach().numpy()) if callable(grad_alpha) else np.asarray(grad_alpha)[k, r_out, c_out]
                ga = torch.as_tensor(ga, dtype=dtype)
                if zero_excluded:
                    ga = ga * ~(eb | ea)
                (a * ga).sum().backward()
            alpha[k, r_out, c_out] = a.detach().numpy()
            count[k, r_out, c_out] = cnt.numpy()
            excl_blur[k, r_out, c_out] = eb.numpy()
            excl_area[k, r_out, c_out] = ea.numpy()
    out = dict(alpha=alpha, count=count, excl_blur=excl_blur, excl_area=excl_area)
    if grad_alpha is not None:
        out["grad_verts"] = v.grad.detach().numpy().astype(np.float64) if v.grad is not None else np.zeros((len(v), 3))
    return out


def smooth_field(n, S, seed=414):
    """the fixed, seeded, smooth grad_alpha of the gradient comparisons: a few low-frequency waves per view, values in [-1, 1]"""
    rs = np.random.RandomState(seed)
    c = (np.arange(S) + 0.5) / S
    x, y = np.meshgrid(c, c)
    out = np.zeros((n, S, S))
    for k in range(n):
        for _ in range(4):
            fx, fy, ph = rs.uniform(0.5, 3.0), rs.uniform(0.5, 3.0), rs.uniform(0, 2 * np.pi)
            out[k] += rs.uniform(0.3, 1.0) * np.sin(2 * np.pi * (fx * x + fy * y) + ph)
        out[k] /= np.abs(out[k]).max()
    return out


_cache = {}


def case(name):
    """-> dict(verts, faces, S, cams, grad_alpha, excluded, f64, f32): the float64 and float32 oracle runs of one case with the
    smooth grad_alpha (zero on the excluded pixels) - computed once per process, shared by the tests, never written to"""
    if name not in _cache:
        fn, S, cams = CASES[name]
        v, f = fn()
        f64 = silhouette(v, f, cams, S, grad_alpha=smooth_field(len(cams), S), zero_excluded=True)
        excluded = f64["excl_blur"] | f64["excl_area"]                     # the float64 run decides what is excluded
        ga = smooth_field(len(cams), S) * ~excluded
        f32 = silhouette(v, f, cams, S, dtype=torch.float32, grad_alpha=ga)
        for d in (f64, f32):
            for a in d.values():
                a.setflags(write=False)
        ga.setflags(write=False)
        _cache[name] = dict(verts=v, faces=f, S=S, cams=cams, grad_alpha=ga, excluded=excluded, f64=f64, f32=f32)
    return _cache[name]


def truncation_report(name, S=None):
    """how far pytorch3d's 50-faces-per-pixel storage limit moves the silhouette: (pixels with more than 50 candidates,
    largest |alpha_all - alpha_50|, largest candidate count), float64"""
    fn, S0, cams = rc.CASES[name] if name in rc.CASES else CASES[name]     # the meshes as render_checker has them: unscaled
    S = S or S0
    v, f = fn()
    a_all = silhouette(v, f, cams, S)
    a_50 = silhouette(v, f, cams, S, faces_per_pixel=50)
    return int((a_all["count"] > 50).sum()), float(np.abs(a_all["alpha"] - a_50["alpha"]).max()), int(a_all["count"].max())


# ---------------------------------------------------------------------------------------------
# the descent of the GPU test: ico at 64^2, cameras 0 and 2, towards the silhouette of the sphere shifted by DESCENT_SHIFT.
# The loss is the SMOOTH one, sum (alpha - target)^2 / (2 S^2): the L1 loss's gradient sign(alpha - target) jumps whenever a pixel
# crosses its target - one pixel moves the gradient by ~3 % here - so its trajectory is not a function any float32 evaluation could
# follow to 1e-6 (measured: the device agreed to 2e-9 and 1.5e-8 on the first two steps and was 7e-4 off by the eighth).
# A pixel whose alpha is off by e moves this loss by at most |alpha - target| e / S^2 <= e / S^2.
# ---------------------------------------------------------------------------------------------
DESCENT_SHIFT = (0.06, -0.04, 0.0)
DESCENT_STEPS = 10
DESCENT_LR = 0.02          # plain gradient steps on the translation; the float64 loss below falls at every step (asserted)


def l1_loss_and_grad(alpha, target):
    """loss = sum |alpha - target| / S^2 (over all views) and its derivative with respect to alpha"""
    S = alpha.shape[-1]
    return float(np.abs(alpha - target).sum()) / (S * S), np.sign(alpha - target) / (S * S)


def l2_loss(alpha, target):
    S = alpha.shape[-1]
    return float(((alpha - target) ** 2).sum()) / (2 * S * S)


def descent_f64():
    """-> target [2,S,S], losses [DESCENT_STEPS + 1] of the float64 oracle, pixels that differ from the target at each of them"""
    if "descent" not in _cache:
        fn, S, _ = CASES["ico"]
        v, f = fn()
        cams = (0, 2)
        target = silhouette(v.astype(np.float64) + np.array(DESCENT_SHIFT), f, cams, S)["alpha"]
        trans = np.zeros(3)
        losses, ndiff = [], []
        for _ in range(DESCENT_STEPS + 1):
            out = silhouette(v.astype(np.float64) + trans, f, cams, S,
                             grad_alpha=lambda k, r, c, a: (a - target[k, r, c]) / (S * S))
            ndiff.append(int((out["alpha"] != target).sum()))
            losses.append(l2_loss(out["alpha"], target))
            trans = trans - DESCENT_LR * out["grad_verts"].sum(0)
        _cache["descent"] = (target, np.array(losses), np.array(ndiff))
    return _cache["descent"]

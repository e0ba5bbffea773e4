"""The gradient of the normal maps with respect to the vertices (icon_amd.render.render_normal_device(differentiable=True);
DESIGN.md 4.15) stated in torch - PARITY UNPINNED like 4.13: restated from pytorch3d's published pipeline
(TexturesVertex(verts_normals_padded()) interpolated by differentiable barycentrics), not held against the package.

Given ``pix_to_face``, ``images`` evaluates the WINNER's colour at every covered pixel, differentiably in the vertices: the
projection is silhouette_oracle.project (the look-at camera and the projection matrix), the normals are index_add sums of the
face cross products, the two clamps of the rule (the barycentrics' [0, 1], the sums' 1e-5) and the normalisation's 1e-6 are explicit
``where`` selections - so |N| = 0 gives no NaN - and the gradients are torch autograd's.  dtype-generic: run in float64 it is the
reference, run in float32 on the CPU it is the yardstick the device's bar is taken from.  Taking the winners as input removes
winner flips from the comparison (the GPU tests hold them bit-equal to render_checker.render_f32 first).

``blend_images`` restates render_checker.render_blend_f64 - the full soft blend - in torch float64: the record of how far the
winner's gradient is from the blend's is taken with it."""
import numpy as np
import torch

import color_checker as cc
import render_checker as rc
import silhouette_oracle as so

EPS = 1e-8                     # pytorch3d's kEpsilon
EXCL_W = 1e-4                  # a barycentric of the winner within this of 0 or of 1: the clamp pattern may flip in float32
EXCL_AREA = 1e-6               # a winner of |area| <= this
EXCLUDED_CAP = 0.02            # excluded pixels <= 2 % of the covered pixels

# name -> (builder, image size, cameras): render_checker's seven as they are, and the icosphere at 16^2 (1,280 faces under a pixel)
CASES = dict(rc.CASES)
CASES["ico16"] = (cc.ico, 16, (0, 1, 2, 3))


def _ef(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def normal_sums(v, f_good):
    """S1's N_v: the sum of (v1 - v0) x (v2 - v0) over the incident good faces (index_add)"""
    ft = torch.as_tensor(f_good)
    fn = torch.cross(v[ft[:, 1]] - v[ft[:, 0]], v[ft[:, 2]] - v[ft[:, 0]], dim=1)
    N = torch.zeros_like(v)
    for k in range(3):
        N = N.index_add(0, ft[:, k], fn)
    return N


def normalise(N):
    """n = N / max(|N|, 1e-6), the branch explicit: where |N| <= 1e-6, n = N 1e6 and no square root is differentiated at 0"""
    len2 = (N * N).sum(1, keepdim=True)
    big = torch.sqrt(len2.detach()) > 1e-6
    length = torch.sqrt(torch.where(big, len2, torch.ones_like(len2)))
    return torch.where(big, N / length, N * 1e6)


def vertex_normals(v, f_good):
    return normalise(normal_sums(v, f_good))


def _winner_terms(v, faces, pix, cam_ids, S, dtype, flip):
    """per view: (rows, output columns, barycentrics w [3][P], area [P], vertex ids [P,3]) of the covered pixels"""
    f_all = torch.as_tensor(np.asarray(faces, np.int64))
    out = []
    for k, cam in enumerate(cam_ids):
        row, col_out = np.nonzero(np.asarray(pix[k]) >= 0)
        col = S - 1 - col_out if (flip and cam == 2) else col_out
        ids = f_all[torch.as_tensor(np.asarray(pix[k])[row, col_out].astype(np.int64))]
        X, Y, _ = so.project(v, cam, dtype)
        px = so._centre(torch.as_tensor(S - 1 - col), S, dtype)
        py = so._centre(torch.as_tensor(S - 1 - row), S, dtype)
        x, y = [X[ids[:, c]] for c in range(3)], [Y[ids[:, c]] for c in range(3)]
        area = _ef(x[2], y[2], x[0], y[0], x[1], y[1])
        den = area + EPS
        w = [_ef(px, py, x[1], y[1], x[2], y[2]) / den, _ef(px, py, x[2], y[2], x[0], y[0]) / den, _ef(px, py, x[0], y[0], x[1], y[1]) / den]
        out.append((row, col_out, w, area, ids))
    return out


def images(v, faces, pix, cam_ids, S, flip=None):
    """-> [n,3,S,S] tensor of v's dtype, differentiable in v [V,3]: the winner's colour of DESIGN.md 4.13 where pix >= 0, else 0"""
    dtype = v.dtype
    n = len(cam_ids)
    flip = (n == 2) if flip is None else flip
    f_np = np.asarray(faces, np.int64)
    nrm = vertex_normals(v, f_np[rc.good_faces(f_np, len(v))])
    planes = []
    for row, col_out, w, _, ids in _winner_terms(v, faces, pix, cam_ids, S, dtype, flip):
        c = [torch.where((wk > 0) & (wk < 1), wk, wk.detach().clamp(0.0, 1.0)) for wk in w]      # gradient only where 0 < w < 1
        sraw = (c[0] + c[1]) + c[2]
        s = torch.where(sraw > 1e-5, sraw, torch.full_like(sraw, 1e-5))                          # ... and only where the sum exceeds 1e-5
        b = [ck / s for ck in c]
        t = [(nrm[ids[:, k]] + 1.0) * 0.5 for k in range(3)]                                     # [P,3]
        colour = (((b[0][:, None] * t[0] + b[1][:, None] * t[1]) + b[2][:, None] * t[2]) - 0.5) * 2.0
        img = torch.zeros((3, S * S), dtype=dtype)
        planes.append(img.index_copy(1, torch.as_tensor(row * S + col_out), colour.T).reshape(3, S, S))
    return torch.stack(planes)


def excluded(verts, faces, pix, cam_ids, S, flip=None):
    """-> [n,S,S] bool, float64: some w_k of the winner within EXCL_W of 0 or of 1, or the winner's |area| <= EXCL_AREA"""
    n = len(cam_ids)
    flip = (n == 2) if flip is None else flip
    v = torch.tensor(np.asarray(verts, np.float64))
    out = np.zeros((n, S, S), bool)
    for k, (row, col_out, w, area, _) in enumerate(_winner_terms(v, faces, pix, cam_ids, S, torch.float64, flip)):
        near = area.abs() <= EXCL_AREA
        for wk in w:
            near = near | (wk.abs() <= EXCL_W) | ((wk - 1.0).abs() <= EXCL_W)
        out[k, row, col_out] = near.numpy()
    return out


def grad_field(n, S, seed=415):
    """the fixed, seeded, smooth grad_images [n,3,S,S] of the comparisons: silhouette_oracle.smooth_field per view and channel"""
    return so.smooth_field(3 * n, S, seed=seed).reshape(n, 3, S, S)


def loss_and_grad(verts, faces, pix, cam_ids, S, grad_images, dtype=torch.float64, flip=None):
    """-> sum(images * grad_images) and its gradient [V,3] (float64 numpy), evaluated in `dtype`"""
    v = torch.tensor(np.asarray(verts, np.float64), dtype=dtype, requires_grad=True)
    loss = (images(v, faces, pix, cam_ids, S, flip) * torch.as_tensor(np.asarray(grad_images), dtype=dtype)).sum()
    loss.backward()
    return float(loss.detach()), v.grad.numpy().astype(np.float64)


_cache = {}


def case(name):
    """-> dict(verts, faces, S, cams, pix, covered, excluded, grad_images, g64, g32): render_f32's winners, the smooth grad_images
    (zero on the excluded pixels), the float64 and the float32 gradient - computed once per process, shared by the tests, never written to"""
    if name not in _cache:
        fn, S, cams = CASES[name]
        if name in rc.CASES:
            v, f, _, _, (pix, _, _) = rc.case(name)
        else:
            v, f = fn()
            pix = rc.render_f32(v, f, cams, S)[0]
        ex = excluded(v, f, pix, cams, S)
        gi = grad_field(len(cams), S) * ~ex[:, None]
        g64 = loss_and_grad(v, f, pix, cams, S, gi)[1]
        g32 = loss_and_grad(v, f, pix, cams, S, gi, dtype=torch.float32)[1]
        for a in (ex, gi, g64, g32):
            a.setflags(write=False)
        _cache[name] = dict(verts=v, faces=f, S=S, cams=cams, pix=pix, covered=int((pix >= 0).sum()), excluded=ex, grad_images=gi, g64=g64, g32=g32)
    return _cache[name]


# ---------------------------------------------------------------------------------------------
# the full soft blend (render_checker.render_blend_f64) in torch float64, differentiable in the vertices
# ---------------------------------------------------------------------------------------------
def blend_images(v, faces, cam_ids, S, flip=None, faces_per_pixel=30, sigma=1e-4, gamma=1e-8, background=0.5, znear=-256.0, zfar=256.0):
    """-> images [n,3,S,S] (differentiable in v), pix_to_face [n,S,S] (the nearest candidate by (depth, face id)), other [n,S,S]: the
    share of the blend's weight that is NOT the nearest candidate's, edge_d2 [n,S,S]: the squared distance of the pixel centre to the
    nearest projected edge of any face.  Every pixel against every face; asserts that no pixel has more than `faces_per_pixel`
    candidates (the truncation is then moot and is not restated)."""
    dt = torch.float64
    f_np = np.asarray(faces, np.int64)
    keep = np.nonzero(rc.good_faces(f_np, len(v)))[0]
    ft = torch.as_tensor(f_np[keep])
    col = (vertex_normals(v, f_np[keep]) + 1.0) * 0.5
    n = len(cam_ids)
    flip = (n == 2) if flip is None else flip
    blur = rc.BLUR
    blur_r = float(np.sqrt(blur))
    imgs, pixs, others, edges = [], [], [], []
    for cam in cam_ids:
        X, Y, Z = so.project(v, cam, dt)
        idx = torch.arange(S, dtype=dt)
        px = (1.0 - (2.0 * idx + 1.0) / S).repeat(S)[:, None]                            # [P,1], P = row * S + column
        py = (1.0 - (2.0 * idx + 1.0) / S).repeat_interleave(S)[:, None]
        x, y, z = [X[ft[:, c]][None] for c in range(3)], [Y[ft[:, c]][None] for c in range(3)], [Z[ft[:, c]][None] for c in range(3)]
        area = (x[2] - x[0]) * (y[1] - y[0]) - (y[2] - y[0]) * (x[1] - x[0])
        live = ~((area <= 1e-8) & (area >= -1e-8))
        den = torch.where(live, area + 1e-8, torch.ones_like(area))
        w = [_ef(px, py, x[1], y[1], x[2], y[2]) / den, _ef(px, py, x[2], y[2], x[0], y[0]) / den, _ef(px, py, x[0], y[0], x[1], y[1]) / den]
        d01, d02, d12 = so._seg(px, py, x[0], y[0], x[1], y[1]), so._seg(px, py, x[0], y[0], x[2], y[2]), so._seg(px, py, x[1], y[1], x[2], y[2])
        dist = torch.where(d02 < d01, d02, d01)
        dist = torch.where(d12 < dist, d12, dist)
        c = [torch.where((wk > 0) & (wk < 1), wk, wk.detach().clamp(0.0, 1.0)) for wk in w]
        sraw = (c[0] + c[1]) + c[2]
        s = torch.where(sraw > 1e-5, sraw, torch.full_like(sraw, 1e-5))
        wc = [ck / s for ck in c]
        pz = (wc[0] * z[0] + wc[1] * z[1]) + wc[2] * z[2]
        with torch.no_grad():
            inside = (w[0] > 0) & (w[1] > 0) & (w[2] > 0)
            xs, ys = torch.cat(x), torch.cat(y)
            inbox = (px >= xs.min(0).values - blur_r) & (px <= xs.max(0).values + blur_r) & (py >= ys.min(0).values - blur_r) & (py <= ys.max(0).values + blur_r)
            cand = live & inbox & (inside | (dist < blur)) & (pz >= 0)
            assert int(cand.sum(1).max()) <= faces_per_pixel
            covered = cand.any(1)
            first = torch.sort(torch.where(cand, pz, torch.full_like(pz, float("inf"))), dim=1, stable=True).indices[:, 0]
            edge = torch.where(live.expand_as(dist), dist, torch.full_like(dist, float("inf"))).min(1).values
        sd = torch.where(cand, torch.where(inside, -dist, dist), torch.zeros_like(dist))
        prob = 1.0 / (1.0 + torch.exp(sd / sigma))
        z_inv = torch.where(cand, (zfar - pz) / (zfar - znear), torch.zeros_like(pz))
        z_inv_max = torch.clamp(z_inv.max(1, keepdim=True).values, min=1e-10)
        wnum = torch.where(cand, prob * torch.exp((z_inv - z_inv_max) / gamma), torch.zeros_like(prob))
        delta = torch.clamp(torch.exp((1e-10 - z_inv_max) / gamma), min=1e-10)
        denom = wnum.sum(1, keepdim=True) + delta
        rgb = []
        for ch in range(3):
            texel = (wc[0] * col[ft[:, 0], ch][None] + wc[1] * col[ft[:, 1], ch][None]) + wc[2] * col[ft[:, 2], ch][None]
            rgb.append(((wnum * texel).sum(1, keepdim=True) + delta * background) / denom)
        img = torch.where(covered[:, None], (torch.cat(rgb, 1) - 0.5) * 2.0, torch.zeros((1, 3), dtype=dt)).T.reshape(3, S, S)
        with torch.no_grad():
            share = (wnum / denom)
            other = share.scatter(1, first[:, None], 0.0).sum(1).reshape(S, S)
            pix = torch.where(covered, torch.as_tensor(keep)[first], torch.full_like(first, -1)).reshape(S, S)
            edge = edge.reshape(S, S)
        if flip and cam == 2:
            img, other, pix, edge = img.flip(2), other.flip(1), pix.flip(1), edge.flip(1)
        imgs.append(img); pixs.append(pix.numpy()); others.append(other.numpy()); edges.append(edge.numpy())
    return torch.stack(imgs), np.stack(pixs), np.stack(others), np.stack(edges)


def blend_difference(name, S=32):
    """the winner's gradient against the full float64 blend's on case `name` at S^2 with the smooth grad_images (zero on the
    excluded pixels) -> dict: rel = ||g_blend - g_winner||inf / ||g_winner||inf; tied [n,S,S]: the pixels where another candidate
    than the nearest holds any of the blend's weight (float64: its share is not exactly 0) - the pixels responsible; rel_rest: the
    same difference with grad_images zero on the tied pixels too (what the 1e-10 background weight alone makes); edge_d2 [n,S,S]"""
    key = ("blend", name, S)
    if key not in _cache:
        fn, _, cams = CASES[name]
        v_np, f = fn()
        n, flip = len(cams), len(cams) == 2
        full = grad_field(n, S)
        g_blend, g_blend_rest = np.zeros(v_np.shape), np.zeros(v_np.shape)
        pix, tied, edge_d2, ex, gi, gi_rest = [], [], [], [], [], []
        for k, cam in enumerate(cams):                                                   # view by view: one view's graph at a time
            v = torch.tensor(np.asarray(v_np, np.float64), requires_grad=True)
            img, p, other, e = blend_images(v, f, (cam,), S, flip=flip)
            x = excluded(v_np, f, p, (cam,), S, flip=flip)
            a = full[k:k + 1] * ~x[:, None]
            b = a * ~(other > 0.0)[:, None]
            g_blend += torch.autograd.grad((img * torch.as_tensor(a)).sum(), v, retain_graph=True)[0].numpy()
            g_blend_rest += torch.autograd.grad((img * torch.as_tensor(b)).sum(), v)[0].numpy()
            pix.append(p[0]); tied.append(other[0] > 0.0); edge_d2.append(e[0]); ex.append(x[0]); gi.append(a[0]); gi_rest.append(b[0])
        pix, tied, edge_d2, ex, gi, gi_rest = (np.stack(a) for a in (pix, tied, edge_d2, ex, gi, gi_rest))
        g_win = loss_and_grad(v_np, f, pix, cams, S, gi)[1]
        g_win_rest = loss_and_grad(v_np, f, pix, cams, S, gi_rest)[1]
        _cache[key] = dict(rel=float(np.abs(g_blend - g_win).max() / np.abs(g_win).max()), tied=tied, edge_d2=edge_d2,
                           rel_rest=float(np.abs(g_blend_rest - g_win_rest).max() / np.abs(g_win_rest).max()),
                           covered=int((pix >= 0).sum()), excluded=int(ex.sum()))
    return _cache[key]

"""Meshes and helpers shared by tests/test_pair_box.py (host) and tests/test_gpu_pair_box.py: the five meshes the oriented pair
boxes are checked on, and the host entry of the rule (icon_debug_pair_box: mesh_rules.h's pair_box_setup / pair_box_bound)."""
import ctypes as C
import importlib.util
import os
from functools import lru_cache

import numpy as np

from common import ROOT, assets, synth


def _load_model():
    spec = importlib.util.spec_from_file_location("pair_box_model", os.path.join(ROOT, "tools", "pair_box_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


model = _load_model()


@lru_cache(maxsize=None)
def mesh(name):
    """(verts f32 [V,3], faces i64 [F,3], cmap f32 [V,3], vis f32 [V]) - the constructions of tests/test_gpu_mesh_build.py"""
    if name in ("ico", "body"):
        a = assets(name)
        v, f = a.smpl_verts[0], a.smpl_faces[0]
        cm, vs = a.smpl_cmap[0], a.smpl_vis[0].reshape(-1)
    else:
        if name == "tiny":                         # a tetrahedron: the root is a leaf
            v = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5]], np.float64) - 0.1
            f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
        elif name == "dup":                        # 3,000 copies of one triangle + a sphere: exact ties
            v0, f0 = synth.icosphere(2, radius=0.3)
            f = np.concatenate([np.tile(f0[:1], (3000, 1)), f0])
            v = v0
        elif name == "line":                       # 2,400 slivers along a line
            t = np.geomspace(1e-6, 0.9, 2401)
            v = np.stack([np.concatenate([t, t]), np.concatenate([np.zeros_like(t), np.full_like(t, 1e-3)]), np.zeros(2 * len(t))], 1)
            i = np.arange(2400)
            f = np.stack([i, i + 1, i + 2401], 1)
        else:
            raise KeyError(name)
        v, f = np.asarray(v, np.float32), np.asarray(f, np.int64)
        vs, cm = synth.make_vis_cmap(v, f)
        cm, vs = np.asarray(cm, np.float32).reshape(-1, 3), np.asarray(vs, np.float32).reshape(-1)
    return (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int64), np.ascontiguousarray(cm, np.float32),
            np.ascontiguousarray(vs, np.float32))


def pair_box(corners, pts, shared):
    """corners [P,6,3] f32; pts [N,3] (shared) or [P,N,3] -> (rec [P,15] f32, kind [P] i32, bound [P,N] f32)"""
    from icon_amd import _lib
    corners = np.ascontiguousarray(corners, np.float32); pts = np.ascontiguousarray(pts, np.float32)
    P = len(corners)
    N = pts.shape[0] if shared else pts.shape[1]
    assert corners.shape == (P, 6, 3) and pts.shape == ((N, 3) if shared else (P, N, 3))
    rec, kind, bound = np.zeros((P, 15), np.float32), np.zeros(P, np.int32), np.full((P, N), np.nan, np.float32)
    _lib.check(_lib.lib().icon_debug_pair_box(_lib.ptr(corners), C.c_int64(P), _lib.ptr(pts), C.c_int64(N), C.c_int(1 if shared else 0),
                                              _lib.ptr(rec), _lib.ptr(kind), _lib.ptr(bound)), "icon_debug_pair_box")
    return rec, kind, bound

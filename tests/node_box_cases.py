"""Meshes and helpers shared by tests/test_node_box.py (host) and tests/test_gpu_node_box.py: the meshes of tests/pair_box_cases.py plus
small strips of 1, 2, 16, 17 and 33 triangles (the root is a leaf; the root is an oriented parent; one child just over the
threshold; `strip<n>` names a strip of any other length), the model of the walk (tools/node_box_model.py) and the host entries of the rule."""
import ctypes as C
import importlib.util
import os
import sys
from functools import lru_cache

import numpy as np

from common import ROOT, synth
from pair_box_cases import mesh as _pair_mesh

K_MAX_TRIS = 16                 # mesh_rules.h: kNodeBoxMaxTris
K_FLAG = 1 << 30                # mesh_rules.h: kNodeBoxFlag
STRIPS = {"strip1": 1, "strip2": 2, "strip16": 16, "strip17": 17, "strip33": 33}


def _load_model():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    spec = importlib.util.spec_from_file_location("node_box_model", os.path.join(tools, "node_box_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


model = _load_model()


@lru_cache(maxsize=None)
def mesh(name):
    """(verts f32 [V,3], faces i64 [F,3], cmap f32 [V,3], vis f32 [V])"""
    if not name.startswith("strip"):
        return _pair_mesh(name)
    n = STRIPS[name] if name in STRIPS else int(name[5:])      # ("strip<n>": any length; STRIPS: the ones every mesh test runs)
    # a triangle strip wound round a helix: slanted, curved, no two triangles coplanar
    j = np.arange(n + 2)
    ang = 0.35 * j
    r = np.where(j % 2 == 0, 0.45, 0.55)
    v = np.stack([r * np.cos(ang), -0.6 + 1.2 * j / (n + 1) + 0.04 * (j % 2), r * np.sin(ang)], 1)
    f = np.stack([j[:n], j[:n] + 1, j[:n] + 2], 1)
    v, f = np.asarray(v, np.float32), np.asarray(f, np.int64)
    vs, cm = synth.make_vis_cmap(v, f)
    cm, vs = np.asarray(cm, np.float32).reshape(-1, 3), np.asarray(vs, np.float32).reshape(-1)
    return (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int64), np.ascontiguousarray(cm, np.float32),
            np.ascontiguousarray(vs, np.float32))


def box_bound(recs, pts, shared):
    """recs [R,16,2] f32 (PairBox-shaped records); pts [N,3] (shared) or [R,N,3] -> bound [R,2,N] f32: pair_box_bound, the function the
    walk evaluates, both packed components"""
    from icon_amd import _lib
    recs = np.ascontiguousarray(recs, np.float32); pts = np.ascontiguousarray(pts, np.float32)
    R = len(recs)
    N = pts.shape[0] if shared else pts.shape[1]
    assert recs.shape == (R, 16, 2) and pts.shape == ((N, 3) if shared else (R, N, 3))
    bound = np.full((R, 2, N), np.nan, np.float32)
    _lib.check(_lib.lib().icon_debug_box_bound(_lib.ptr(recs), C.c_int64(R), _lib.ptr(pts), C.c_int64(N), C.c_int(1 if shared else 0),
                                               _lib.ptr(bound)), "icon_debug_box_bound")
    return bound


def range_box(tris):
    """tris [n,3,3] f32 -> (rec [15] f32, kind): range_box_setup"""
    from icon_amd import _lib
    tris = np.ascontiguousarray(tris, np.float32)
    rec, kind = np.zeros(15, np.float32), C.c_int32(0)
    _lib.check(_lib.lib().icon_debug_range_box(_lib.ptr(tris), C.c_int64(len(tris)), _lib.ptr(rec), C.byref(kind)), "icon_debug_range_box")
    return rec, kind.value

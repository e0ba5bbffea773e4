"""The reference's own skinning, run from where it lies (tests/test_smpl.py, tools/make_smpl_golden.py) - only where the reference
tree is present.  ``lib/smplx`` is loaded by file path under a stand-in package name, so ``lib/__init__`` and its third-party
imports never run; nothing is copied."""
import importlib
import os
import sys
import types

import numpy as np
import torch

import smpl_oracle as so
from oracle import ref_loader

PACKAGE = "icon_ref_smplx"


def available() -> bool:
    return os.path.isfile(os.path.join(ref_loader.REFERENCE_ROOT, "lib", "smplx", "lbs.py"))


def load(name: str):
    """module ``name`` (``lbs``, ``body_models``, ``utils``) of the reference's ``lib/smplx``"""
    sys.dont_write_bytecode = True                                         # never drop __pycache__ into the reference tree
    if PACKAGE not in sys.modules:
        pkg = types.ModuleType(PACKAGE)
        pkg.__path__ = [os.path.join(ref_loader.REFERENCE_ROOT, "lib", "smplx")]
        sys.modules[PACKAGE] = pkg
    return importlib.import_module(f"{PACKAGE}.{name}")


def run(name, B=1, seed=0, identity=False):
    """``smpl_oracle.run`` in float64 with the reference's ``lbs(..., pose2rot=False)`` in place of the oracle's"""
    lbs = load("lbs").lbs
    m = so.model(name, torch.float64)
    betas, rot, gv, gj = (torch.from_numpy(a).double() for a in so.inputs(name, B, seed, identity))
    out = {}
    for loss in so.LOSSES:
        b, r = betas.clone().requires_grad_(True), rot.clone().requires_grad_(True)
        verts, joints = lbs(b, r, m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["lbs_weights"],
                            pose2rot=False)
        total = ((verts * gv).sum() if loss != "joints" else 0) + ((joints * gj).sum() if loss != "verts" else 0)
        gb, gr = torch.autograd.grad(total, (b, r), allow_unused=True)
        gb, gr = (torch.zeros_like(x) if g is None else g for g, x in ((gb, b), (gr, r)))
        out[loss] = dict(verts=verts.detach().numpy(), joints=joints.detach().numpy(), grad_betas=gb.numpy(), grad_rot=gr.numpy())
    return out


def smpl_module(name, batch_size=1, create_transl=False):
    """the reference's ``SMPL`` class built from a case's arrays through ``data_struct`` - no model file"""
    bm, c = load("body_models"), so.case(name)
    V, J, NB, _ = so.CASES[name]
    struct = load("utils").Struct(
        shapedirs=c["shapedirs"], v_template=c["v_template"].copy(), J_regressor=c["J_regressor"], weights=c["lbs_weights"],
        posedirs=np.ascontiguousarray(c["posedirs"].T).reshape(V, 3, 9 * (J - 1)), f=np.zeros((1, 3), dtype=np.int64),
        kintree_table=np.stack([np.maximum(c["parents"], 0), np.arange(J)]))
    return bm.SMPL("", data_struct=struct, num_betas=NB, batch_size=batch_size, create_transl=create_transl)

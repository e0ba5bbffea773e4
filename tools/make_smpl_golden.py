"""Writes tests/golden/smpl_lbs_ref.npz: the reference's own lbs(..., pose2rot=False) in float64 (lib/smplx/lbs.py, loaded from
where it lies by tests/smpl_reference.py) on two seeded cases of tests/smpl_oracle.py - outputs and autograd gradients for the
three losses.  Data only; this is how the pin to the reference travels to machines without the reference tree
(tests/test_smpl.py::test_oracle_equals_the_stored_reference_run)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import smpl_oracle as so  # noqa: E402
import smpl_reference as sr  # noqa: E402

STORED = (("chain3", 1), ("tree", 2))


def main() -> None:
    out = {}
    for name, B in STORED:
        ref = sr.run(name, B)
        out[f"{name}.B{B}.verts"], out[f"{name}.B{B}.joints"] = ref["both"]["verts"], ref["both"]["joints"]
        for loss in so.LOSSES:
            for k in ("grad_betas", "grad_rot"):
                out[f"{name}.B{B}.{loss}.{k}"] = ref[loss][k]
    path = os.path.join(ROOT, "tests", "golden", "smpl_lbs_ref.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()

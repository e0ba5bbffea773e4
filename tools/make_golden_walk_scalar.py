#!/usr/bin/env python3
"""The results tests/test_gpu_walk_scalar.py pins, computed by the library of the tree this file lies in.

    python tools/make_golden_walk_scalar.py [out.npz]      (on the GPU; default tests/golden/walk_scalar_parent.npz)

Run at the commit BEFORE a change to the loop of the packet walk (geom_device.h: nearest_packet): such a change moves instructions
and addresses, never a bit of a result or a visit.  The cases are tests/walk_scalar_cases.py's, which the test calls as well, so the
two cannot drift apart.  The file holds names, SHA-256 digests and counters only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from icon_amd import _lib  # noqa: E402
import walk_scalar_cases as cases  # noqa: E402

if __name__ == "__main__":
    _lib.require_device()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "walk_scalar_parent.npz")
    got = cases.record_all()
    names = sorted(got)
    np.savez_compressed(path, names=np.array(names), values=np.array([str(got[k]) for k in names]))
    for k in names:
        print(k, got[k])
    print(f"{path}: {len(names)} entries, {os.path.getsize(path)} bytes")

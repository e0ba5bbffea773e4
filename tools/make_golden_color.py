#!/usr/bin/env python3
"""tests/golden/query_color_ref.npz: the reference's OWN query_color (lib/common/render.py:60-84, run verbatim from its file
by tests/color_checker.py:reference_query_color, third-party leaves bound to the oracle) on the 6,890-vertex synthetic body and
the level-3 icosphere, with a seeded 64 x 64 image.  Inputs are regenerated from icon_amd.synth by the tests; the file holds
the image, the expected colours and the visibility only.  Needs the reference tree (build container).

    python tools/make_golden_color.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import color_checker as cc  # noqa: E402
from common import orc  # noqa: E402


def main():
    ref = cc.reference_query_color()
    image = cc.make_image()
    out = {"image": image.numpy()}
    for name in ("body", "ico"):
        v, f = cc.MESHES[name]()
        colors = ref(torch.from_numpy(v), torch.from_numpy(f), image, "cpu").numpy()
        vis = orc.visibility(v[:, :2], v[:, 2], f[:, [0, 2, 1]], 4096)[:, 0]
        out[f"{name}_colors"] = colors.astype(np.float32)
        out[f"{name}_vis"] = vis.astype(np.uint8)
        print(f"{name}: {len(v)} vertices, {100 * vis.mean():.1f} % visible, colours {colors.min():.2f} .. {colors.max():.2f}")
    path = os.path.join(ROOT, "tests", "golden", "query_color_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Records tests/golden/extract_cloth_ref.npz and tests/golden/smpl_part_labels.npz: the reference's own extract_cloth
(lib/common/cloth_extraction.py, loaded from the reference tree behind the stand-in trimesh container of tests/test_garment.py),
run verbatim on test_garment.golden_case() for the garment types test_garment.GOLDEN_TYPES with the matrices of
apps/infer.py:576-585, and the reference's part table as 24 names and one int8 label per SMPL vertex.

    ICON_REFERENCE_ROOT=/path/to/ICON python tests/make_garment_golden.py

Needs the reference tree, matplotlib and scikit-learn; the tests that read the fixtures need none of them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import test_garment as tg  # noqa: E402


def main():
    ref, table = tg.load_reference(), tg.reference_part_table()
    assert ref is not None and table is not None, "the reference tree, matplotlib and scikit-learn are needed"
    case = tg.golden_case()
    out = dict(verts=case["verts"], faces=case["faces"])
    for k, c in enumerate(case["coords"]):
        out[f"coords_{k}"] = c
    for type_id in tg.GOLDEN_TYPES:
        mesh = ref.extract_cloth(tg._Mesh(case["verts"], case["faces"]), dict(coord_normalized=case["coords"], type_id=type_id),
                                 tg.K_INFER, tg.R_INFER, tg.T_INFER, tg._Mesh(case["body"], case["body_faces"]))
        out[f"out_verts_{type_id}"] = np.asarray(mesh.vertices, dtype=np.float32)
        out[f"out_faces_{type_id}"] = np.asarray(mesh.faces, dtype=np.int32)
        print(f"type_id {type_id}: {len(mesh.vertices)} vertices, {len(mesh.faces)} faces of {len(case['verts'])} / {len(case['faces'])}")
    np.savez_compressed(os.path.join(tg.ROOT, "tests", "golden", "extract_cloth_ref.npz"), **out)
    names, labels = tg.reference_labels(ref)                                      # through the reference's own smpl_to_recon_labels
    assert names == list(table.keys())
    np.savez_compressed(os.path.join(tg.ROOT, "tests", "golden", "smpl_part_labels.npz"), names=np.array(names), labels=labels)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Records tests/golden/sampling_geo_ref.npz: the reference's own PIFuDataset.get_sampling_geo (lib/dataset/PIFuDataset.py:483-607,
loaded from the reference tree behind the stand-ins of tests/test_sampling.py), run verbatim for test_sampling.CASES after
``np.random.seed(s)``, with a ``mesh`` that has ``verts``, ``vert_normals`` and ``contains`` = oracle.check_sign - and numpy's own
draws of that run in the reference's order, taken again after re-seeding: the vertex ids, the unused choice without replacement,
the offsets, the space points, the z noise, and the shuffle as the permutation of an [n,1] column of indices.

    ICON_REFERENCE_ROOT=/path/to/ICON python tests/make_sampling_golden.py

Needs the reference tree; the tests that read the fixture do not."""
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import test_sampling as ts  # noqa: E402


class Mesh:
    def __init__(self, name):
        v, f, vn = ts.scan(name)
        self.verts, self.vert_normals = v.astype(np.float64), vn.astype(np.float64)
        self._inside, self.flags = ts.inside_fn(name), None

    def contains(self, samples):
        self.flags = self._inside(samples.astype(np.float32))
        return self.flags


def numpy_draws(seed, V, N, sigma, Z, R):
    """the calls of PIFuDataset.py:495-547 that consume numpy's global stream, in their order"""
    np.random.seed(seed)
    p = np.ones(V, dtype=np.float32)
    p /= p.sum()
    ids = np.random.choice(np.arange(V), 4 * N, replace=True, p=p)
    np.random.choice(np.arange(V), N // 2, replace=False, p=p)
    offsets = np.random.normal(scale=sigma, size=(4 * N, 1))
    u = np.random.rand(N // 4, 3)
    znoise = np.random.normal(scale=0.40, size=(4 * N * R,)) if Z else np.zeros(0)
    n = 4 * N + N // 4 + len(znoise)
    state = np.random.get_state()
    column = np.arange(n).reshape(n, 1)
    np.random.shuffle(column)
    np.random.set_state(state)                                         # the [n,3] rows take the same path: checked here
    rows = np.repeat(np.arange(n, dtype=np.float64).reshape(n, 1), 3, axis=1)
    np.random.shuffle(rows)
    assert np.array_equal(rows[:, 0], column[:, 0]) and np.array_equal(rows[:, 2], column[:, 0])
    return dict(ids=ids.astype(np.int32), offsets=offsets[:, 0], u=u, znoise=znoise, perm=column[:, 0].astype(np.int32))


def main():
    ref = ts.load_reference()
    assert ref is not None, "the reference tree is needed"
    out = {}
    for case, (name, N, sigma, zray, R, is_valid, seed) in ts.CASES.items():
        mesh = Mesh(name)
        me = SimpleNamespace(opt=SimpleNamespace(num_sample_geo=N, sigma_geo=sigma, zray_type=zray, ray_sample_num=R))
        np.random.seed(seed)
        res = ref(me, dict(mesh=mesh, calib=ts.CALIB.copy()), is_valid=is_valid, is_sdf=False)
        rec = numpy_draws(seed, len(mesh.verts), N, sigma, zray and not is_valid, R)
        rec.update(samples=res["samples_geo"].numpy(), labels=res["labels_geo"].numpy(), inside_all=np.asarray(mesh.flags, dtype=np.uint8))
        assert len(rec["inside_all"]) == len(rec["perm"])
        out.update({f"{case}.{k}": v for k, v in rec.items()})
        print(f"{case}: n = {len(rec['perm'])}, {int(rec['inside_all'].sum())} inside -> {int(rec['labels'].sum())} + "
              f"{int((rec['labels'] == 0).sum())} rows")
    path = os.path.join(HERE, "golden", "sampling_geo_ref.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()

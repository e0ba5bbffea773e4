"""Different kinds of query call one after another on ONE workspace (icon prior, reference cmap mode).

Every kind - a lattice slab, a point call with the cooperative and with the packet search, the batched call, the coarse-to-fine
schedule, the split slab pair finished in two pieces, the training rows - describes itself in a call record that the native
entry point fills; whatever the workspace keeps between calls (its scratch, the byte of higher slot bits of big meshes, the slab
prepared by slab_features) must not leak from one kind into the next.  The yardstick needs no tolerance: every result must equal,
bit for bit, the same call on a fresh engine."""
import os
import sys
import types
from functools import lru_cache

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_subjects as bs  # noqa: E402
import test_gpu_batch_oracle as tbo  # noqa: E402
from icon_amd import training  # noqa: E402
from icon_amd._lib import IconAmdError  # noqa: E402

pytestmark = pytest.mark.gpu
T, DEV, MESH_KEYS, PACKET_MIN = tbo.T, tbo.DEV, tbo.MESH_KEYS, tbo.PACKET_MIN
N_COOP, N_PACKET = 300, PACKET_MIN + 37
SCHEDULE = [17, 33, 65]
assert N_PACKET == 98341 and N_PACKET % 64 != 0


def one_subject(S, b=0):
    return {k: S[k][b:b + 1] for k in MESH_KEYS + ("calibs",)}


class Bound:
    """device tensors of a set of subjects, made once: binding the same tensors again keeps the engine's mesh handles"""

    def __init__(self, S):
        B = S["smpl_verts"].shape[0]
        self.S, self.B = S, B
        self.mesh = tuple(T(S[k]) for k in MESH_KEYS)
        self.calibs = T(S["calibs"])
        self.feat = T(tbo.planes(2)[:B])

    @lru_cache(maxsize=None)
    def points(self, n, seed):
        return T(bs.candidate_points(self.S, n, seed).transpose(0, 2, 1))

    def query(self, eng, n, seed=3):
        eng.set_mesh(*self.mesh)
        return eng.query([self.feat], self.points(n, seed), self.calibs)[0]


@lru_cache(maxsize=None)
def small():
    S = bs.subjects(2)
    return Bound(one_subject(S)), Bound(S)


@lru_cache(maxsize=None)
def big():
    S = tbo.big_subjects()
    return Bound(one_subject(S)), Bound(S)


@lru_cache(maxsize=None)
def train_regressor():
    torch.manual_seed(5)
    return torch.nn.Conv1d(13, 1, 1).to(DEV).train()


def fresh_engine():
    return tbo.engine(small()[1].S, np.zeros(0, np.float32))[0]


# ---- the kinds of call: eng -> tuple of tensors --------------------------------------------------------------------------------
def call_eval_slab(eng, one=None):
    one = one or small()[0]
    eng.set_mesh(*one.mesh)
    return (eng.eval_slab(one.feat, 33, 0, 33),)


def call_query_coop(eng):
    return (small()[0].query(eng, N_COOP),)


def call_query_packet(eng):
    return (small()[0].query(eng, N_PACKET),)


def call_batch(eng):
    return (small()[1].query(eng, 3000),)


def call_adaptive(eng, one=None):
    one = one or small()[0]
    eng.set_mesh(*one.mesh)
    vol, counts, any_pos = eng.adaptive_eval(one.feat, SCHEDULE)
    print(f"adaptive_eval({SCHEDULE}): points queried per level {counts}, any above 0.5 on the coarsest level: {any_pos}")
    assert counts[0] == 17 ** 3 and 0 < counts[1] < 33 ** 3, "the queried level must hold points (a subset of its lattice)"
    return vol, torch.tensor(counts + [int(any_pos)])


def call_split_slab(eng):
    one = small()[0]
    eng.set_mesh(*one.mesh)
    # (msg=: the slab's sign list stays in the workspace, where a finish without an exchange looks for it; with a caller's `signs`
    #  buffer the list goes there and the exchange is the caller's - slab_finish)
    eng.slab_features(one.feat, 33, 0, 33, msg=torch.zeros(8 + (33 ** 3 + 3) // 4, dtype=torch.uint8, device=DEV))
    out = torch.full((33, 33, 33), float("nan"), device=DEV)
    eng.slab_finish_gathered(33, 0, 33, None, 0, 1, 0, out=out, za=0, zb=16)
    eng.slab_finish_gathered(33, 0, 33, None, 0, 1, 0, out=out, za=16, zb=33)
    return (out,)


def call_train_rows(eng):
    two = small()[1]
    eng.set_mesh(*two.mesh)
    out = training.TrainQuery(types.SimpleNamespace(), eng)([two.feat], two.points(500, 9), two.calibs, regressor=train_regressor())
    assert len(out) == 1 and tuple(out[0].shape) == (2, 1, 500)
    return (out[0].detach(),)


def in_f32(call):
    def run(eng):
        eng.precision = "f32"
        try:
            return call(eng)
        finally:
            eng.precision = "f16x3"
    run.__name__ = call.__name__ + "_f32"
    return run


KINDS = [call_eval_slab, call_query_coop, call_query_packet, call_batch, call_adaptive, call_split_slab, call_train_rows]
F32 = [in_f32(call_query_coop), in_f32(call_batch)]


@lru_cache(maxsize=None)
def on_fresh_engine(call):
    return tuple(t.clone() for t in call(fresh_engine()))


def assert_same(got, want, what):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert torch.isfinite(w.float()).all(), what
        assert torch.equal(g.to(w.device), w), f"{what}: differs from the same call on a fresh engine in {(g.to(w.device) != w).sum().item()} of {w.numel()} values"


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_every_kind_of_call_after_every_other_on_one_workspace(order):
    calls = KINDS + F32
    want = [on_fresh_engine(c) for c in calls]
    if order == "reverse":
        calls, want = calls[::-1], want[::-1]
    eng = fresh_engine()
    for c, w in zip(calls, want):
        assert_same(c(eng), w, f"{c.__name__} ({order} order)")
    assert eng.work is not None and not getattr(eng, "_extra_works", None), "every call ran on the engine's one workspace"


# ---- the byte of higher slot bits (meshes beyond 32,768 triangle slots) ----------------------------------------------------------
def big_third_single(eng):
    return (big()[0].query(eng, 50000, 6),)


def big_third_batch(eng):
    return (big()[1].query(eng, 50000, 6),)


def big_third_adaptive(eng):
    return call_adaptive(eng, big()[0])


@pytest.mark.parametrize("variant", ["single", "batch", "adaptive"])
def test_high_slot_byte_follows_the_point_arrays(variant):
    """a big-mesh call sizes the byte of higher slot bits for 3,000 points; a small-mesh call (which has no such byte) grows the
    point arrays; the next big-mesh call needs the byte for all of its points"""
    b = 1 if variant == "batch" else 0
    tbo.assert_high_slots_reached(big()[1].S, bs.candidate_points(big()[1].S, 3000, 4))
    first = lambda eng: (big()[b].query(eng, 3000, 4),)                                         # noqa: E731
    grow = lambda eng: (small()[b].query(eng, N_PACKET),)                                       # noqa: E731
    third = dict(single=big_third_single, batch=big_third_batch, adaptive=big_third_adaptive)[variant]
    eng = fresh_engine()
    for step, call in (("first", first), ("grow", grow), ("third", third)):
        assert_same(call(eng), call(fresh_engine()), f"{variant}: {step} call")


# ---- the split slab protocol's state ---------------------------------------------------------------------------------------------
def finish_calls(eng, signs):
    yield "slab_finish", lambda: eng.slab_finish(33, 0, 33, signs, 0, 0, device=DEV)
    yield "slab_finish_gathered", lambda: eng.slab_finish_gathered(33, 0, 33, None, 0, 1, 0, device=DEV)


def test_finish_without_features_is_refused():
    eng = fresh_engine()
    eng.set_mesh(*small()[0].mesh)
    for name, finish in finish_calls(eng, torch.zeros(33 ** 3, dtype=torch.int8, device=DEV)):
        with pytest.raises(IconAmdError, match="no matching icon_grid_slab_features"):
            finish()


@pytest.mark.parametrize("between", [call_query_coop, call_batch, call_adaptive, call_train_rows], ids=lambda c: c.__name__)
def test_any_other_call_between_features_and_finish_invalidates_the_slab(between):
    one = small()[0]
    for which in (0, 1):
        eng = fresh_engine()
        eng.set_mesh(*one.mesh)
        signs, _ = eng.slab_features(one.feat, 33, 0, 33)
        assert_same(between(eng), on_fresh_engine(between), between.__name__)
        eng.set_mesh(*one.mesh)
        name, finish = list(finish_calls(eng, signs))[which]
        with pytest.raises(IconAmdError, match="no matching icon_grid_slab_features"):
            finish()
        assert_same(call_split_slab(eng), on_fresh_engine(call_split_slab), f"the split pair after the refused {name}")

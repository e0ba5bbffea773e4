"""icon_amd._native without a device: the refusal, the faces as the native calls read them, and - one table - the scratch checks
of the C entries (common.h: scratch_check) that no other host test reaches.  SCRATCH_ROWS is shared with
tests/test_gpu_native_call.py, which runs the rows that need a device."""
import ctypes as C

import pytest
import torch

from icon_amd import _lib, _native
from icon_amd._lib import IconAmdError

P = C.c_void_p(4096)                # a non-null pointer that is never dereferenced: every row is refused before a launch
Z = C.c_void_p(0)
i32, i64 = C.c_int, C.c_int64


def test_need_device_refuses_with_the_unchanged_text(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # "where no device is visible": here, and forced on a GPU host
    with pytest.raises(IconAmdError) as e:
        _native.need_device("render_normal_device")
    assert str(e.value) == "render_normal_device needs the HIP device (there is no CPU fallback)"


def test_need_device_passes_where_a_device_is_visible(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    assert _native.need_device("anything") is None


def test_faces_arg_on_cpu_tensors():
    base = torch.tensor([[0, 1, 2], [2, 1, 3]])
    f, flag = _native.faces_arg(base.to(torch.int32))
    assert f.dtype == torch.int32 and flag.value == 0 and f.is_contiguous() and torch.equal(f, base.int())
    f, flag = _native.faces_arg(base.to(torch.int64))
    assert f.dtype == torch.int64 and flag.value == 1 and f.data_ptr() == base.data_ptr()       # read in place
    for narrow in (torch.int16, torch.uint8, torch.int8):
        f, flag = _native.faces_arg(base.to(narrow))
        assert f.dtype == torch.int64 and flag.value == 1 and torch.equal(f, base)
    wide = torch.arange(24, dtype=torch.int32).reshape(4, 6)
    view = wide[:, ::2]                                                   # [4,3], strides (6, 2)
    assert not view.is_contiguous()
    f, flag = _native.faces_arg(view)
    assert f.is_contiguous() and f.dtype == torch.int32 and flag.value == 0 and torch.equal(f, view)
    assert isinstance(flag, C.c_int)


def test_faces_arg_shares_no_autograd_history():
    leaf = torch.tensor([[0.0, 1.0, 2.0]], requires_grad=True)
    tracked = (leaf * 1.0).to(torch.int64)                                # an integer tensor cannot require grad; a float one can
    for t in (tracked, leaf * 2.0):
        f, _ = _native.faces_arg(t)
        assert not f.requires_grad and f.grad_fn is None


# ---- the scratch checks of the C entries, one table ----------------------------------------------------------------------------
# (entry, its *_bytes entry, that entry's size arguments, call(lib, scratch, nbytes, scan) -> code, needs a device)
def _smpl_backward(L, scratch, nbytes, scan):
    from icon_amd.smpl import _Tables
    V, J, NB, K = 100, 4, 3, 2
    t = _Tables(*([4096] * 8), V, J, NB, K, 9 * (J - 1))
    return L.icon_smpl_backward(C.byref(t), P, P, i64(2), P, P, P, P, P, scratch, i64(nbytes), Z)


def _extract_cloth(L, scratch, nbytes, scan):
    hc = (C.c_int64 * 2)()
    return L.icon_extract_cloth(P, i64(12), P, i64(20), i32(1), P, P, i64(5), i64(1), Z, i64(0), Z, P, P, P, hc, scratch, i64(nbytes), Z)


def _sample_geo(L, scratch, nbytes, scan):
    cal = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    return L.icon_sample_geo(scan, P, P, cal, cal, i64(16), C.c_double(5.0), i32(0), i32(1), C.c_uint64(7), P, P, P, Z, Z, Z, Z,
                             scratch, i64(nbytes), Z)


def _train_rows_backward(L, scratch, nbytes, scan):
    return L.icon_train_rows_backward(P, P, i32(2), C.c_uint32(3), i32(2), i32(7), i32(6), i32(8), i32(8), i32(1), i64(100), P,
                                      scratch, i64(nbytes), Z)


def _render_turntable(L, scratch, nbytes, scan):
    return L.icon_render_turntable(P, i64(12), P, i64(20), i32(1), P, i32(5), i32(32), P, i64(32), i64(0), Z, Z, Z, scratch, i64(nbytes), Z)


def _render_normal(L, scratch, nbytes, scan):
    return L.icon_render_normal(P, i64(12), P, i64(20), i32(1), (C.c_int * 2)(0, 2), i32(2), i32(32), P, Z, Z, scratch, i64(nbytes), Z)


def _query_color(L, scratch, nbytes, scan):
    return L.icon_query_color(P, i64(12), P, i64(20), i32(1), P, i32(16), i32(16), i32(64), P, Z, scratch, i64(nbytes), Z)


SCRATCH_ROWS = [
    ("icon_smpl_backward", "icon_smpl_bytes", (i64(2), i64(100), i32(4), i32(3), i32(2)), _smpl_backward, False),
    ("icon_extract_cloth", "icon_extract_cloth_bytes", (i64(12), i64(20), i64(5), i64(1)), _extract_cloth, False),
    ("icon_sample_geo", "icon_sample_geo_bytes", (i64(4 * 16 + 16 // 4),), _sample_geo, True),      # reads the scan's handle on the host
    ("icon_train_rows_backward", "icon_train_rows_bytes", (i32(2), i64(100), i32(2), i32(6), i32(8), i32(8)), _train_rows_backward, False),
    ("icon_render_turntable", "icon_render_turntable_bytes", (i64(12), i64(20), i32(32), i32(5)), _render_turntable, False),
    ("icon_render_normal", "icon_render_bytes", (i64(12), i64(20), i32(32), i32(2)), _render_normal, False),
    ("icon_query_color", "icon_query_color_bytes", (i64(12), i64(20), i32(64)), _query_color, False),
]


def check_scratch_row(row, scan=None):
    """a scratch at address 260 -> code 1, "256-byte aligned"; an aligned one a byte short -> "scratch smaller than <bytes entry>" """
    entry, bytes_entry, size_args, call, _ = row
    L = _lib.lib()
    n = C.c_int64(0)
    assert getattr(L, bytes_entry)(*size_args, C.byref(n)) == 0, L.icon_last_error()
    assert n.value > 0 and n.value % 256 == 0
    assert call(L, C.c_void_p(260), n.value, scan) == 1
    assert L.icon_last_error() == f"{entry}: the scratch must be 256-byte aligned".encode()
    assert call(L, C.c_void_p(8192), n.value - 1, scan) == 1
    assert L.icon_last_error() == f"{entry}: scratch smaller than {bytes_entry}".encode()


@pytest.mark.parametrize("row", [r for r in SCRATCH_ROWS if not r[4]], ids=lambda r: r[0])
def test_scratch_checks_of_the_entries_without_a_device(row):
    check_scratch_row(row)


def test_scratch_for_names_the_entry_it_asked(monkeypatch):
    """a refused size query surfaces under the *_bytes entry's own name, before any allocation"""
    monkeypatch.setattr(_native, "scratch", lambda device, nbytes: pytest.fail("allocated for a refused query"))
    with pytest.raises(IconAmdError, match=r"^icon_render_bytes failed \(code 1\): icon_render_normal: size must be 8\.\.2048"):
        _native.scratch_for(torch.device("cuda", 0), "icon_render_bytes", i64(12), i64(20), i32(4), i32(2))

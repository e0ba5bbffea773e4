"""How the Python modules call the native library: the stream a call is enqueued on, the refusal without a device, the scratch
a call is handed and how it is sized, the small constants a call reads, the faces as the calls read them.

Imports only ``torch``, ``ctypes`` and ``._lib``, so every other module imports it at the top of the file.
"""
from __future__ import annotations

import ctypes as C
import threading

import torch

from . import _lib
from ._lib import IconAmdError, check

_tls = threading.local()


def stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def need_device(what: str) -> None:
    if not torch.cuda.is_available():
        raise IconAmdError(f"{what} needs the HIP device (there is no CPU fallback)")


def _slot(name: str, device: torch.device):
    """this thread's dict ``name`` and the part of a key that says where a call runs: (device index, current stream)"""
    store = getattr(_tls, name, None)
    if store is None:
        store = {}
        setattr(_tls, name, store)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return store, idx, (idx, torch.cuda.current_stream(idx).cuda_stream)


def scratch(device: torch.device, nbytes: int) -> torch.Tensor:
    """the scratch of a native call: one uint8 tensor per (thread, device, stream), grown on demand and reused by every call
    of every family.  Per stream, because two calls on different streams may run at once and must not share a z-buffer; and
    because torch's allocator orders the reuse of a freed block only against the stream it was allocated on - which, keyed
    like this, is the stream that used it.  Per thread: a backward call runs on autograd's device thread and so has its own.
    A call finds whatever the previous user - of any family - left: it clears what it reads before it reads it."""
    pool, idx, key = _slot("pool", device)
    buf = pool.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = pool[key] = torch.empty(nbytes, dtype=torch.uint8, device=torch.device("cuda", idx))
    return buf


def scratch_for(device: torch.device, bytes_entry: str, *size_args) -> torch.Tensor:
    """the scratch of the call that the library's ``bytes_entry`` sizes, given that entry's arguments (ctypes values).  The
    entry is named because the names do not pair up: ``icon_render_bytes`` sizes ``icon_render_normal``."""
    n = C.c_int64(0)
    check(getattr(_lib.lib(), bytes_entry)(*size_args, C.byref(n)), bytes_entry)
    return scratch(device, n.value)


def constants(device: torch.device, *arrays) -> tuple:
    """small host numpy arrays on the device, one tensor per array, kept per (thread, device, stream) like the scratch and
    keyed by their bytes: a call repeated after a warm-up uploads nothing - so it can be captured into a graph.  Reset
    when it passes 64 entries."""
    cache, idx, where = _slot("consts", device)
    if len(cache) > 64:
        cache.clear()
    key = where + tuple(a.tobytes() for a in arrays)
    if key not in cache:
        cache[key] = tuple(torch.from_numpy(a).to(torch.device("cuda", idx)) for a in arrays)
    return cache[key]


def faces_arg(faces: torch.Tensor):
    """-> the faces as the native calls read them - detached, int32 or int64 (any other integer type widened to int64),
    contiguous - and the flag that tells the call which: ``c_int(1)`` for int64"""
    f = faces.detach()
    if f.dtype not in (torch.int32, torch.int64):
        f = f.to(torch.int64)
    return f.contiguous(), C.c_int(1 if f.dtype == torch.int64 else 0)

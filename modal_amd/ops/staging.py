"""Pinned-buffer host<->device staging on a side HIP stream.

BASELINE's blob-plane obligation: Volume/blob payloads ride pinned
hipMemcpyAsync on a dedicated stream instead of pageable copies on the
default stream (pageable H2D is roughly half pinned bandwidth and
serializes with compute). One process-wide pinned arena is reused and
guarded by a lock; callers get an ordinary device tensor synchronized
with the caller's current stream. ``copy_to_device``/``copy_from_device``
are the pointer-based twins for memory torch does not own (ops/devcodec.py):
same arena, same lock, the copy on the caller's own stream.
"""

from __future__ import annotations

import threading
from typing import Any

_lock = threading.Lock()
_pin_buf: Any = None  # torch uint8 pinned host tensor
_pin_np: Any = None  # numpy view of _pin_buf
_h2d_stream: Any = None
_d2h_stream: Any = None

_MIN_CAP = 64 * 1024 * 1024
_MAX_PIN = 1 << 30  # larger payloads are not pinned whole
_H2D, _D2H = 1, 2  # ma_malz_copy kinds


def _ensure(n: int) -> None:
    global _pin_buf, _pin_np, _h2d_stream, _d2h_stream
    import torch

    if _pin_buf is None or _pin_buf.numel() < n:
        cap = max(_MIN_CAP, 1 << max(n - 1, 1).bit_length())
        _pin_buf = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
        _pin_np = _pin_buf.numpy()
    if _h2d_stream is None:
        _h2d_stream = torch.cuda.Stream()
        _d2h_stream = torch.cuda.Stream()


def stage_to_gpu(data: Any) -> Any:
    """bytes/bytearray/memoryview -> device uint8 tensor via the pinned
    arena + side-stream hipMemcpyAsync. Falls back to a pageable copy for
    payloads larger than we are willing to pin (1 GiB)."""
    import numpy as np
    import torch

    n = len(data)
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    if n > _MAX_PIN:
        return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    with _lock:
        _ensure(n)
        _pin_np[:n] = np.frombuffer(data, dtype=np.uint8)  # one memcpy to pinned
        dst = torch.empty(n, dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(_h2d_stream):
            dst.copy_(_pin_buf[:n], non_blocking=True)
        # the arena is reused by the next caller: wait for the DMA here,
        # then order the caller's stream after it
        _h2d_stream.synchronize()
    torch.cuda.current_stream().wait_stream(_h2d_stream)
    return dst


def stage_many_to_gpu(buffers: list, align: int = 1) -> tuple:
    """Stage several host buffers into ONE device tensor with a single
    pinned H2D, each placed at an ``align``-aligned offset (skips the
    intermediate concat bytearray a caller would otherwise build — a
    full extra pass over the payload). Returns (device_tensor, offsets)."""
    import numpy as np
    import torch

    offsets = []
    off = 0
    for data in buffers:
        offsets.append(off)
        off += -(-len(data) // align) * align
    total = off
    if total == 0:
        return torch.empty(0, dtype=torch.uint8, device="cuda"), offsets
    if total > _MAX_PIN:
        big = bytearray(total)
        for data, o in zip(buffers, offsets):
            big[o : o + len(data)] = data
        return torch.frombuffer(big, dtype=torch.uint8).cuda(), offsets
    with _lock:
        _ensure(total)
        for data, o in zip(buffers, offsets):
            _pin_np[o : o + len(data)] = np.frombuffer(data, dtype=np.uint8)
        dst = torch.empty(total, dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(_h2d_stream):
            dst.copy_(_pin_buf[:total], non_blocking=True)
        _h2d_stream.synchronize()
    torch.cuda.current_stream().wait_stream(_h2d_stream)
    return dst, offsets


def fetch_from_gpu(tensor: Any) -> bytes:
    """Device uint8 tensor -> bytes via the pinned arena + side stream."""
    import torch

    n = tensor.numel()
    if n == 0:
        return b""
    if n > _MAX_PIN:
        return tensor.cpu().numpy().tobytes()
    with _lock:
        _ensure(n)
        with torch.cuda.stream(_d2h_stream):
            _d2h_stream.wait_stream(torch.cuda.current_stream())
            _pin_buf[:n].copy_(tensor, non_blocking=True)
        _d2h_stream.synchronize()
        return _pin_np[:n].tobytes()


def _copy(dst: int, src: int, n: int, kind: int) -> None:
    """ma_malz_copy on the caller's stream, then wait for it."""
    import torch

    from . import load_lib

    stream = torch.cuda.current_stream()
    rc = load_lib(required=True).ma_malz_copy(dst, src, n, kind, stream.cuda_stream)
    if rc != 0:
        raise RuntimeError(f"staging copy failed: hipError {rc}")
    stream.synchronize()  # the arena is reused by the next caller


def copy_to_device(dev_ptr: int, parts: Any) -> None:
    """Host buffers, concatenated -> device memory at ``dev_ptr``, through
    the pinned arena on the caller's stream."""
    import numpy as np

    total = sum(len(p) for p in parts)
    if total == 0:
        return
    with _lock:
        _ensure(total)
        pos = 0
        for p in parts:
            _pin_np[pos : pos + len(p)] = np.frombuffer(p, dtype=np.uint8)
            pos += len(p)
        _copy(dev_ptr, _pin_buf.data_ptr(), total, _H2D)


def copy_from_device(dev_ptr: int, n: int) -> bytes:
    """``n`` bytes of device memory at ``dev_ptr`` -> bytes, through the
    pinned arena on the caller's stream, at most _MAX_PIN at a time."""
    chunks = []
    with _lock:
        for pos in range(0, n, _MAX_PIN):
            m = min(_MAX_PIN, n - pos)
            _ensure(m)
            _copy(_pin_buf.data_ptr(), dev_ptr + pos, m, _D2H)
            chunks.append(_pin_np[:m].tobytes())
    return chunks[0] if len(chunks) == 1 else b"".join(chunks)

"""Chunk (de)compression: container format over the HIP LZ4 kernels.

Container layout (little-endian):
  magic  b"MALZ41"             (6 bytes)
  raw_len  u64
  n_segments  u32              (raw split into 4 KiB segments)
  comp_len[n_segments]  u32    (0 => segment stored raw)
  payload                      (concatenated per-segment LZ4 blocks / raw)

Each segment is a standard LZ4 block, so any LZ4 block decoder can read the
payload; the CPU reference codec (utils/lz4ref.py) serves GPU-less readers.

Everything that touches the format lives here once:

  ``validate_container``   the only parser; bounds all a decoder indexes with
  ``compress_spans_gpu``   the only device encoder: LZ4 kernel per span, then
                           the plan/assemble kernels (csrc/malz.hip) finish
                           the containers in HBM and one dense D2H fetches them
  ``decompress_run_gpu``   the only device decoder launch

``compress_buffer_gpu``/``compress_buffers_gpu`` (blobs) and ops/devcodec.py
(snapshots) are thin callers of these, so their containers are byte-identical
by construction and the CAS dedups between them.
"""

from __future__ import annotations

import struct
from typing import Any, Optional, Sequence

from . import gpu_available, load_lib

MAGIC = b"MALZ41"
HEADER_FIXED = len(MAGIC) + 12  # magic + u64 raw_len + u32 n_seg
SEG_SIZE = 4096
OUT_STRIDE = SEG_SIZE + 256
MIN_GAIN = 0.95  # store raw unless compression saves >=5%
_STATUS_CLEAN = 2**31 - 1  # decompress status word when no segment is corrupt


def _header(raw_len: int, comp_lens: Sequence[int]) -> bytes:
    return (
        MAGIC
        + struct.pack("<QI", raw_len, len(comp_lens))
        + struct.pack(f"<{len(comp_lens)}I", *comp_lens)
    )


def worth_keeping(payload_len: Any, raw_len: Any) -> Any:
    """THE keep/raw rule: a container is kept only when its payload saves
    at least 1 - MIN_GAIN of the raw bytes (scalars or numpy arrays)."""
    return payload_len < raw_len * MIN_GAIN


def effective_lens(comp_lens: Any, raw_len: int) -> Any:
    """Bytes every segment takes in the payload (int64 array): its comp_len,
    or the raw segment length where comp_len is 0."""
    import numpy as np

    comp_lens = np.asarray(comp_lens)
    seg_raw = np.full(len(comp_lens), SEG_SIZE, dtype=np.int64)
    if len(comp_lens):
        seg_raw[-1] = raw_len - (len(comp_lens) - 1) * SEG_SIZE
    return np.where(comp_lens == 0, seg_raw, comp_lens.astype(np.int64))


def validate_container(
    blob: bytes, raw_len: Optional[int] = None, what: str = "container"
) -> tuple[int, Any, int]:
    """Parse a container and bound everything a decoder will index with:
    magic, raw_len against the caller's (when given), n_seg against raw_len,
    every comp_len < SEG_SIZE, header + payload == len(blob). Returns
    (raw_len, comp_lens int32 array, payload offset); raises ValueError
    naming ``what``."""
    import numpy as np

    def bad(why: str) -> ValueError:
        return ValueError(f"{what}: {why}")

    n = len(blob)
    if n < HEADER_FIXED or bytes(blob[: len(MAGIC)]) != MAGIC:
        raise bad("not a MALZ41 container")
    hdr_raw, n_seg = struct.unpack_from("<QI", blob, len(MAGIC))
    if raw_len is not None and hdr_raw != raw_len:
        raise bad(f"container raw_len {hdr_raw} != manifest {raw_len}")
    if n_seg != -(-hdr_raw // SEG_SIZE):
        raise bad(f"container has {n_seg} segments for {hdr_raw} bytes")
    off = HEADER_FIXED + 4 * n_seg
    if n < off:
        raise bad("container truncated inside its segment table")
    comp_lens = np.frombuffer(blob, dtype="<u4", count=n_seg, offset=HEADER_FIXED)
    if n_seg and int(comp_lens.max()) >= SEG_SIZE:
        raise bad("segment comp_len out of range")
    payload = int(effective_lens(comp_lens, hdr_raw).sum())
    if off + payload != n:
        raise bad(f"container is {n} bytes, header says {off + payload}")
    return hdr_raw, comp_lens.astype(np.int32), off


def parse_header(blob: bytes) -> tuple[int, list[int], int]:
    """Returns (raw_len, comp_lens, payload_offset) of a valid container."""
    raw_len, comp_lens, off = validate_container(blob)
    return raw_len, comp_lens.tolist(), off


def is_compressed(blob: bytes) -> bool:
    return blob.startswith(MAGIC)


def _is_float_plane(blob: bytes) -> bool:
    """A stored container is one of ours, MALZ41 or MAFP10 (ops/fpcodec.py):
    whether a blob is compressed at all is out of band (the ``.z`` suffix),
    so the magic only has to tell the two apart."""
    return bytes(blob[:6]) == b"MAFP10"


# ---------------------------------------------------------------------------
# CPU reference paths
# ---------------------------------------------------------------------------


def _native_core() -> Optional[object]:
    try:
        from .. import _core

        return _core if hasattr(_core, "malz_compress") else None
    except ImportError:
        return None


def compress_buffer_cpu(data: bytes) -> Optional[bytes]:
    core = _native_core()
    if core is not None:
        # C++ segment-parallel codec (csrc/core.cpp): same container, same
        # compress/raw decisions, ~1000x the pure-Python reference
        return core.malz_compress(bytes(data), MIN_GAIN)
    from ..utils import lz4ref

    n = len(data)
    comp_lens: list[int] = []
    payload = bytearray()
    for start in range(0, n, SEG_SIZE):
        seg = data[start : start + SEG_SIZE]
        comp = lz4ref.compress_block(seg)
        if len(comp) < len(seg):
            comp_lens.append(len(comp))
            payload += comp
        else:
            comp_lens.append(0)
            payload += seg
    if not comp_lens or not worth_keeping(len(payload), n):
        return None
    return _header(n, comp_lens) + bytes(payload)


def decompress_buffer_cpu(blob: bytes) -> bytes:
    """Raw bytes of a container; ``ValueError`` on a malformed header or a
    corrupt LZ4 segment, whichever backend decodes."""
    if _is_float_plane(blob):
        from . import fpcodec

        return fpcodec.decompress_buffer_cpu(blob)
    raw_len, comp_lens, off = validate_container(blob)
    core = _native_core()
    if core is not None:
        try:
            return core.malz_decompress(bytes(blob))
        except RuntimeError as exc:  # the core's std::runtime_error
            raise ValueError(f"LZ4 container corrupt: {exc}") from None
    from ..utils import lz4ref

    out = bytearray()
    pos = off
    for i, clen in enumerate(comp_lens):
        seg_raw = min(SEG_SIZE, raw_len - i * SEG_SIZE)
        if clen == 0:
            out += blob[pos : pos + seg_raw]
            pos += seg_raw
        else:
            try:
                out += lz4ref.decompress_block(blob[pos : pos + clen], seg_raw)
            except ValueError as exc:
                raise ValueError(f"{corrupt_message(i + 1)}: {exc}") from None
            pos += clen
    return bytes(out)


# ---------------------------------------------------------------------------
# GPU paths
# ---------------------------------------------------------------------------


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed: hipError {rc}")


def _to_dev(arr: Any) -> Any:
    import numpy as np
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


class Workspace:
    """Device buffers of one ``compress_spans_gpu`` call: the strided LZ4
    output (OUT_STRIDE per segment), comp_lens and seg_off per segment, and
    the dense containers."""

    def __init__(self, n_seg: int, dense_bytes: int) -> None:
        import torch

        self.n_seg = n_seg
        self.stride = torch.empty(n_seg * OUT_STRIDE, dtype=torch.uint8, device="cuda")
        self.dense = torch.empty(dense_bytes, dtype=torch.uint8, device="cuda")
        self.comp_lens = torch.empty(n_seg, dtype=torch.int32, device="cuda")
        self.seg_off = torch.empty(n_seg, dtype=torch.int64, device="cuda")

    @classmethod
    def for_lengths(cls, raw_lens: Sequence[int]) -> "Workspace":
        """Sized to one call: every span kept would still fit the dense part."""
        n_seg = sum(-(-n // SEG_SIZE) for n in raw_lens)
        return cls(n_seg, len(raw_lens) * HEADER_FIXED + 4 * n_seg + sum(raw_lens))


def compress_spans_gpu(
    lib: Any, base: int, spans: Sequence[tuple[int, int]], ws: Workspace
) -> list:
    """Containers of the device bytes ``(base + offset, raw_len)`` per span,
    None where compression does not pay. One LZ4 launch per span, one plan
    launch, ONE sync (the per-span payload totals), one assemble launch and
    one D2H of the dense containers, all on the current stream."""
    import numpy as np
    import torch

    from .staging import copy_from_device

    out: list = [None] * len(spans)
    if not spans:
        return out
    stream = torch.cuda.current_stream().cuda_stream
    first_seg, n_segs, sb = [], [], 0
    for off, ln in spans:
        n_seg = -(-ln // SEG_SIZE)
        if sb + n_seg > ws.n_seg:
            raise RuntimeError("compress spans exceed the workspace")
        _check(
            lib.ma_lz4_compress(
                base + off, ln, ws.stride.data_ptr() + sb * OUT_STRIDE,
                ws.comp_lens.data_ptr() + sb * 4, OUT_STRIDE, n_seg, stream,
            ),
            "lz4 compress kernel",
        )
        first_seg.append(sb)
        n_segs.append(n_seg)
        sb += n_seg
    raw_lens = np.array([ln for _off, ln in spans], dtype=np.int64)
    first_d = _to_dev(np.array(first_seg, dtype=np.int32))
    raw_d = _to_dev(raw_lens)
    src_off_d = _to_dev(np.array([off for off, _ln in spans], dtype=np.int64))
    payload_d = torch.empty(len(spans), dtype=torch.int64, device="cuda")
    _check(
        lib.ma_malz_plan(
            ws.comp_lens.data_ptr(), first_d.data_ptr(), raw_d.data_ptr(),
            ws.seg_off.data_ptr(), payload_d.data_ptr(), len(spans), stream,
        ),
        "malz plan kernel",
    )
    totals = payload_d.cpu().numpy()  # the one sync
    keep = worth_keeping(totals, raw_lens)
    sizes = np.where(keep, HEADER_FIXED + 4 * np.array(n_segs, dtype=np.int64) + totals, 0)
    ends = np.cumsum(sizes)
    out_off = np.where(keep, ends - sizes, -1)  # -1: the kernel skips the span
    dense_len = int(ends[-1])
    if dense_len == 0:
        return out
    if dense_len > ws.dense.numel():
        raise RuntimeError("dense containers exceed the workspace")
    out_off_d = _to_dev(out_off)
    _check(
        lib.ma_malz_assemble(
            base, src_off_d.data_ptr(), ws.stride.data_ptr(), OUT_STRIDE,
            ws.comp_lens.data_ptr(), ws.seg_off.data_ptr(), first_d.data_ptr(),
            raw_d.data_ptr(), ws.dense.data_ptr(), out_off_d.data_ptr(),
            len(spans), stream,
        ),
        "malz assemble kernel",
    )
    dense = copy_from_device(ws.dense.data_ptr(), dense_len)
    for j in np.flatnonzero(keep):
        out[j] = dense[out_off[j] : out_off[j] + sizes[j]]
    return out


def compress_buffer_gpu(data: bytes) -> Optional[bytes]:
    if len(data) == 0:
        return None
    lib = load_lib(required=True)
    from .staging import stage_to_gpu

    src = stage_to_gpu(data)
    ws = Workspace.for_lengths([len(data)])
    return compress_spans_gpu(lib, src.data_ptr(), [(0, len(data))], ws)[0]


def compress_buffers_gpu(buffers: list, staged: "object" = None, only: "object" = None) -> list:
    """Batched compression: ONE host->device transfer, ONE sync and ONE
    readback for a whole upload's blocks. ``staged`` is a
    ``stage_many_to_gpu`` result shared with the digest pass; ``only`` picks
    the buffers to compress. Returns per-buffer container bytes or None
    (incompressible / empty / not picked)."""
    lib = load_lib(required=True)
    out: list = [None] * len(buffers)
    pick = sorted(set(range(len(buffers))) if only is None else set(only))
    pick = [i for i in pick if len(buffers[i])]
    if not pick:
        return out
    if staged is None:
        from .staging import stage_many_to_gpu

        # one pinned H2D for all buffers, 4 KiB-aligned (no concat bytearray)
        staged = stage_many_to_gpu(buffers, align=SEG_SIZE)
    src, src_offsets = staged
    spans = [(src_offsets[i], len(buffers[i])) for i in pick]
    ws = Workspace.for_lengths([n for _off, n in spans])
    for i, container in zip(pick, compress_spans_gpu(lib, src.data_ptr(), spans, ws)):
        out[i] = container
    return out


def compress_buffers(buffers: list, staged: "object" = None, only: "object" = None) -> list:
    """GPU-batched when present; None entries otherwise (CPU compression
    is not worth its cost on the storage path)."""
    if gpu_available():
        return compress_buffers_gpu(buffers, staged=staged, only=only)
    return [None] * len(buffers)


def decompress_run_gpu(
    lib: Any, comp: int, headers: Sequence[tuple[int, Sequence[int]]], dst: int
) -> int:
    """Decompress a run of VALIDATED containers, ``headers`` their
    ``(raw_len, comp_lens)``, whose payloads lie back to back at device
    pointer ``comp`` and whose raw bytes are consecutive at ``dst``, on the
    current stream. Returns 0, or 1 + the run's first segment found corrupt;
    the stream has drained either way."""
    import numpy as np
    import torch

    comp_lens = np.concatenate([np.asarray(cl, dtype=np.int32) for _n, cl in headers])
    eff = np.concatenate([effective_lens(cl, n) for n, cl in headers])
    comp_offs = np.cumsum(eff)
    comp_offs -= eff  # exclusive
    offs_d = _to_dev(comp_offs)
    lens_d = _to_dev(comp_lens)
    # the kernel takes the min of 1 + index over the corrupt segments, so the
    # answer does not depend on which lane stores last; the max means none
    status = torch.full((1,), _STATUS_CLEAN, dtype=torch.int32, device="cuda")
    _check(
        lib.ma_lz4_decompress(
            comp, offs_d.data_ptr(), lens_d.data_ptr(), dst,
            sum(n for n, _cl in headers), status.data_ptr(), len(comp_lens),
            torch.cuda.current_stream().cuda_stream,
        ),
        "lz4 decompress kernel",
    )
    first_bad = int(status.item())  # syncs: the tables may be freed
    return 0 if first_bad == _STATUS_CLEAN else first_bad


def corrupt_message(status: int) -> str:
    return f"LZ4 container corrupt at segment {status - 1}"


def decompress_buffer_gpu(blob: bytes) -> bytes:
    if _is_float_plane(blob):
        from . import fpcodec

        return fpcodec.decompress_buffer_gpu(blob)
    raw_len, comp_lens, off = validate_container(blob)  # before any launch
    lib = load_lib(required=True)
    import torch

    from .staging import fetch_from_gpu, stage_to_gpu

    comp = stage_to_gpu(memoryview(blob)[off:])
    dst = torch.empty(raw_len, dtype=torch.uint8, device="cuda")
    bad = decompress_run_gpu(lib, comp.data_ptr(), [(raw_len, comp_lens)], dst.data_ptr())
    if bad:
        raise ValueError(corrupt_message(bad))
    return fetch_from_gpu(dst)


# ---------------------------------------------------------------------------
# dispatching front door (used by the CAS)
# ---------------------------------------------------------------------------


def compress_buffer(data: bytes) -> Optional[bytes]:
    """GPU when present; else the native C++ segment-parallel codec (the
    pure-Python fallback alone was not worth its cost — the C++ one is)."""
    if gpu_available():
        return compress_buffer_gpu(data)
    core = _native_core()
    if core is not None:
        return core.malz_compress(bytes(data), MIN_GAIN)
    return None


def decompress_buffer(blob: bytes) -> bytes:
    if gpu_available():
        try:
            return decompress_buffer_gpu(blob)
        except RuntimeError:
            pass
    return decompress_buffer_cpu(blob)

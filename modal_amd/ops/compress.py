"""Chunk (de)compression: container format over the HIP LZ4 kernels.

Container layout (little-endian):
  magic  b"MALZ41"             (6 bytes)
  raw_len  u64
  n_segments  u32              (raw split into 4 KiB segments)
  comp_len[n_segments]  u32    (0 => segment stored raw)
  payload                      (concatenated per-segment LZ4 blocks / raw)

Each segment is a standard LZ4 block, so any LZ4 block decoder can read the
payload; the CPU reference codec (utils/lz4ref.py) serves GPU-less readers.

What only MALZ41 knows lives here once: its header (``validate_container``,
the only parser), the LZ4 launches in front of the shared encoder tail
(``compress_spans_gpu``, the only device encoder) and the LZ4 decode launch
(``decompress_run_gpu``). The segmented container under it is
ops/container.py, which MAFP10 (ops/fpcodec.py) stands on as well.

``compress_buffer_gpu``/``compress_buffers_gpu`` (blobs) and ops/devcodec.py
(snapshots) are thin callers of these, so their containers are byte-identical
by construction and the CAS dedups between them.
"""

from __future__ import annotations

import struct
from typing import Any, NamedTuple, Optional, Sequence

from . import container, gpu_available, load_lib
from .container import MIN_GAIN, OUT_STRIDE, SEG_SIZE, Workspace, effective_lens, worth_keeping

MAGIC = b"MALZ41"
HEADER_FIXED = len(MAGIC) + 12  # magic + u64 raw_len + u32 n_seg


class Header(NamedTuple):
    raw_len: int
    seg_lens: Any  # int32 array: the comp_len of every segment
    payload_off: int


def _header(raw_len: int, comp_lens: Sequence[int]) -> bytes:
    return (
        MAGIC
        + struct.pack("<QI", raw_len, len(comp_lens))
        + struct.pack(f"<{len(comp_lens)}I", *comp_lens)
    )


def validate_container(
    blob: bytes, raw_len: Optional[int] = None, what: str = "container"
) -> Header:
    """Parse a container and bound everything a decoder will index with:
    magic, raw_len against the caller's (when given), n_seg against raw_len,
    every comp_len < SEG_SIZE, header + payload == len(blob). Returns
    (raw_len, comp_lens int32 array, payload offset); raises ValueError
    naming ``what``."""
    import numpy as np

    hdr_raw, n_seg, comp_lens, off = container.read_header(
        blob, raw_len, what, MAGIC, HEADER_FIXED, HEADER_FIXED - 4
    )
    if n_seg and int(comp_lens.max()) >= SEG_SIZE:
        raise ValueError(f"{what}: segment comp_len out of range")
    container.check_size(blob, off, int(effective_lens(comp_lens, hdr_raw).sum()), what)
    return Header(hdr_raw, comp_lens.astype(np.int32), off)


def parse_header(blob: bytes) -> tuple[int, list[int], int]:
    """Returns (raw_len, comp_lens, payload_offset) of a valid container."""
    raw_len, comp_lens, off = validate_container(blob)
    return raw_len, comp_lens.tolist(), off


def is_compressed(blob: bytes) -> bool:
    return blob.startswith(MAGIC)


def codec_of(blob: bytes) -> Any:
    """The module that reads a stored container: fpcodec for the MAFP10 magic,
    this one otherwise. Whether a blob is compressed at all is out of band (the
    ``.z`` suffix), so the magic only has to tell our two formats apart."""
    from . import compress, fpcodec  # here, so that importing this module needs no numpy

    return fpcodec if fpcodec.is_fp_container(blob) else compress


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
    codec = codec_of(blob)
    if codec.MAGIC != MAGIC:
        return codec.decompress_buffer_cpu(blob)
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


def compress_spans_gpu(
    lib: Any, base: int, spans: Sequence[tuple[int, int]], ws: Workspace
) -> list:
    """Containers of the device bytes ``(base + offset, raw_len)`` per span,
    None where compression does not pay. One LZ4 launch per span, then
    ``container.finish_containers``: one plan launch, ONE sync, one assemble
    launch and one D2H of the dense containers, all on the current stream."""
    import torch

    if not spans:
        return []
    stream = torch.cuda.current_stream().cuda_stream
    first_seg, n_segs, sb = [], [], 0
    for off, ln in spans:
        n_seg = -(-ln // SEG_SIZE)
        if sb + n_seg > ws.n_seg:
            raise RuntimeError("compress spans exceed the workspace")
        container.check(
            lib.ma_lz4_compress(
                base + off, ln, ws.stride.data_ptr() + sb * OUT_STRIDE,
                ws.comp_lens.data_ptr() + sb * 4, OUT_STRIDE, n_seg, stream,
            ),
            "lz4 compress kernel",
        )
        first_seg.append(sb)
        n_segs.append(n_seg)
        sb += n_seg
    first_d, raw_d, src_off_d = container.span_tables(spans, first_seg)

    def assemble(out_off_d: Any) -> None:
        rc = lib.ma_malz_assemble(
            base, src_off_d.data_ptr(), ws.stride.data_ptr(), OUT_STRIDE,
            ws.comp_lens.data_ptr(), ws.seg_off.data_ptr(), first_d.data_ptr(),
            raw_d.data_ptr(), ws.dense.data_ptr(), out_off_d.data_ptr(), len(spans), stream,
        )
        container.check(rc, "malz assemble kernel")

    return container.finish_containers(
        lib, spans, ws, first_d, raw_d, n_segs, HEADER_FIXED, assemble
    )


def compress_buffer_gpu(data: bytes) -> Optional[bytes]:
    if len(data) == 0:
        return None
    lib = load_lib(required=True)
    from .staging import stage_to_gpu

    src = stage_to_gpu(data)
    ws = Workspace.for_lengths([len(data)], HEADER_FIXED)
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
    ws = Workspace.for_lengths([n for _off, n in spans], HEADER_FIXED)
    for i, container in zip(pick, compress_spans_gpu(lib, src.data_ptr(), spans, ws)):
        out[i] = container
    return out


def compress_buffers(buffers: list, staged: "object" = None, only: "object" = None) -> list:
    """GPU-batched when present; None entries otherwise (CPU compression
    is not worth its cost on the storage path)."""
    if gpu_available():
        return compress_buffers_gpu(buffers, staged=staged, only=only)
    return [None] * len(buffers)


def decompress_run_gpu(lib: Any, comp: int, headers: Sequence[Sequence], dst: int) -> int:
    """Decompress a run of VALIDATED containers, ``headers`` what
    ``validate_container`` returned for each (only ``raw_len`` and the
    comp_lens, fields 0 and 1, are read), whose payloads lie back to back at
    device pointer ``comp`` and whose raw bytes are consecutive at ``dst``, on
    the current stream. Returns 0, or 1 + the run's first segment found
    corrupt; the stream has drained either way."""
    import numpy as np

    comp_lens = np.concatenate([np.asarray(h[1], dtype=np.int32) for h in headers])
    eff = np.concatenate([effective_lens(h[1], h[0]) for h in headers])
    comp_offs = np.cumsum(eff)
    comp_offs -= eff  # exclusive
    offs_d = container.to_dev(comp_offs)
    lens_d = container.to_dev(comp_lens)
    raw_total = sum(h[0] for h in headers)
    return container.decode_status(
        lambda status, stream: lib.ma_lz4_decompress(
            comp, offs_d.data_ptr(), lens_d.data_ptr(), dst, raw_total, status,
            len(comp_lens), stream,
        ),
        "lz4 decompress kernel",
    )


def corrupt_message(status: int) -> str:
    return f"LZ4 container corrupt at segment {status - 1}"


def decompress_buffer_gpu(blob: bytes) -> bytes:
    return container.decompress_buffer_gpu(codec_of(blob), blob)


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

"""Byte-plane codec: the MAFB10 container for blocks of 1-byte elements.

An fp8 tensor, an fp8 KV cache and the e8m0 scale tensor of an MX-quantised
model have no mantissa bytes to leave alone: the whole element is sign and
exponent and a few mantissa bits, and its distribution is as skewed as the
top byte of a bf16. MAFB10 is MAFP10 (ops/fpcodec.py) at element size 1: it
codes EVERY byte of a block as its rank in the block's frequency order,
packs the ranks at a fixed width chosen per 4 KiB segment and escapes the
rare ones. N(0,1) cast to float8_e4m3fn comes out at 0.88 of raw, to
float8_e5m2 at 0.76, e8m0 block scales at 0.20. Packed fp4 pairs and
per-block absmax int8 do not compress this way; the 5 % rule leaves them raw.

Container layout (little-endian, 4096-byte segments; the fixed header has
the size and the fields of MAFP10's, so ops/container.py serves both):

  magic    b"MAFB10"                 6
  raw_len  u64                       8
  es       u8  (1)                   1
  reserved u8  (0)                   1
  n_seg    u32 == ceil(raw_len/4096) 4
  order    u8[256]   a permutation: order[r] = the byte value of rank r
  seg_len  u32[n_seg]  bytes the segment takes in the payload; 0 => raw (L)
  payload  segments back to back

``order``: histogram of every byte of the block, sorted by count descending,
ties by byte value ascending.

A coded segment of ``m = L`` bytes is: one byte ``b`` in 1..7; ceil(m*b/8)
bytes of codes, element i in bits [i*b, (i+1)*b) of the stream, least
significant bit first, zero pad bits; then the raw byte of every element
whose code is the escape 2^b-1, in element order. A code is the byte's rank
when that is below the escape. ``b`` minimises
hi = 1 + ceil(m*b/8) + n_escapes(b), smallest b on ties; the segment is coded
only if hi < m (never when m < 3), and then seg_len = hi. The container is
kept under the one 5 % rule, ``container.worth_keeping``.

The magic is new because a deployed MAFP10 reader knows element sizes 2 and
4 only: it rejects a MAFB10 container where it would misread an ``es`` of 1.

What only MAFB10 knows lives here once: its header checks, the numpy codec
(the model the kernels in csrc/bytez.hip are held to byte for byte, and the
reader of GPU-less processes), the device encoder's launches up to the stride
slots and the decode launch. The width rule and the bit packing are
fpcodec's own helpers.
"""

from __future__ import annotations

import struct
import sys
from typing import Any, NamedTuple, Optional, Sequence

import numpy as np

from . import container, gpu_available, load_lib
from .container import OUT_STRIDE, SEG_SIZE, Workspace, effective_lens, seg_raw_lens, worth_keeping
from .fpcodec import _code_rows, _pack_rows, block_order

MAGIC = b"MAFB10"
HEADER_FIXED = len(MAGIC) + 8 + 1 + 1 + 4 + 256  # up to the seg_len table


class Header(NamedTuple):
    raw_len: int
    seg_lens: Any  # int32 array
    payload_off: int
    order: Any  # uint8[256]


def is_byte_container(blob: bytes) -> bool:
    return bytes(blob[: len(MAGIC)]) == MAGIC


def validate_container(
    blob: bytes, raw_len: Optional[int] = None, what: str = "container"
) -> Header:
    """Parse a MAFB10 container and bound everything a decoder indexes with.
    Raises ValueError naming ``what``."""
    order = None  # set by the check that runs inside the shared reader

    def elem_fields() -> None:
        es, reserved = struct.unpack_from("<BB", blob, len(MAGIC) + 8)
        if es != 1:
            raise ValueError(f"{what}: element size {es} is not 1")
        if reserved != 0:
            raise ValueError(f"{what}: reserved byte is not 0")

    def order_table() -> None:
        nonlocal order
        order = np.frombuffer(blob, dtype=np.uint8, count=256, offset=HEADER_FIXED - 256)
        if not np.array_equal(np.sort(order), np.arange(256, dtype=np.uint8)):
            raise ValueError(f"{what}: order table is not a permutation")

    hdr_raw, n_seg, seg_lens, off = container.read_header(
        blob, raw_len, what, MAGIC, HEADER_FIXED, len(MAGIC) + 10, elem_fields, order_table
    )
    seg_lens = seg_lens.astype(np.int64)
    L = seg_raw_lens(n_seg, hdr_raw)
    coded = seg_lens != 0
    if np.any(coded & ((seg_lens < 2) | (seg_lens >= L))):
        raise ValueError(f"{what}: segment seg_len out of range")
    container.check_size(blob, off, int(np.where(coded, seg_lens, L).sum()), what)
    return Header(hdr_raw, seg_lens.astype(np.int32), off, order)


def corrupt_message(status: int) -> str:
    return f"MAFB10 container corrupt at segment {status - 1}"


# ---------------------------------------------------------------------------
# the numpy model
# ---------------------------------------------------------------------------


def _groups(n: int) -> list:
    """(first segment, count, m) of the segments that can be coded: the full
    ones together, then the short last one."""
    groups = [(0, n // SEG_SIZE, SEG_SIZE), (n // SEG_SIZE, 1, n % SEG_SIZE)]
    return [(first, count, m) for first, count, m in groups if count and m >= 3]


def compress_buffer_cpu(data: Any) -> Optional[bytes]:
    """The MAFB10 container of ``data``, or None when it does not save 5 %."""
    data = np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8)
    n = len(data)
    if n == 0:
        return None
    n_seg = -(-n // SEG_SIZE)
    order = block_order(data, 1)
    rank_of = np.empty(256, dtype=np.uint8)
    rank_of[order] = np.arange(256, dtype=np.uint8)
    ranks = rank_of[data]

    # pass 1: every segment's width and seg_len
    seg_lens = np.zeros(n_seg, dtype=np.int64)
    widths = np.zeros(n_seg, dtype=np.int64)
    for first, count, m in _groups(n):
        rows = ranks[first * SEG_SIZE : first * SEG_SIZE + count * m].reshape(count, m)
        b_row, hi = _code_rows(rows, m)
        coded = hi < m
        widths[first : first + count] = np.where(coded, b_row, 0)
        seg_lens[first : first + count] = np.where(coded, hi, 0)
    eff = effective_lens(seg_lens, n)
    if not worth_keeping(int(eff.sum()), n):
        return None

    # pass 2: the payload, every segment at its offset
    offs = np.cumsum(eff) - eff
    payload = np.empty(int(eff.sum()), dtype=np.uint8)
    for s in np.flatnonzero(seg_lens == 0):
        payload[offs[s] : offs[s] + eff[s]] = data[s * SEG_SIZE : s * SEG_SIZE + eff[s]]
    for first, count, m in _groups(n):
        span = slice(first * SEG_SIZE, first * SEG_SIZE + count * m)
        elems, rows_ranks = data[span].reshape(count, m), ranks[span].reshape(count, m)
        for b in np.unique(widths[first : first + count]):
            if b == 0:
                continue
            b = int(b)
            rows = np.flatnonzero(widths[first : first + count] == b)
            at = offs[first + rows][:, None]
            nbytes = (m * b + 7) // 8
            payload[at[:, 0]] = b
            payload[at + 1 + np.arange(nbytes)] = _pack_rows(rows_ranks[rows], b)
            esc = rows_ranks[rows] >= (1 << b) - 1
            nth = np.cumsum(esc, axis=1) - 1  # an escape's place among its segment's
            payload[(at + (1 + nbytes) + nth)[esc]] = elems[rows][esc]
    header = (
        MAGIC + struct.pack("<QBBI", n, 1, 0, n_seg) + order.tobytes()
        + seg_lens.astype("<u4").tobytes()
    )
    return header + payload.tobytes()


def decompress_buffer_cpu(blob: bytes) -> bytes:
    """Raw bytes of a MAFB10 container; ValueError on a malformed header or
    a corrupt segment (the first one is named)."""
    hdr = validate_container(blob)
    n = hdr.raw_len
    buf = np.frombuffer(blob, dtype=np.uint8)
    out = np.empty(n, dtype=np.uint8)
    seg_lens = hdr.seg_lens.astype(np.int64)
    m_of = seg_raw_lens(len(seg_lens), n)
    eff = effective_lens(seg_lens, n)
    offs = hdr.payload_off + np.cumsum(eff) - eff
    for s in np.flatnonzero(seg_lens == 0):
        out[s * SEG_SIZE : s * SEG_SIZE + eff[s]] = buf[offs[s] : offs[s] + eff[s]]

    coded = np.flatnonzero(seg_lens)
    b_of = np.zeros(len(seg_lens), dtype=np.int64)
    b_of[coded] = buf[offs[coded]]
    ok = (b_of >= 1) & (b_of <= 7) & (1 + (m_of * b_of + 7) // 8 <= seg_lens)
    bad = coded[~ok[coded]].tolist()
    # segments of one length and one width decode together
    for m, b in sorted({(int(m_of[s]), int(b_of[s])) for s in coded if ok[s]}):
        rows = coded[(m_of[coded] == m) & (b_of[coded] == b) & ok[coded]]
        nbytes = (m * b + 7) // 8
        at = offs[rows][:, None]
        bits = np.unpackbits(buf[at + 1 + np.arange(nbytes)], axis=1, bitorder="little")
        bits = bits[:, : m * b].reshape(len(rows), m, b)
        codes = np.packbits(bits, axis=2, bitorder="little").reshape(len(rows), m)
        esc = codes == (1 << b) - 1
        fits = esc.sum(axis=1) == seg_lens[rows] - 1 - nbytes
        bad += rows[~fits].tolist()
        rows, at, codes, esc = rows[fits], at[fits], codes[fits], esc[fits]
        elems = hdr.order[codes]
        nth = np.cumsum(esc, axis=1) - 1
        elems[esc] = buf[(at + (1 + nbytes) + nth)[esc]]
        for row, s in zip(elems, rows):
            out[s * SEG_SIZE : s * SEG_SIZE + m] = row
    if bad:
        raise ValueError(f"{corrupt_message(min(bad) + 1)}: bad code width or escape count")
    return out.tobytes()


# ---------------------------------------------------------------------------
# GPU paths
# ---------------------------------------------------------------------------


def compress_spans_gpu(
    lib: Any, base: int, spans: Sequence[tuple[int, int]], ws: Workspace
) -> list:
    """MAFB10 containers of the device bytes ``(base + offset, raw_len)`` per
    span, None where the container is not kept. One histogram, one rank and
    one encode launch for all spans, then ``container.finish_containers`` (one
    plan launch, ONE sync, one assemble launch, one D2H of the dense
    containers), all on the current stream."""
    import torch

    if not spans:
        return []
    stream = torch.cuda.current_stream().cuda_stream
    n_segs = np.array([-(-ln // SEG_SIZE) for _off, ln in spans], dtype=np.int64)
    ends_seg = np.cumsum(n_segs)
    if int(ends_seg[-1]) > ws.n_seg:
        raise RuntimeError("compress spans exceed the workspace")
    first_d, raw_d, src_off_d = container.span_tables(spans, ends_seg - n_segs)
    tables = torch.empty(2, len(spans) * 256, dtype=torch.uint8, device="cuda")
    order_d, rank_d = tables[0], tables[1]
    counts = torch.zeros(len(spans) * 256, dtype=torch.int32, device="cuda")
    container.check(
        lib.ma_bytez_rank(
            base, src_off_d.data_ptr(), raw_d.data_ptr(), counts.data_ptr(),
            order_d.data_ptr(), rank_d.data_ptr(), len(spans), stream,
        ),
        "bytez histogram/rank kernels",
    )
    container.check(
        lib.ma_bytez_encode(
            base, src_off_d.data_ptr(), raw_d.data_ptr(), first_d.data_ptr(),
            rank_d.data_ptr(), ws.stride.data_ptr(), OUT_STRIDE,
            ws.comp_lens.data_ptr(), len(spans), int(n_segs.max()), stream,
        ),
        "bytez encode kernel",
    )

    def assemble(out_off_d: Any) -> None:
        rc = lib.ma_bytez_assemble(
            base, src_off_d.data_ptr(), ws.stride.data_ptr(), OUT_STRIDE,
            ws.comp_lens.data_ptr(), ws.seg_off.data_ptr(), first_d.data_ptr(),
            raw_d.data_ptr(), order_d.data_ptr(), ws.dense.data_ptr(),
            out_off_d.data_ptr(), len(spans), stream,
        )
        container.check(rc, "bytez assemble kernel")

    return container.finish_containers(
        lib, spans, ws, first_d, raw_d, n_segs, HEADER_FIXED, assemble
    )


def decompress_run_gpu(lib: Any, comp: int, headers: Sequence[Header], dst: int) -> int:
    """Decompress a run of VALIDATED containers, ``headers`` what
    ``validate_container`` returned for each, whose payloads lie back to back
    at device pointer ``comp`` and whose raw bytes are consecutive at ``dst``,
    on the current stream. Returns 0, or 1 + the run's first segment found
    corrupt; the stream has drained either way."""
    if not sum(len(h.seg_lens) for h in headers):
        return 0
    offs_d, ints_d, order_d, n_segments = container.run_tables(headers)
    return container.decode_status(
        lambda status, stream: lib.ma_bytez_decode(
            comp, offs_d[0].data_ptr(), offs_d[1].data_ptr(), ints_d[0].data_ptr(),
            ints_d[1].data_ptr(), ints_d[2].data_ptr(), order_d.data_ptr(),
            dst, status, n_segments, stream,
        ),
        "bytez decode kernel",
    )


def decompress_buffer_gpu(blob: bytes) -> bytes:
    return container.decompress_buffer_gpu(sys.modules[__name__], blob)


# ---------------------------------------------------------------------------
# dispatching front door
# ---------------------------------------------------------------------------


def compress_buffer_gpu(data: bytes) -> Optional[bytes]:
    if len(data) == 0:
        return None
    lib = load_lib(required=True)
    from .staging import stage_to_gpu

    src = stage_to_gpu(data)
    ws = Workspace.for_lengths([len(data)], HEADER_FIXED)
    return compress_spans_gpu(lib, src.data_ptr(), [(0, len(data))], ws)[0]


def compress_buffer(data: bytes) -> Optional[bytes]:
    """GPU when present, else the numpy codec: the same container either way."""
    if gpu_available():
        return compress_buffer_gpu(data)
    return compress_buffer_cpu(data)

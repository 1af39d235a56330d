"""Float-plane codec: the MAFP10 container for bf16/fp16/fp32 blocks.

LZ4 finds no matches in floating-point weights; their redundancy is in the
exponent. MAFP10 codes the TOP byte of every element (sign + exponent bits)
as its rank in a per-block frequency order, packs the ranks at a fixed width
chosen per 4 KiB segment, escapes the rare ranks, and leaves the mantissa
bytes alone.

Container layout (little-endian; ``es`` the element size, 4096-byte segments
as in MALZ41, ``m = L // es`` the element count of a segment of ``L`` bytes):

  magic    b"MAFP10"                 6
  raw_len  u64                       8
  es       u8  (2 or 4)              1
  reserved u8  (0)                   1
  n_seg    u32 == ceil(raw_len/4096) 4
  order    u8[256]   a permutation: order[r] = the byte value of rank r
  seg_len  u32[n_seg]  bytes the segment takes in the payload; 0 => raw (L)
  payload  segments back to back

``order``: histogram of the byte at offset es-1 of every WHOLE element of
the block, sorted by count descending, ties by byte value ascending.

A coded segment is: the low es-1 bytes of each element in memory order
(m*(es-1) bytes); one byte ``b`` in 1..7; ceil(m*b/8) bytes of codes, element
i in bits [i*b, (i+1)*b) of the stream, least significant bit first, zero
pad bits; then the raw top byte of every element whose code is the escape
2^b-1, in element order. A code is the top byte's rank when that is below
the escape. ``b`` minimises hi = 1 + ceil(m*b/8) + n_escapes(b), smallest b
on ties; the segment is coded only if L % es == 0 and hi < m, so
seg_len = m*(es-1) + hi < L. The container is kept under the one 5 % rule,
``container.worth_keeping``.

A caller that does not know ``es`` (untyped device memory) asks the bytes:
the probe gives the block's top-byte histograms at both element sizes and
``choose_elem_size`` picks the one at which the container comes out smaller,
or none.

What only MAFP10 knows lives here once: its header fields and their checks,
the numpy codec (the model the kernels in csrc/fpz.hip are held to byte for
byte, and the reader of GPU-less processes), the probe and its rule, the
device encoder's launches up to the stride slots and the decode launch.
``seg_len`` means what MALZ41's ``comp_len`` means, so the segmented
container under both is one layer, ops/container.py.
"""

from __future__ import annotations

import struct
import sys
from typing import Any, NamedTuple, Optional, Sequence

import numpy as np

from . import container, gpu_available, load_lib
from .container import OUT_STRIDE, SEG_SIZE, Workspace, effective_lens, seg_raw_lens, worth_keeping

MAGIC = b"MAFP10"
ELEM_SIZES = (2, 4)
HEADER_FIXED = len(MAGIC) + 8 + 1 + 1 + 4 + 256  # up to the seg_len table


class Header(NamedTuple):
    raw_len: int
    seg_lens: Any  # int32 array
    payload_off: int
    es: int
    order: Any  # uint8[256]


def is_fp_container(blob: bytes) -> bool:
    return bytes(blob[: len(MAGIC)]) == MAGIC


def validate_container(
    blob: bytes, raw_len: Optional[int] = None, what: str = "container"
) -> Header:
    """Parse a MAFP10 container and bound everything a decoder indexes with.
    Raises ValueError naming ``what``."""

    es, order = 0, None  # set by the two checks that run inside the shared reader

    def elem_fields() -> None:
        nonlocal es
        es, reserved = struct.unpack_from("<BB", blob, len(MAGIC) + 8)
        if es not in ELEM_SIZES:
            raise ValueError(f"{what}: element size {es} is not 2 or 4")
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
    if np.any(coded & (L % es != 0)):
        raise ValueError(f"{what}: coded segment is not a whole number of elements")
    lo = (L // es) * (es - 1)
    if np.any(coded & ((seg_lens < lo + 2) | (seg_lens >= L))):
        raise ValueError(f"{what}: segment seg_len out of range")
    container.check_size(blob, off, int(np.where(coded, seg_lens, L).sum()), what)
    return Header(hdr_raw, seg_lens.astype(np.int32), off, es, order)


def corrupt_message(status: int) -> str:
    return f"MAFP10 container corrupt at segment {status - 1}"


# ---------------------------------------------------------------------------
# the numpy model
# ---------------------------------------------------------------------------


def _header(raw_len: int, es: int, order: Any, seg_lens: Any) -> bytes:
    return (
        MAGIC
        + struct.pack("<QBBI", raw_len, es, 0, len(seg_lens))
        + np.asarray(order, dtype=np.uint8).tobytes()
        + np.asarray(seg_lens, dtype="<u4").tobytes()
    )


def block_order(data: Any, es: int) -> Any:
    """order[r] = byte value of rank r over the top bytes of the block's
    whole elements: count descending, byte value ascending on ties."""
    whole = (len(data) // es) * es
    counts = np.bincount(data[es - 1 : whole : es], minlength=256)
    return np.lexsort((np.arange(256), -counts)).astype(np.uint8)


def _code_rows(ranks: Any, m: int) -> tuple[Any, Any]:
    """(b, hi) per row of ``ranks`` (n x m): the width that minimises
    1 + ceil(m*b/8) + n_escapes(b), smallest b on ties."""
    widths = np.arange(1, 8)
    esc = np.stack([(ranks >= (1 << b) - 1).sum(axis=1) for b in widths], axis=1)
    cost = 1 + (m * widths + 7) // 8 + esc
    pick = cost.argmin(axis=1)  # the first minimum: the smallest b
    return widths[pick], cost[np.arange(len(pick)), pick]


def _pack_rows(ranks: Any, b: int) -> Any:
    """Rows of ranks (n x m) -> n x ceil(m*b/8) code bytes at width b."""
    codes = np.minimum(ranks, (1 << b) - 1).astype(np.uint8)
    bits = np.unpackbits(codes[:, :, None], axis=2, bitorder="little")[:, :, :b]
    return np.packbits(bits.reshape(len(ranks), -1), axis=1, bitorder="little")


def compress_buffer_cpu(data: Any, es: int) -> Optional[bytes]:
    """The MAFP10 container of ``data`` at element size ``es``, or None when
    it does not save 5 %."""
    if es not in ELEM_SIZES:
        raise ValueError(f"element size {es} is not 2 or 4")
    data = np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8)
    n = len(data)
    if n == 0:
        return None
    n_seg = -(-n // SEG_SIZE)
    order = block_order(data, es)
    rank_of = np.empty(256, dtype=np.uint8)
    rank_of[order] = np.arange(256, dtype=np.uint8)

    # pass 1: every segment's width and seg_len; full segments together, then
    # the short last one, through the same steps
    seg_lens = np.zeros(n_seg, dtype=np.int64)
    widths = np.zeros(n_seg, dtype=np.int64)
    groups = [(0, n // SEG_SIZE, SEG_SIZE), (n // SEG_SIZE, 1 if n % SEG_SIZE else 0, n % SEG_SIZE)]
    groups = [(first, count, L) for first, count, L in groups if count and L % es == 0]
    ranks_of_group = {}
    for first, count, L in groups:
        m = L // es
        tops = data[first * SEG_SIZE : first * SEG_SIZE + count * L].reshape(count, m, es)[:, :, es - 1]
        ranks = ranks_of_group[first] = rank_of[tops]
        b_row, hi = _code_rows(ranks, m)
        coded = hi < m
        widths[first : first + count] = np.where(coded, b_row, 0)
        seg_lens[first : first + count] = np.where(coded, m * (es - 1) + hi, 0)
    eff = effective_lens(seg_lens, n)
    if not worth_keeping(int(eff.sum()), n):
        return None

    # pass 2: the payload, every segment at its offset
    offs = np.cumsum(eff) - eff
    payload = np.empty(int(eff.sum()), dtype=np.uint8)
    for s in np.flatnonzero(seg_lens == 0):
        payload[offs[s] : offs[s] + eff[s]] = data[s * SEG_SIZE : s * SEG_SIZE + eff[s]]
    for first, count, L in groups:
        m = L // es
        lo = m * (es - 1)
        elems = data[first * SEG_SIZE : first * SEG_SIZE + count * L].reshape(count, m, es)
        for b in np.unique(widths[first : first + count]):
            if b == 0:
                continue
            b = int(b)
            rows = np.flatnonzero(widths[first : first + count] == b)
            at = offs[first + rows][:, None]
            nbytes = (m * b + 7) // 8
            payload[at + np.arange(lo)] = elems[rows, :, : es - 1].reshape(len(rows), lo)
            payload[at[:, 0] + lo] = b
            ranks = ranks_of_group[first][rows]
            payload[at + (lo + 1) + np.arange(nbytes)] = _pack_rows(ranks, b)
            esc = ranks >= (1 << b) - 1
            nth = np.cumsum(esc, axis=1) - 1  # an escape's place among its segment's
            payload[(at + (lo + 1 + nbytes) + nth)[esc]] = elems[rows, :, es - 1][esc]
    return _header(n, es, order, seg_lens) + payload.tobytes()


# ---------------------------------------------------------------------------
# the element-size probe: its numpy twin and the rule
# ---------------------------------------------------------------------------

#: "find the element size in the bytes": what callers that have no element
#: type pass where 0, 2 or 4 goes
AUTO = -1


def probe_counts_cpu(data: Any) -> tuple[Any, Any]:
    """(counts2, counts4): the histograms ``block_order`` sorts at ``es`` 2
    and at ``es`` 4, 256 int64 counts each. The numpy twin of
    ``fpz_probe_kernel``."""
    data = np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8)
    n = len(data)
    return (
        np.bincount(data[1 : n - n % 2 : 2], minlength=256),
        np.bincount(data[3 : n - n % 4 : 4], minlength=256),
    )


def _estimate(counts: Any, raw_len: Any, es: int) -> Any:
    """The estimate of ``choose_elem_size`` at ``es``, in int64: for one
    table (256 counts, a scalar raw_len) or a table per row and as many
    lengths."""
    raw_len = np.asarray(raw_len, dtype=np.int64)
    n = raw_len // es
    # top[..., k - 1]: the k largest counts together
    top = np.cumsum(-np.sort(-np.asarray(counts, dtype=np.int64), axis=-1), axis=-1)
    hi = np.min(
        [-(-n * b // 8) + n - top[..., (1 << b) - 2] for b in range(1, 8)], axis=0
    )
    return n * (es - 1) + hi + -(-raw_len // SEG_SIZE) + (raw_len - n * es)


def _choose(counts2: Any, counts4: Any, raw_len: Any) -> tuple[Any, Any]:
    e2, e4 = _estimate(counts2, raw_len, 2), _estimate(counts4, raw_len, 4)
    est = np.minimum(e2, e4)
    es = np.where(e2 <= e4, 2, 4)
    return np.where(worth_keeping(est, np.asarray(raw_len, dtype=np.int64)), es, 0), est


def choose_elem_size(counts2: Any, counts4: Any, raw_len: int) -> tuple[int, int]:
    """(es, estimate): the element size at which MAFP10 would store a block
    of ``raw_len`` bytes with these two histograms smaller, and the payload
    estimated for it; ``es`` is 0 when even that misses
    ``container.worth_keeping``. Exact integer arithmetic, so the same tables
    give the same answer anywhere.

    For ``es`` in (2, 4), ``n = raw_len // es`` elements and the counts
    sorted descending, the top bytes cost
    ``hi = min over b in 1..7 of ceil(n*b/8) + (n - the 2^b - 1 largest counts)``
    (codes at ONE width for the block plus the elements that width escapes) and
    ``estimate = n*(es-1) + hi + n_seg + (raw_len - n*es)``: the low bytes, a
    width byte per segment, the bytes of no whole element. 2 wins ties.

    Why this bounds the encoder's payload. The escapes of a width summed over
    the segments are the block's, and a full segment's ``m`` (2048 or 1024) is
    a multiple of 8, so its code bytes at any width are exactly ``m*b/8``:
    the segments coded all at the block's best width cost what the estimate
    says. The encoder picks a width per segment, which can only cost less,
    and stores a segment raw only when coding it would not be smaller. What
    is left is the short last segment: its ``ceil`` can round up, and when its
    length is no multiple of ``es`` it is stored raw, where the estimate coded
    its whole elements. Either way the excess is less than ``SEG_SIZE``, and
    there is none when ``raw_len`` is a multiple of 4. The estimate leaves out
    the header and the segment table, as ``worth_keeping`` does."""
    es, est = _choose(counts2, counts4, raw_len)
    return int(es), int(est)


def decompress_buffer_cpu(blob: bytes) -> bytes:
    """Raw bytes of a MAFP10 container; ValueError on a malformed header or
    a corrupt segment (the first one is named)."""
    hdr = validate_container(blob)
    es, n = hdr.es, hdr.raw_len
    buf = np.frombuffer(blob, dtype=np.uint8)
    out = np.empty(n, dtype=np.uint8)
    seg_lens = hdr.seg_lens.astype(np.int64)
    L_of = seg_raw_lens(len(seg_lens), n)
    eff = effective_lens(seg_lens, n)
    offs = hdr.payload_off + np.cumsum(eff) - eff
    for s in np.flatnonzero(seg_lens == 0):
        out[s * SEG_SIZE : s * SEG_SIZE + eff[s]] = buf[offs[s] : offs[s] + eff[s]]

    coded = np.flatnonzero(seg_lens)
    lo_of = (L_of // es) * (es - 1)
    b_of = np.zeros(len(seg_lens), dtype=np.int64)
    b_of[coded] = buf[offs[coded] + lo_of[coded]]
    nbytes_of = ((L_of // es) * b_of + 7) // 8
    ok = (b_of >= 1) & (b_of <= 7) & (lo_of + 1 + nbytes_of <= seg_lens)
    bad = coded[~ok[coded]].tolist()
    # segments of one length and one width decode together
    for L, b in sorted({(int(L_of[s]), int(b_of[s])) for s in coded if ok[s]}):
        rows = coded[(L_of[coded] == L) & (b_of[coded] == b) & ok[coded]]
        m = L // es
        lo, nbytes = m * (es - 1), (m * b + 7) // 8
        at = offs[rows][:, None]
        bits = np.unpackbits(buf[at + (lo + 1) + np.arange(nbytes)], axis=1, bitorder="little")
        bits = bits[:, : m * b].reshape(len(rows), m, b)
        codes = np.packbits(bits, axis=2, bitorder="little").reshape(len(rows), m)
        esc = codes == (1 << b) - 1
        fits = esc.sum(axis=1) == seg_lens[rows] - lo - 1 - nbytes
        bad += rows[~fits].tolist()
        rows, at, codes, esc = rows[fits], at[fits], codes[fits], esc[fits]
        elems = np.empty((len(rows), m, es), dtype=np.uint8)
        elems[:, :, : es - 1] = buf[at + np.arange(lo)].reshape(len(rows), m, es - 1)
        tops = hdr.order[codes]
        nth = np.cumsum(esc, axis=1) - 1
        tops[esc] = buf[(at + (lo + 1 + nbytes) + nth)[esc]]
        elems[:, :, es - 1] = tops
        if L == SEG_SIZE:
            out[: (n // SEG_SIZE) * SEG_SIZE].reshape(-1, SEG_SIZE)[rows] = elems.reshape(-1, L)
        elif len(rows):
            out[rows[0] * SEG_SIZE :] = elems.reshape(-1)
    if bad:
        raise ValueError(
            f"{corrupt_message(min(bad) + 1)}: bad code width or escape count"
        )
    return out.tobytes()


# ---------------------------------------------------------------------------
# GPU paths
# ---------------------------------------------------------------------------


def probe_spans_gpu(lib: Any, base: int, spans: Sequence[tuple[int, int]]) -> tuple[list, Any]:
    """``choose_elem_size`` for the device bytes ``(base + offset, raw_len)``
    of every span: (the element size per span, 0 where MAFP10 would not pay;
    the probe's tables, a ``len(spans) x 2 x 256`` int32 device tensor whose
    ``[:, 0]`` and ``[:, 1]`` are the histograms at es 2 and 4). One probe
    launch and one D2H of the tables (2 KiB per span) on the current stream;
    the rule itself runs on the host, on the same tables as the numpy path."""
    import torch

    counts = torch.zeros(len(spans), 2, 256, dtype=torch.int32, device="cuda")
    if not spans:
        return [], counts
    src_off_d = container.to_dev(np.array([off for off, _ln in spans], dtype=np.int64))
    raw_d = container.to_dev(np.array([ln for _off, ln in spans], dtype=np.int64))
    container.check(
        lib.ma_fpz_probe(
            base, src_off_d.data_ptr(), raw_d.data_ptr(), counts.data_ptr(), len(spans),
            torch.cuda.current_stream().cuda_stream,
        ),
        "fpz probe kernel",
    )
    host = counts.cpu().numpy().view(np.uint32)  # syncs: the tables may be freed
    es, _est = _choose(host[:, 0], host[:, 1], [ln for _off, ln in spans])  # all spans at once
    return es.tolist(), counts


def compress_spans_gpu(
    lib: Any, base: int, spans: Sequence[tuple[int, int]], es: int, ws: Workspace,
    counts: Any = None,
) -> list:
    """MAFP10 containers of the device bytes ``(base + offset, raw_len)`` per
    span, None where the container is not kept. One histogram, one rank and
    one encode launch for all spans, then ``container.finish_containers`` (one
    plan launch, ONE sync, one assemble launch, one D2H of the dense
    containers), all on the current stream. ``counts``, a contiguous
    ``len(spans) x 256`` int32 device tensor, is the spans' histograms at ``es``
    where the caller has them (``probe_spans_gpu``): no histogram launch then."""
    import torch

    if es not in ELEM_SIZES:
        raise ValueError(f"element size {es} is not 2 or 4")
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
    if counts is None:
        counts = torch.zeros(len(spans) * 256, dtype=torch.int32, device="cuda")
        rc = lib.ma_fpz_rank(
            base, src_off_d.data_ptr(), raw_d.data_ptr(), es, counts.data_ptr(),
            order_d.data_ptr(), rank_d.data_ptr(), len(spans), stream,
        )
    else:
        if (
            counts.dtype != torch.int32 or counts.numel() != len(spans) * 256
            or not counts.is_cuda or not counts.is_contiguous()
        ):
            raise ValueError("counts is a contiguous int32 device tensor of len(spans) x 256")
        rc = lib.ma_fpz_rank_counts(
            counts.data_ptr(), order_d.data_ptr(), rank_d.data_ptr(), len(spans), stream
        )
    container.check(rc, "fpz histogram/rank kernels")
    container.check(
        lib.ma_fpz_encode(
            base, src_off_d.data_ptr(), raw_d.data_ptr(), first_d.data_ptr(),
            rank_d.data_ptr(), es, ws.stride.data_ptr(), OUT_STRIDE,
            ws.comp_lens.data_ptr(), len(spans), int(n_segs.max()), stream,
        ),
        "fpz encode kernel",
    )

    def assemble(out_off_d: Any) -> None:
        rc = lib.ma_fpz_assemble(
            base, src_off_d.data_ptr(), ws.stride.data_ptr(), OUT_STRIDE,
            ws.comp_lens.data_ptr(), ws.seg_off.data_ptr(), first_d.data_ptr(),
            raw_d.data_ptr(), order_d.data_ptr(), es, ws.dense.data_ptr(),
            out_off_d.data_ptr(), len(spans), stream,
        )
        container.check(rc, "fpz assemble kernel")

    return container.finish_containers(
        lib, spans, ws, first_d, raw_d, n_segs, HEADER_FIXED, assemble
    )


def decompress_run_gpu(lib: Any, comp: int, headers: Sequence[Header], dst: int) -> int:
    """Decompress a run of VALIDATED containers, ``headers`` what
    ``validate_container`` returned for each, whose payloads lie back to back
    at device pointer ``comp`` and whose raw bytes are consecutive at ``dst``,
    on the current stream. Returns 0, or 1 + the run's first segment found
    corrupt; the stream has drained either way."""
    seg_lens = np.concatenate([np.asarray(h.seg_lens, dtype=np.int32) for h in headers])
    if len(seg_lens) == 0:
        return 0
    eff = np.concatenate([effective_lens(h.seg_lens, h.raw_len) for h in headers])
    raw = np.concatenate([seg_raw_lens(len(h.seg_lens), h.raw_len) for h in headers])
    comp_offs = np.cumsum(eff) - eff
    dst_offs = np.cumsum(raw) - raw
    blk = np.repeat(np.arange(len(headers), dtype=np.int32), [len(h.seg_lens) for h in headers])
    offs_d = container.to_dev(np.stack([comp_offs, dst_offs]).astype(np.int64))
    ints_d = container.to_dev(np.stack([seg_lens, raw.astype(np.int32), blk]).astype(np.int32))
    order_d = container.to_dev(np.concatenate([np.asarray(h.order, dtype=np.uint8) for h in headers]))
    es_d = container.to_dev(np.array([h.es for h in headers], dtype=np.uint8))
    return container.decode_status(
        lambda status, stream: lib.ma_fpz_decode(
            comp, offs_d[0].data_ptr(), offs_d[1].data_ptr(), ints_d[0].data_ptr(),
            ints_d[1].data_ptr(), ints_d[2].data_ptr(), order_d.data_ptr(),
            es_d.data_ptr(), dst, status, len(seg_lens), stream,
        ),
        "fpz decode kernel",
    )


def decompress_buffer_gpu(blob: bytes) -> bytes:
    return container.decompress_buffer_gpu(sys.modules[__name__], blob)


# ---------------------------------------------------------------------------
# dispatching front door
# ---------------------------------------------------------------------------


def compress_buffer_gpu(data: bytes, es: int) -> Optional[bytes]:
    if len(data) == 0:
        return None
    lib = load_lib(required=True)
    from .staging import stage_to_gpu

    src = stage_to_gpu(data)
    ws = Workspace.for_lengths([len(data)], HEADER_FIXED)
    return compress_spans_gpu(lib, src.data_ptr(), [(0, len(data))], es, ws)[0]


def compress_buffer(data: bytes, es: int) -> Optional[bytes]:
    """GPU when present, else the numpy codec: the same container either way."""
    if gpu_available():
        return compress_buffer_gpu(data, es)
    return compress_buffer_cpu(data, es)

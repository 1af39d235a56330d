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

What only MAFP10 knows lives here: its magic and element sizes, the kernels
of csrc/fpz.hip that encode and decode it, and the probe and its rule. The
codec itself, numpy model and device paths, is ops/rankcodec.py, which
MAFB10 (ops/bytecodec.py) stands on too; the names below are that codec
bound to ``FORMAT``. ``seg_len`` means what MALZ41's ``comp_len`` means, so
the segmented container under all three is one layer, ops/container.py.
"""

from __future__ import annotations

from typing import Any, Sequence

import numpy as np

from . import container, rankcodec
from .container import SEG_SIZE, worth_keeping
from .container import Workspace  # noqa: F401  (a public name of this module)
from .rankcodec import HEADER_FIXED, Header, block_order  # noqa: F401  (public names)

MAGIC = b"MAFP10"
ELEM_SIZES = (2, 4)
FORMAT = rankcodec.Format(
    MAGIC, ELEM_SIZES, "2 or 4", "fpz", "ma_fpz_encode", "ma_fpz_decode",
    es_in_abi=True,
)

is_fp_container = FORMAT.is_container
validate_container = FORMAT.validate_container
corrupt_message = FORMAT.corrupt_message
compress_buffer_cpu = FORMAT.compress_buffer_cpu
decompress_buffer_cpu = FORMAT.decompress_buffer_cpu
compress_spans_gpu = FORMAT.compress_spans_gpu
decompress_run_gpu = FORMAT.decompress_run_gpu
decompress_buffer_gpu = FORMAT.decompress_buffer_gpu
compress_buffer_gpu = FORMAT.compress_buffer_gpu
compress_buffer = FORMAT.compress_buffer


# ---------------------------------------------------------------------------
# the element-size probe: its numpy twin and the rule
# ---------------------------------------------------------------------------

#: "find the element size in the bytes": what callers that have no element
#: type pass where 0, 2 or 4 goes
AUTO = -1


def probe_counts_cpu(data: Any) -> tuple[Any, Any]:
    """(counts2, counts4): the histograms ``block_order`` sorts at ``es`` 2
    and at ``es`` 4, 256 int64 counts each. The numpy twin of
    ``ma_fpz_probe``."""
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

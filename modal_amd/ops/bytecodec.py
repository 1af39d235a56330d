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

What only MAFB10 knows lives here: its magic, its one element size and the
kernels of csrc/bytez.hip that encode and decode it. The codec itself, numpy
model and device paths, is ops/rankcodec.py at element size 1; the names
below are that codec bound to ``FORMAT``, without the ``es`` argument.
"""

from __future__ import annotations

from typing import Any, Optional, Sequence

from . import rankcodec
from .container import SEG_SIZE, Workspace  # noqa: F401  (public names)
from .rankcodec import HEADER_FIXED, Header  # noqa: F401  (public names)

MAGIC = b"MAFB10"
FORMAT = rankcodec.Format(
    MAGIC, (1,), "1", "bytez", "ma_bytez_encode", "ma_bytez_decode",
    es_in_abi=False,
)

is_byte_container = FORMAT.is_container
validate_container = FORMAT.validate_container
corrupt_message = FORMAT.corrupt_message
decompress_buffer_cpu = FORMAT.decompress_buffer_cpu
decompress_run_gpu = FORMAT.decompress_run_gpu
decompress_buffer_gpu = FORMAT.decompress_buffer_gpu


def compress_buffer_cpu(data: Any) -> Optional[bytes]:
    return FORMAT.compress_buffer_cpu(data, 1)


def compress_spans_gpu(
    lib: Any, base: int, spans: Sequence[tuple[int, int]], ws: Workspace
) -> list:
    return FORMAT.compress_spans_gpu(lib, base, spans, 1, ws)


def compress_buffer_gpu(data: bytes) -> Optional[bytes]:
    return FORMAT.compress_buffer_gpu(data, 1)


def compress_buffer(data: bytes) -> Optional[bytes]:
    return FORMAT.compress_buffer(data, 1)

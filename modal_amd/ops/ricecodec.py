"""Rice-coded rank planes: the MARC10 container, the opt-in alternative to
MAFP10 (ops/fpcodec.py) and MAFB10 (ops/bytecodec.py) at element sizes 1, 2
and 4 under one magic.

Those two pack the rank of every element's top byte at one fixed width per
4 KiB segment. The ranks of a Gaussian's sign-and-exponent byte fall off
geometrically, and a Golomb-Rice code is the code for that: no table, no tree,
and a parameter per segment. N(0,1) as bf16 comes out at 0.68 of raw where
MAFP10 gives 0.71, float8_e4m3fn at 0.83 for 0.88, float8_e5m2 at 0.71 for
0.76. A variable-length code still has to decode in parallel, so a segment's
elements are cut into 16 byte-aligned sub-streams with a table of their ends.

Container layout: the fixed header of ``rankcodec.HEADER_FIXED`` (magic
b"MARC10", raw_len u64, es u8 in {1, 2, 4}, reserved 0, n_seg u32, ``order``
u8[256] = ``rankcodec.block_order``, ``seg_len`` u32[n_seg] with 0 => raw),
then the segments back to back. A segment of ``L`` bytes is coded only when
``L % es == 0``; with ``m = L // es`` and ``lo = m * (es - 1)`` it is

  low      lo bytes: the low es-1 bytes of every element in memory order
  k        u8, the Rice parameter, 0..7
  end      u16[16]: end[j] is the byte offset in the stream area at which
           sub-stream j ends; non-decreasing, end[15] the area's length
  streams  sub-stream j holds elements [j*per, (j+1)*per), per = ceil(m/16),
           in order, bits filling every byte from the least significant

For rank ``r`` of an element's top byte and ``q = r >> k``: when ``q < 12``,
``q`` one-bits, a zero bit and the ``k`` low bits of ``r``, lowest first;
otherwise 12 one-bits and the 8 bits of the raw top byte, lowest first. A
sub-stream is exactly ceil(bits/8) bytes and its pad bits are zero.
``hi = 1 + 32 + end[15]``; ``k`` minimises it, smallest on ties; the segment
is coded only if ``hi < m`` and then ``seg_len = lo + hi``. The container is
kept under ``container.worth_keeping``.

A reader rejects a coded segment whose ``k`` is above 7, whose ``end``
decreases, where ``lo + 33 + end[15] != seg_len``, where a sub-stream's
elements consume more bits than it has, where a sub-stream is not exactly
ceil(consumed/8) bytes, where a pad bit is set, or where a code stands for a
rank above 255 (``q << k`` can, no encoder writes one). ``validate_container``
checks the first three, which bound everything a decoder indexes with and
cost 33 bytes a segment; the walk that finds the others is the decoder's.

The numpy codec here is the specification; the kernels of csrc/ricez.hip
match it byte for byte. It advances every sub-stream of every segment one
element per step, at most 256 steps a call. Histogram, rank, assemble, plan
and the container layer are the ones MAFP10 and MAFB10 use.
"""

from __future__ import annotations

from typing import Any, Optional

import numpy as np

from . import rankcodec
from .container import SEG_SIZE, Workspace, effective_lens, seg_raw_lens, worth_keeping  # noqa: F401
from .rankcodec import HEADER_FIXED, Header, block_order  # noqa: F401  (public names)

MAGIC = b"MARC10"
ELEM_SIZES = (1, 2, 4)
SUBS = 16  # sub-streams per segment
Q_ESC = 12  # a unary run this long announces a raw byte
HI_FIXED = 1 + 2 * SUBS  # k and the end table
_KS = np.arange(8)
#: trailing one-bits of a 12-bit value, capped at Q_ESC
_ONES = np.array([(~v & (v + 1)).bit_length() - 1 for v in range(1 << Q_ESC)], dtype=np.int64)
_ONES[-1] = Q_ESC


def code_bits(ranks: Any, k: Any) -> Any:
    """Bits the code of every rank takes at parameter ``k`` (broadcast)."""
    q = ranks >> k
    return np.where(q < Q_ESC, q + 1 + k, Q_ESC + 8)


def estimate(counts: Any, raw_len: Any, es: int) -> Any:
    """What ``probe.choose_elem_size`` compares under Rice coding, in int64:
    with the counts sorted descending ``c_r`` and ``n = raw_len // es``,
    ``n*(es-1) + min_k ceil(sum_r c_r * code_bits(r, k) / 8) + 49*n_seg
    + (raw_len - n*es)``; the 49 is k, the end table and a pad byte per
    sub-stream. For one table or a table per row, like ``fpcodec._estimate``."""
    raw_len = np.asarray(raw_len, dtype=np.int64)
    n = raw_len // es
    c = -np.sort(-np.asarray(counts, dtype=np.int64), axis=-1)
    bits = np.stack([(c * code_bits(np.arange(256), k)).sum(axis=-1) for k in _KS])
    top = (-(-bits // 8)).min(axis=0)
    return n * (es - 1) + top + (HI_FIXED + SUBS) * -(-raw_len // SEG_SIZE) + (raw_len - n * es)


def _groups(n: int, es: int) -> list:
    """(first segment, count, L) of the segments that may be coded: the full
    ones together, then the short last one when it is whole elements."""
    groups = [(0, n // SEG_SIZE, SEG_SIZE), (n // SEG_SIZE, 1 if n % SEG_SIZE else 0, n % SEG_SIZE)]
    return [(first, count, L) for first, count, L in groups if count and L % es == 0]


def _by_sub(a: Any, m: int) -> Any:
    """count x m values -> count x SUBS x per, zero past element m."""
    per = -(-m // SUBS)
    out = np.zeros((len(a), SUBS * per), dtype=a.dtype)
    out[:, :m] = a
    return out.reshape(len(a), SUBS, per)


def _encode_streams(ranks: Any, tops: Any, k: Any, m: int) -> tuple[Any, Any]:
    """(rows x width bytes, rows bit counts) of the sub-streams of segments
    whose ranks and top bytes are ``count x m`` and parameters ``k``; row
    ``SUBS * s + j`` is sub-stream j of segment s."""
    per = -(-m // SUBS)
    rows = len(ranks) * SUBS
    r_of = _by_sub(ranks.astype(np.int64), m).reshape(rows, per)
    t_of = _by_sub(tops.astype(np.int64), m).reshape(rows, per)
    live = _by_sub(np.ones_like(ranks, dtype=bool), m).reshape(rows, per)
    k = np.repeat(np.asarray(k, dtype=np.int64), SUBS)
    buf = np.zeros((rows, (per * (Q_ESC + 8) + 7) // 8 + 4), dtype=np.uint8)
    pos = np.zeros(rows, dtype=np.int64)
    at = np.arange(rows)
    for j in range(per):  # every sub-stream advances one element
        r, q = r_of[:, j], r_of[:, j] >> k
        code = np.where(
            q < Q_ESC,
            ((1 << np.minimum(q, Q_ESC)) - 1) | ((r & ((1 << k) - 1)) << np.minimum(q + 1, Q_ESC)),
            ((1 << Q_ESC) - 1) | (t_of[:, j] << Q_ESC),
        )
        code = np.where(live[:, j], code, 0) << (pos & 7)
        for b in range(4):  # 20 bits from any bit of a byte: four bytes
            buf[at, (pos >> 3) + b] |= ((code >> (8 * b)) & 255).astype(np.uint8)
        pos += np.where(live[:, j], code_bits(r, k), 0)
    return buf, pos


class _RiceFormat(rankcodec.Format):
    """``rankcodec.Format`` with MARC10's segment layout: its device paths
    and header, this module's numpy codec and checks."""

    # -- what a reader checks ------------------------------------------------

    def _segment_fields(self, buf: Any, hdr: Header) -> tuple:
        """Per segment: (L, lo, offset in ``buf``, k, end as n_seg x SUBS
        int64, whether it is coded and its three fields are sound)."""
        seg_lens = hdr.seg_lens.astype(np.int64)
        L = seg_raw_lens(len(seg_lens), hdr.raw_len)
        eff = effective_lens(seg_lens, hdr.raw_len)
        offs = hdr.payload_off + np.cumsum(eff) - eff
        lo = (L // hdr.es) * (hdr.es - 1)
        coded = seg_lens != 0
        at = np.where(coded, offs + lo, 0)  # validated: lo + 33 <= seg_len
        fields = np.lib.stride_tricks.sliding_window_view(buf, HI_FIXED)[at]  # n_seg x 33, a copy
        k = fields[:, 0].astype(np.int64)
        end = np.ascontiguousarray(fields[:, 1:]).view("<u2").astype(np.int64)
        sound = (
            (k <= 7) & np.all(np.diff(end, axis=1) >= 0, axis=1)
            & (lo + HI_FIXED + end[:, -1] == seg_lens)
        )
        return L, lo, offs, k, end, coded, coded & sound

    def validate_container(
        self, blob: bytes, raw_len: Optional[int] = None, what: str = "container"
    ) -> Header:
        hdr = super().validate_container(blob, raw_len, what)
        buf = np.frombuffer(blob, dtype=np.uint8)
        *_rest, coded, sound = self._segment_fields(buf, hdr)
        if np.any(coded & ~sound):
            first = int(np.flatnonzero(coded & ~sound)[0])
            raise ValueError(f"{what}: segment {first}: bad Rice parameter or end table")
        return hdr

    # -- the numpy model -----------------------------------------------------

    def compress_buffer_cpu(self, data: Any, es: int) -> Optional[bytes]:
        """The container of ``data`` at element size ``es``, or None when it
        does not save 5 %."""
        self._check_es(es)
        data = np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8)
        n = len(data)
        if n == 0:
            return None
        n_seg = -(-n // SEG_SIZE)
        order = block_order(data, es)
        rank_of = np.empty(256, dtype=np.uint8)
        rank_of[order] = np.arange(256, dtype=np.uint8)

        # pass 1: every segment's k and seg_len, from the bits per sub-stream
        seg_lens = np.zeros(n_seg, dtype=np.int64)
        k_of = np.zeros(n_seg, dtype=np.int64)
        groups = _groups(n, es)
        for first, count, L in groups:
            m = L // es
            tops = data[first * SEG_SIZE : first * SEG_SIZE + count * L].reshape(count, m, es)[:, :, es - 1]
            ranks = rank_of[tops].astype(np.int32)
            hi = np.stack(
                [
                    HI_FIXED + (-(-_by_sub(code_bits(ranks, k), m).sum(axis=2) // 8)).sum(axis=1)
                    for k in range(8)
                ],
                axis=1,
            )
            pick = hi.argmin(axis=1)  # the first minimum: the smallest k
            best = hi[np.arange(count), pick]
            k_of[first : first + count] = pick
            seg_lens[first : first + count] = np.where(best < m, m * (es - 1) + best, 0)
        eff = effective_lens(seg_lens, n)
        if not worth_keeping(int(eff.sum()), n):
            return None

        # pass 2: the payload, every segment at its offset
        offs = np.cumsum(eff) - eff
        payload = np.empty(int(eff.sum()), dtype=np.uint8)
        for s in np.flatnonzero(seg_lens == 0):
            payload[offs[s] : offs[s] + eff[s]] = data[s * SEG_SIZE : s * SEG_SIZE + eff[s]]
        for first, count, L in groups:
            rows = np.flatnonzero(seg_lens[first : first + count])
            if not len(rows):
                continue
            m = L // es
            lo = m * (es - 1)
            elems = data[first * SEG_SIZE : first * SEG_SIZE + count * L].reshape(count, m, es)[rows]
            at = offs[first + rows][:, None]
            k = k_of[first + rows]
            buf, bits = _encode_streams(rank_of[elems[:, :, es - 1]], elems[:, :, es - 1], k, m)
            lens = (-(-bits // 8)).reshape(len(rows), SUBS)
            end = np.cumsum(lens, axis=1)
            payload[at + np.arange(lo)] = elems[:, :, : es - 1].reshape(len(rows), lo)
            payload[at[:, 0] + lo] = k
            payload[at + (lo + 1) + np.arange(2 * SUBS)] = end.astype("<u2").view(np.uint8)
            start = (at + (lo + HI_FIXED) + end - lens).reshape(-1, 1)
            col = np.arange(buf.shape[1])
            mine = col < lens.reshape(-1, 1)
            payload[(start + col)[mine]] = buf[mine]
        return self._header(n, es, order, seg_lens) + payload.tobytes()

    def decompress_buffer_cpu(self, blob: bytes) -> bytes:
        """Raw bytes of a container; ValueError on a malformed header or a
        corrupt segment (the first one is named)."""
        hdr = rankcodec.Format.validate_container(self, blob)
        es, n = hdr.es, hdr.raw_len
        buf = np.frombuffer(blob, dtype=np.uint8)
        out = np.empty(n, dtype=np.uint8)
        L_of, lo_of, offs, k_of, end_of, coded, sound = self._segment_fields(buf, hdr)
        for s in np.flatnonzero(~coded):
            out[s * SEG_SIZE : s * SEG_SIZE + L_of[s]] = buf[offs[s] : offs[s] + L_of[s]]
        bad = np.flatnonzero(coded & ~sound).tolist()
        for L in sorted(set(L_of[sound].tolist())):  # the full segments, the short last one
            rows = np.flatnonzero(sound & (L_of == L))
            m = L // es
            lo, per = m * (es - 1), -(-m // SUBS)
            at = offs[rows][:, None]
            end = end_of[rows]
            lens = np.diff(end, axis=1, prepend=0).reshape(-1)
            start = (at + (lo + HI_FIXED) + end).reshape(-1) - lens
            k = np.repeat(k_of[rows], SUBS)
            count = np.clip(m - np.arange(SUBS) * per, 0, per)
            count = np.tile(count, len(rows))
            # every sub-stream in a row of its own, zeros behind it
            width = (per * (Q_ESC + 8) + 7) // 8 + 4
            col = np.arange(width)
            mine = col < lens[:, None]
            sbuf = np.zeros((len(lens), width), dtype=np.uint8)
            sbuf[mine] = buf[np.minimum(start[:, None] + col, len(buf) - 1)[mine]]
            pos = np.zeros(len(lens), dtype=np.int64)
            fine = np.ones(len(lens), dtype=bool)
            tops = np.zeros((len(lens), per), dtype=np.uint8)
            row = np.arange(len(lens))
            for j in range(per):  # every sub-stream advances one element
                live = j < count
                byte = np.minimum(pos >> 3, width - 4)
                w = sum(sbuf[row, byte + b].astype(np.int64) << (8 * b) for b in range(4)) >> (pos & 7)
                q = _ONES[w & ((1 << Q_ESC) - 1)]
                esc = q == Q_ESC
                r = (q << k) | ((w >> (q + 1)) & ((1 << k) - 1))
                fine &= ~live | esc | (r < 256)
                tops[:, j] = np.where(esc, (w >> Q_ESC) & 255, hdr.order[np.minimum(r, 255)])
                pos += np.where(live, np.where(esc, Q_ESC + 8, q + 1 + k), 0)
                fine &= pos <= 8 * lens  # zeros behind a stream decode; this catches them
            last = sbuf[row, np.maximum(lens - 1, 0)].astype(np.int64)
            fine &= (-(-pos // 8) == lens) & (((pos & 7) == 0) | ((last >> (pos & 7)) == 0))
            fine = fine.reshape(len(rows), SUBS).all(axis=1)
            bad += rows[~fine].tolist()
            rows, at = rows[fine], at[fine]
            elems = np.empty((len(rows), m, es), dtype=np.uint8)
            elems[:, :, : es - 1] = buf[at + np.arange(lo)].reshape(len(rows), m, es - 1)
            elems[:, :, es - 1] = tops.reshape(-1, SUBS * per)[fine][:, :m]
            if L == SEG_SIZE:
                out[: (n // SEG_SIZE) * SEG_SIZE].reshape(-1, SEG_SIZE)[rows] = elems.reshape(-1, L)
            elif len(rows):
                out[rows[0] * SEG_SIZE :] = elems.reshape(-1)
        if bad:
            raise ValueError(f"{self.corrupt_message(min(bad) + 1)}: bad Rice header or sub-stream")
        return out.tobytes()


FORMAT = _RiceFormat(
    MAGIC, ELEM_SIZES, "1, 2 or 4", "ricez", "ma_ricez_encode", "ma_ricez_decode",
    es_in_abi=True, min_hi=HI_FIXED,
)

is_rice_container = FORMAT.is_container
validate_container = FORMAT.validate_container
corrupt_message = FORMAT.corrupt_message
compress_buffer_cpu = FORMAT.compress_buffer_cpu
decompress_buffer_cpu = FORMAT.decompress_buffer_cpu
compress_spans_gpu = FORMAT.compress_spans_gpu
decompress_run_gpu = FORMAT.decompress_run_gpu
decompress_buffer_gpu = FORMAT.decompress_buffer_gpu
compress_buffer_gpu = FORMAT.compress_buffer_gpu
compress_buffer = FORMAT.compress_buffer

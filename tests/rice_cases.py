"""Inputs of the MARC10 path tests (tests/test_ricecases_cpu.py, _gpu.py): a
bit-serial reference of the segment and container layout, and named inputs
that reach every Rice parameter the encoder can pick, dense escapes, the
smallest segments that code and a block of mixed segments.

The reference is written from the "Container layout" and "A reader rejects"
paragraphs of the ``ops/ricecodec.py`` docstring alone, in plain Python
integers, a bit or a code at a time; of ``ricecodec`` it takes constants and
nothing else. Its writer is given ``k``, so it also makes the segments no
encoder writes: a ``k`` that is not the minimum, ``k`` = 7, a rank above 255.

At ``k`` = 7 every code is at least 8 bits, so a sub-stream is at least a byte
an element and ``seg_len`` is at least ``L + 33``: ``validate_container`` and
the kernel's ``seg_len < L`` turn every such segment away before a walk. A
segment at ``k`` = 7 therefore reaches a decoder only malformed further on,
and ``bad_rank`` makes one whose first code is the first rule broken.
"""

from __future__ import annotations

import struct
from typing import Any, Optional

import numpy as np

from modal_amd.ops.ricecodec import HEADER_FIXED, HI_FIXED, MAGIC, Q_ESC, SEG_SIZE, SUBS

SEG = SEG_SIZE
#: the rules of "A reader rejects", in the order of that paragraph
RULES = ("k", "end", "seg_len", "overrun", "length", "pad", "rank")


class Esc(int):
    """A code that is an escaped top byte; a plain int is a rank."""


# ---------------------------------------------------------------------------
# the bit-serial reference
# ---------------------------------------------------------------------------


def _code(c: int, k: int) -> list:
    if isinstance(c, Esc):
        return [1] * Q_ESC + [(c >> i) & 1 for i in range(8)]
    q = c >> k
    if q >= Q_ESC:
        raise ValueError(f"rank {c} has no unary code at k = {k}")
    return [1] * q + [0] + [(c >> i) & 1 for i in range(k)]


def write_segment(low: bytes, codes: list, k: int) -> bytes:
    """``low | k | end[16] | streams`` of a segment of ``len(codes)`` elements."""
    m = len(codes)
    per = -(-m // SUBS)
    streams, ends = b"", []
    for j in range(SUBS):
        bits: list = []
        for c in codes[j * per : (j + 1) * per]:
            bits += _code(c, k)
        bits += [0] * (-len(bits) % 8)
        streams += bytes(
            sum(bit << i for i, bit in enumerate(bits[b : b + 8])) for b in range(0, len(bits), 8)
        )
        ends.append(len(streams))
    return bytes(low) + bytes([k]) + struct.pack("<16H", *ends) + streams


def read_segment(seg: bytes, L: int, es: int) -> Any:
    """The codes of a coded segment of ``L`` raw bytes (ranks, ``Esc`` top
    bytes), or the name of the first rule of ``RULES`` it breaks."""
    m = L // es
    lo, per = m * (es - 1), -(-m // SUBS)
    k = seg[lo]
    if k > 7:
        return "k"
    ends = struct.unpack_from("<16H", seg, lo + 1)
    if any(b < a for a, b in zip(ends, ends[1:])):
        return "end"
    if lo + HI_FIXED + ends[-1] != len(seg):
        return "seg_len"
    codes: list = []
    for j in range(SUBS):
        first = ends[j - 1] if j else 0
        stream = seg[lo + HI_FIXED + first : lo + HI_FIXED + ends[j]]
        bits = [(byte >> i) & 1 for byte in stream for i in range(8)]
        pos = 0
        for _ in range(min(max(m - j * per, 0), per)):
            q = 0
            while q < Q_ESC and pos + q < len(bits) and bits[pos + q]:
                q += 1
            width = Q_ESC + 8 if q == Q_ESC else q + 1 + k
            if pos + width > len(bits):
                return "overrun"
            body = bits[pos + width - (8 if q == Q_ESC else k) : pos + width]
            value = sum(bit << i for i, bit in enumerate(body))
            pos += width
            if q == Q_ESC:
                codes.append(Esc(value))
            elif (q << k) | value > 255:
                return "rank"
            else:
                codes.append((q << k) | value)
        if -(-pos // 8) != len(stream):
            return "length"
        if any(bits[pos:]):
            return "pad"
    return codes


def tops_of(codes: list, order: Any) -> bytes:
    return bytes(c if isinstance(c, Esc) else int(order[c]) for c in codes)


def write_container(raw_len: int, es: int, order: Any, segments: list) -> bytes:
    """The container of ``segments``, each ``(coded, its bytes)``."""
    table = [len(body) if coded else 0 for coded, body in segments]
    return (
        MAGIC + struct.pack("<QBBI", raw_len, es, 0, len(segments)) + bytes(bytearray(order))
        + struct.pack(f"<{len(table)}I", *table) + b"".join(body for _coded, body in segments)
    )


def read_container(blob: bytes) -> tuple:
    """(raw_len, es, order, [(coded, its bytes, L)]) of a well-formed container."""
    raw_len, es, _zero, n_seg = struct.unpack_from("<QBBI", blob, len(MAGIC))
    order = blob[HEADER_FIXED - 256 : HEADER_FIXED]
    table = struct.unpack_from(f"<{n_seg}I", blob, HEADER_FIXED)
    at, segments = HEADER_FIXED + 4 * n_seg, []
    for s, seg_len in enumerate(table):
        L = min(SEG, raw_len - s * SEG)
        segments.append((seg_len != 0, blob[at : at + (seg_len or L)], L))
        at += seg_len or L
    assert at == len(blob)
    return raw_len, es, order, segments


def decode_container(blob: bytes) -> Any:
    """The raw bytes, or (segment, rule) of the first segment a reader rejects."""
    raw_len, es, order, segments = read_container(blob)
    out = b""
    for s, (coded, body, L) in enumerate(segments):
        if not coded:
            out += body
            continue
        codes = read_segment(body, L, es)
        if isinstance(codes, str):
            return s, codes
        m = L // es
        elems = np.empty((m, es), dtype=np.uint8)
        elems[:, : es - 1] = np.frombuffer(body[: m * (es - 1)], dtype=np.uint8).reshape(m, es - 1)
        elems[:, es - 1] = np.frombuffer(tops_of(codes, order), dtype=np.uint8)
        out += elems.tobytes()
    assert len(out) == raw_len
    return out


def order_of(raw: bytes, es: int) -> list:
    """``order`` of the layout: the top bytes of the whole elements by count
    descending, byte value ascending on ties."""
    counts = [0] * 256
    for i in range(es - 1, (len(raw) // es) * es, es):
        counts[raw[i]] += 1
    return sorted(range(256), key=lambda v: (-counts[v], v))


def forced(raw: bytes, es: int, ks: list, patch: Optional[dict] = None) -> bytes:
    """The container of ``raw`` with segment s coded at ``ks[s]`` (None: stored
    raw), an element's rank escaped where ``k`` leaves it no unary code;
    ``patch`` maps (segment, element) to the code written there instead."""
    order = order_of(raw, es)
    rank_of = {v: r for r, v in enumerate(order)}
    segments = []
    for s, k in enumerate(ks):
        seg = raw[s * SEG : (s + 1) * SEG]
        if k is None:
            segments.append((False, seg))
            continue
        tops = seg[es - 1 :: es]
        codes = [rank_of[t] if rank_of[t] >> k < Q_ESC else Esc(t) for t in tops]
        for (ps, i), c in (patch or {}).items():
            if ps == s:
                codes[i] = c
        low = bytes(b for i, b in enumerate(seg) if i % es != es - 1)
        segments.append((True, write_segment(low, codes, k)))
    return write_container(len(raw), es, order, segments)


# ---------------------------------------------------------------------------
# the named cases: name -> (raw bytes, es)
# ---------------------------------------------------------------------------

ELEM_SIZES = (1, 2, 4)
#: tails of the small-segment cases in elements; 49 is the fewest that code
#: at every element size (48 elements are 16 sub-streams of a byte: hi = 49)
MIN_M = {1: 49, 2: 49, 4: 49}
TAILS = {1: (49, 50, 64, 65, 100, 257), 2: (49, 50), 4: (49, 50)}
#: A segment with e escapes has at least 20e + (m - e) bits, and hi < m needs
#: 33 + bits/8 < m: e < (7m - 264) / 19, 363 at es 4 where m is 1024. The
#: dense-escape case asks for 500 in a segment at es 1 and 2 and 250 at es 4.
ESCAPE_SHARE = {1: 0.25, 2: 0.30, 4: 0.29}
MIN_ESCAPES = {1: 500, 2: 500, 4: 250}
#: 1024 elements over N values as often as each other, at ranks 1..N: k = 6
#: beats k = 5 once N passes 129 and still codes while 9 - 192/N bits an
#: element fit 1024 - 33 bytes, N up to 144
K6_VALUES_ES4 = 136


def _elems(rng: Any, tops: Any, es: int) -> bytes:
    """Elements with the top bytes ``tops`` and random low bytes."""
    out = rng.integers(0, 256, (len(tops), es), dtype=np.uint8)
    out[:, es - 1] = tops
    return out.tobytes()


def _uniform(rng: Any, n_values: int, m: int, first: int = 0) -> Any:
    """``m`` top bytes, every one of ``n_values`` values as often as the next
    (the smaller values once more where it does not divide), shuffled."""
    return rng.permutation((np.arange(m) % n_values + first).astype(np.uint8))


def _dominant(rng: Any, m: int, byte: int, others: Any, share: float) -> Any:
    """``m`` top bytes ``byte`` but for ``int(share * m)`` of them, which take
    ``others`` in turn, at random places."""
    tops = np.full(m, byte, dtype=np.uint8)
    where = rng.permutation(m)[: int(share * m)]
    tops[where] = np.resize(np.asarray(others, dtype=np.uint8), len(where))
    return tops


def _build() -> dict:
    cases: dict = {}
    for es in ELEM_SIZES:
        rng = np.random.default_rng(1000 + es)
        full = SEG // es
        # the low bytes are stored as they are, so at es 2 and 4 a block keeps
        # its container only with constant segments in front of the others
        front = np.full((es - 1) * full, 7, dtype=np.uint8)
        # every k: top bytes uniform over 2^j values, two segments
        for j in range(1, 8):
            tops = np.concatenate([front, _uniform(rng, 1 << j, 2 * full, 40)])
            cases[f"uniform_{1 << j}_es{es}"] = (_elems(rng, tops, es), es)
        # k = 6: a segment uniform over N values behind three constant ones
        n_values = {1: 160, 2: 160, 4: K6_VALUES_ES4}[es]
        tops = np.concatenate([np.full(3 * full, 7, dtype=np.uint8), _uniform(rng, n_values, full, 40)])
        cases[f"k6_es{es}"] = (_elems(rng, tops, es), es)
        # dense escapes: a dominant byte, a share of elements over 200 others
        tops = np.concatenate([front, _dominant(rng, 2 * full, 7, np.arange(50, 250), ESCAPE_SHARE[es])])
        cases[f"escapes_es{es}"] = (_elems(rng, tops, es), es)
        # forty escapes in a row inside one sub-stream
        tops = np.full(full, 0x3C, dtype=np.uint8)
        tops[5 : 5 + 40] = 0xA7 - np.arange(40)
        tops[full - 50 : full - 10] = 0x47 - np.arange(40)
        cases[f"escape_run_es{es}"] = (_elems(rng, tops, es), es)
        # a compressible full segment and a short tail, one in ten of whose
        # elements has the second most frequent byte
        for m in TAILS[es]:
            tops = _dominant(rng, full + m, 0x3C, [0x3D], 0.1)
            cases[f"tail_{m}_es{es}"] = (_elems(rng, tops, es), es)
        # three k and a raw segment in the middle
        tops = np.concatenate([
            np.full(full, 0x10, dtype=np.uint8),
            _uniform(rng, 8, full, 0x10),
            rng.integers(0, 256, full, dtype=np.uint8),
            _uniform(rng, 64, full, 0x10),
            _dominant(rng, full // 2, 0x10, [0x11, 0x12], 0.3),
        ])
        cases[f"mixed_es{es}"] = (_elems(rng, tops, es), es)
    return cases


CASES = _build()

#: case -> a k per segment that the encoder does not pick for it and that
#: still codes (hi < m): rank codes longer than need be, and at a larger k
#: fewer escapes, at a smaller one more
FORCED = {
    "uniform_2_es1": [3, 1],
    "escapes_es1": [1, 2],
    "uniform_64_es1": [3, 6],
    "mixed_es2": [2, 3, None, 5, 1],
    "tail_49_es4": [1, 1],
}


def forced_case(name: str) -> bytes:
    raw, es = CASES[name]
    return forced(raw, es, FORCED[name])


def bad_rank(k: int) -> tuple:
    """(good, bad, the raw bytes): three segments of ranks below 32, coded at
    ``k`` = 5 in ``good``; in ``bad`` the first code of segment 1 stands for
    rank 256 + 3, as ``q`` = 8 at ``k`` = 5 or ``q`` = 2 at ``k`` = 7. At 5
    that code is the only fault of the container. At 7 no segment is otherwise
    whole (the module docstring): segment 1 is that code and zero bytes up to
    ``seg_len`` = L - 1, so its header fields are sound and its first code is
    the first rule broken."""
    rng = np.random.default_rng(77)
    raw = _uniform(rng, 32, 3 * SEG).tobytes()
    good = forced(raw, 1, [5, 5, 5])
    if k == 5:
        return good, forced(raw, 1, [5, 5, 5], {(1, 0): 256 + 3}), raw
    assert k == 7
    _raw_len, _es, order, segments = read_container(good)
    area = SEG - 1 - HI_FIXED
    ends = [area * (j + 1) // SUBS for j in range(SUBS)]
    first = bytes(sum(bit << i for i, bit in enumerate(_code(256 + 3, 7)[b : b + 8])) for b in (0, 8))
    seg1 = bytes([7]) + struct.pack("<16H", *ends) + first + bytes(area - 2)
    segments = [(True, segments[0][1]), (True, seg1), (True, segments[2][1])]
    return good, write_container(len(raw), 1, order, segments), raw

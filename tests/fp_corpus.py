"""Conformance corpus for the MAFP10 float-plane container (ops/fpcodec.py).

Helpers, not tests: an independent strict decoder written from the format
text in scalar pure Python (it shares no code with ``fpcodec``), named inputs
that drive every path of the encoders, one container assembled by hand that
pins the bit order, and one malformed container per rejection branch.

Format (little-endian; es the element size, m = L // es):
  b"MAFP10" | raw_len u64 | es u8 | reserved u8 | n_seg u32 | order u8[256]
  | seg_len u32[n_seg] | payload
A coded segment: m*(es-1) low bytes, b in 1..7, ceil(m*b/8) code bytes (element
i in bits [i*b, (i+1)*b), LSB first), then the top bytes of the escaped
elements (code 2^b-1) in order. seg_len 0: the L raw bytes.
"""

from __future__ import annotations

import functools
import struct

import numpy as np

SEG = 4096
MiB = 1024 * 1024
HEADER = 6 + 8 + 1 + 1 + 4 + 256


# ---------------------------------------------------------------------------
# the independent strict decoder
# ---------------------------------------------------------------------------


def parse(blob: bytes, raw_len=None):
    """(raw_len, es, order, seg_lens, payload offset); ValueError when the
    header breaks any rule of the format."""
    if len(blob) < HEADER or blob[:6] != b"MAFP10":
        raise ValueError("magic")
    hdr_raw, es, reserved, n_seg = struct.unpack_from("<QBBI", blob, 6)
    if es not in (2, 4):
        raise ValueError("es")
    if reserved != 0:
        raise ValueError("reserved")
    if raw_len is not None and raw_len != hdr_raw:
        raise ValueError("raw_len")
    if n_seg != (hdr_raw + SEG - 1) // SEG:
        raise ValueError("n_seg")
    order = blob[20:276]
    if sorted(order) != list(range(256)):
        raise ValueError("order")
    off = HEADER + 4 * n_seg
    if len(blob) < off:
        raise ValueError("table")
    seg_lens = list(struct.unpack_from(f"<{n_seg}I", blob, HEADER))
    total = 0
    for s, slen in enumerate(seg_lens):
        L = min(SEG, hdr_raw - s * SEG)
        if slen == 0:
            total += L
            continue
        if L % es:
            raise ValueError("coded odd segment")
        lo = (L // es) * (es - 1)
        if not lo + 2 <= slen < L:
            raise ValueError("seg_len")
        total += slen
    if off + total != len(blob):
        raise ValueError("length")
    return hdr_raw, es, order, seg_lens, off


def strict_decode(blob: bytes, raw_len=None) -> bytes:
    hdr_raw, es, order, seg_lens, pos = parse(blob, raw_len)
    out = bytearray()
    for s, slen in enumerate(seg_lens):
        L = min(SEG, hdr_raw - s * SEG)
        if slen == 0:
            out += blob[pos : pos + L]
            pos += L
            continue
        seg = blob[pos : pos + slen]
        pos += slen
        m = L // es
        lo = m * (es - 1)
        b = seg[lo]
        if not 1 <= b <= 7:
            raise ValueError(f"segment {s}: b")
        nbytes = (m * b + 7) // 8
        if lo + 1 + nbytes > slen:
            raise ValueError(f"segment {s}: codes past seg_len")
        stream = int.from_bytes(seg[lo + 1 : lo + 1 + nbytes], "little")
        esc_at = lo + 1 + nbytes
        escape = (1 << b) - 1
        for i in range(m):
            code = (stream >> (i * b)) & escape
            out += seg[i * (es - 1) : (i + 1) * (es - 1)]
            if code == escape:
                if esc_at >= slen:
                    raise ValueError(f"segment {s}: escapes past seg_len")
                out.append(seg[esc_at])
                esc_at += 1
            else:
                out.append(order[code])
        if esc_at != slen:
            raise ValueError(f"segment {s}: escape count")
    return bytes(out)


def segment_offsets(blob: bytes) -> list:
    """Offset in ``blob`` of every segment's payload."""
    hdr_raw, _es, _order, seg_lens, pos = parse(blob)
    offs = []
    for s, slen in enumerate(seg_lens):
        offs.append(pos)
        pos += slen if slen else min(SEG, hdr_raw - s * SEG)
    return offs


def break_segment(blob: bytes, s: int) -> bytes:
    """``blob`` with coded segment ``s`` given the width byte 0: the header
    still validates, a decoder must reject the segment."""
    hdr_raw, es, _order, seg_lens, _off = parse(blob)
    assert seg_lens[s] != 0, "segment is stored raw"
    L = min(SEG, hdr_raw - s * SEG)
    bad = bytearray(blob)
    bad[segment_offsets(blob)[s] + (L // es) * (es - 1)] = 0
    return bytes(bad)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns (uint16), round to nearest even; torch-free."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_gauss(n_bytes: int, seed: int, sigma: float = 1.0) -> bytes:
    rng = np.random.default_rng(seed)
    n = n_bytes // 2
    body = bf16_bits((rng.standard_normal(n) * sigma).astype(np.float32)).tobytes()
    return body + bytes(rng.integers(0, 256, n_bytes - 2 * n, dtype=np.uint8))


def random_bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _with_tops(n_elem: int, es: int, tops: np.ndarray, seed: int) -> bytes:
    """n_elem elements with random low bytes and the given top bytes."""
    data = np.random.default_rng(seed).integers(0, 256, (n_elem, es), dtype=np.uint8)
    data[:, es - 1] = tops
    return data.tobytes()


def _distinct(k: int, es: int) -> bytes:
    """Exactly k distinct top bytes, uniformly spread: codes at width
    log2(k + 1) with no escapes, and every narrower width escapes half."""
    n_elem = 4 * SEG // es
    tops = (np.arange(n_elem) % k) * 2 + 1
    return _with_tops(n_elem, es, tops.astype(np.uint8), seed=100 + k)


def _escapes(es: int) -> bytes:
    """Top byte 0x3F but for a few rare bytes, so b = 1 and the rare ones
    escape: at the first and last element of lanes' runs (a lane owns 32
    elements at es 2, 16 at es 4), then all inside one lane's run, then a
    whole last run, then none."""
    m = SEG // es
    run = m // 64
    tops = np.full((4, m), 0x3F, dtype=np.uint8)
    edge = [0, run - 1, run, 2 * run - 1, 5 * run, 63 * run, m - 1]
    tops[0, edge] = 0x80 + np.arange(len(edge))
    tops[1, 2 * run : 3 * run] = 0x90 + np.arange(run)
    tops[2, m - run :] = 0xC0
    return _with_tops(4 * m, es, tops.reshape(-1), seed=7 + es)


def _random_segment(es: int) -> bytes:
    body = bytearray(bf16_gauss(16 * SEG, seed=31) if es == 2 else fp32_gauss(16 * SEG, seed=32))
    body[5 * SEG : 6 * SEG] = random_bytes(SEG, seed=33)
    return bytes(body)


def fp32_gauss(n_bytes: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    body = rng.standard_normal(n_bytes // 4).astype(np.float32).tobytes()
    return body + bytes(rng.integers(0, 256, n_bytes - len(body), dtype=np.uint8))


def fp16_gauss(n_bytes: int, seed: int) -> bytes:
    return np.random.default_rng(seed).standard_normal(n_bytes // 2).astype(np.float16).tobytes()


TAILS = {2: (2, 126, 128, 130, 4094, 4095), 4: (4, 124, 128, 132, 4092, 4094, 4095)}


@functools.lru_cache(maxsize=None)
def corpus() -> dict:
    """name -> (bytes, es). Built once; nobody changes it."""
    c: dict = {
        "bf16_n01_1m": (bf16_gauss(MiB, seed=1), 2),
        "bf16_n002_1m": (bf16_gauss(MiB, seed=2, sigma=0.02), 2),
        "fp32_n01": (fp32_gauss(256 * 1024, seed=3), 4),
        "fp16_n01": (fp16_gauss(256 * 1024, seed=4), 2),
        "random_es2": (random_bytes(64 * 1024, seed=5), 2),
        "random_es4": (random_bytes(64 * 1024, seed=6), 4),
        "zeros_es2": (bytes(64 * 1024), 2),
        "zeros_es4": (bytes(64 * 1024), 4),
        "constant_bf16": (bf16_bits(np.full(8192, 1.5, dtype=np.float32)).tobytes(), 2),
        "constant_fp32": (np.full(4096, -3.25, dtype=np.float32).tobytes(), 4),
    }
    for k in (1, 3, 7, 15, 31, 63, 127):
        c[f"distinct{k}_es2"] = (_distinct(k, 2), 2)
    c["distinct7_es4"] = (_distinct(7, 4), 4)
    c["distinct127_es4"] = (_distinct(127, 4), 4)
    for es in (2, 4):
        c[f"random_segment_es{es}"] = (_random_segment(es), es)
        c[f"escapes_es{es}"] = (_escapes(es), es)
        gauss = bf16_gauss if es == 2 else fp32_gauss
        for tail in TAILS[es]:
            c[f"tail{tail}_es{es}"] = (gauss(2 * SEG + tail, seed=40 + tail % 37), es)
        c[f"only_tail126_es{es}"] = (gauss(126 if es == 2 else 124, seed=50), es)
    for n_seg, n in ((1, SEG), (4, 4 * SEG), (5, 4 * SEG + 100), (257, MiB + 130)):
        c[f"nseg{n_seg}_es2"] = (bf16_gauss(n, seed=60 + n_seg), 2)
    c["nseg5_es4"] = (fp32_gauss(4 * SEG + 100, seed=70), 4)
    return c


#: the width every full segment of distinct<k> must be coded at
DISTINCT_WIDTH = {1: 1, 3: 2, 7: 3, 15: 4, 31: 5, 63: 6, 127: 7}


# ---------------------------------------------------------------------------
# the hand-assembled container: 64 bf16-sized elements, 128 raw bytes
# ---------------------------------------------------------------------------
#
# Element i is (low byte i, top byte T[i]). Letters: A 0x3F (40 of them),
# B 0x40 (12), C 0xBF (8), D 0x00 (2), E 0xFF (2), so the ranks are A0 B1 C2
# D3 E4 and every other byte follows in ascending order. Costs: b=1 1+8+24,
# b=2 1+16+4 = 21, b=3 1+24+0, so b = 2, codes A=0 B=1 C=2 and D, E escape (3).
HAND_TOPS = (
    "AAAAABAC" "AABAADAC" "AAABAAEC" "ABAAAACA"
    "AABACAAB" "EAABAACA" "ABAADACA" "BAAABCBB"
)
HAND_RAW = bytes(
    x
    for i, t in enumerate(HAND_TOPS)
    for x in (i, {"A": 0x3F, "B": 0x40, "C": 0xBF, "D": 0x00, "E": 0xFF}[t])
)
HAND_CONTAINER = bytes.fromhex(
    "4d4146503130"  # MAFP10
    "8000000000000000"  # raw_len 128
    "02" "00"  # es, reserved
    "01000000"  # n_seg
    # order: the five used bytes by count, then every other byte ascending
    "3f40bf00ff"
    "0102030405060708090a0b0c0d0e0f"
    "101112131415161718191a1b1c1d1e1f"
    "202122232425262728292a2b2c2d2e2f"
    "303132333435363738393a3b3c3d3e"
    "4142434445464748494a4b4c4d4e4f"
    "505152535455565758595a5b5c5d5e5f"
    "606162636465666768696a6b6c6d6e6f"
    "707172737475767778797a7b7c7d7e7f"
    "808182838485868788898a8b8c8d8e8f"
    "909192939495969798999a9b9c9d9e9f"
    "a0a1a2a3a4a5a6a7a8a9aaabacadaeaf"
    "b0b1b2b3b4b5b6b7b8b9babbbcbdbe"
    "c0c1c2c3c4c5c6c7c8c9cacbcccdcecf"
    "d0d1d2d3d4d5d6d7d8d9dadbdcdddedf"
    "e0e1e2e3e4e5e6e7e8e9eaebecedeeef"
    "f0f1f2f3f4f5f6f7f8f9fafbfcfdfe"
    "55000000"  # seg_len 85 = 64 low bytes + 21
    # the 64 low bytes
    "000102030405060708090a0b0c0d0e0f"
    "101112131415161718191a1b1c1d1e1f"
    "202122232425262728292a2b2c2d2e2f"
    "303132333435363738393a3b3c3d3e3f"
    "02"  # b
    # codes, four elements a byte, element 0 in bits 0-1: AAAA -> 00,
    # ABAC -> 0 | 1<<2 | 0 | 2<<6 = 84, ...
    "0084108c40b004201042432004230159"
    "00ffff00"  # escapes in element order: D E E D
)


# ---------------------------------------------------------------------------
# malformed containers
# ---------------------------------------------------------------------------


def _set(blob: bytes, at: int, new: bytes) -> bytes:
    return blob[:at] + new + blob[at + len(new) :]


def malformed() -> list:
    """(name, blob, raw_len given to the reader or None): one container per
    rejection branch of the validator, then of the decoder."""
    good = HAND_CONTAINER
    lo = 64
    seg = HEADER + 4  # the one segment's payload
    # 130 raw bytes of es 4: one segment that is no whole number of elements
    odd = good[:6] + struct.pack("<QBBI", 130, 4, 0, 1) + good[20:276]
    return [
        ("magic", _set(good, 0, b"MALZ41"), None),
        ("short", good[:100], None),
        ("es", _set(good, 14, b"\x03"), None),
        ("reserved", _set(good, 15, b"\x01"), None),
        ("n_seg", _set(good, 16, struct.pack("<I", 2)), None),
        ("order_duplicate", _set(good, 21, b"\x3f"), None),
        ("truncated_table", good[:278], None),
        ("seg_len_low", _set(good, HEADER, struct.pack("<I", lo + 1))[: seg + lo + 1], None),
        ("seg_len_high", _set(good, HEADER, struct.pack("<I", 128)) + bytes(128 - 85), None),
        ("coded_odd_segment", odd + struct.pack("<I", 100) + bytes(100), None),
        ("blob_short", good[:-1], None),
        ("blob_long", good + b"\x00", None),
        ("caller_raw_len", good, 256),
        ("b_zero", _set(good, seg + lo, b"\x00"), None),
        ("b_eight", _set(good, seg + lo, b"\x08"), None),
        # element 0's code 0 -> 3: one escape more than seg_len holds
        ("escape_count_more", _set(good, seg + lo + 1, b"\x03"), None),
        # element 13's code 3 -> 0 (code byte 3: 8c -> 80): one escape fewer
        ("escape_count_fewer", _set(good, seg + lo + 1 + 3, b"\x80"), None),
    ]

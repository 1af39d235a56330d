"""Pure-Python LZ4 block codec (reference implementation for the HIP kernel).

Standard LZ4 block format (token | literals | 2-byte LE offset | extended
lengths). Used to cross-check ops/csrc/lz4.hip on CPU and to decompress
CAS entries on GPU-less machines. Not fast — the GPU kernel is the hot path.

``compress_block`` is an exact model of the kernel's ``lz4_compress_segment``
(same 7-bit hash, same skip through miss runs, same emit order, same slot
bail-out), so a test can hold every byte the kernel emits to it.
``decompress_block`` bounds every read and raises ``ValueError`` on anything
the kernel's ``lz4_decompress_segment`` rejects.
"""

from __future__ import annotations

from typing import Optional

MIN_MATCH = 4
MFLIMIT = 12
LASTLITERALS = 5
HASH_BITS = 7


def _hash(v: int) -> int:
    return ((v * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def _ext_len(n: int) -> bytes:
    """Length-extension bytes of a token nibble that saturated (n >= 15)."""
    rest = n - 15
    return b"\xff" * (rest // 255) + bytes([rest % 255])


def compress_block(src: bytes, accel: bool = True, max_out: Optional[int] = None) -> bytes:
    """Greedy LZ4 block compression, the kernel's parser step for step.

    ``accel`` is the kernel's skip through matchless regions: after ``m``
    consecutive misses the next probe is ``1 + (m >> 6)`` bytes on. With
    ``accel=False`` every position is probed (a slightly denser parse the
    kernel never produces). ``max_out`` is the kernel's output slot: where
    the kernel gives up (``return 0``) this returns ``b""``."""
    n = len(src)
    out = bytearray()
    table: dict[int, int] = {}
    ip = 0
    anchor = 0
    misses = 0
    mflimit = n - MFLIMIT

    if n >= MIN_MATCH + LASTLITERALS:
        while ip < mflimit:
            seq = src[ip : ip + 4]
            h = _hash(int.from_bytes(seq, "little"))
            cand = table.get(h, -1)
            table[h] = ip
            if 0 <= cand < ip and ip - cand <= 0xFFFF and src[cand : cand + 4] == seq:
                misses = 0
                mlen = MIN_MATCH
                maxm = n - LASTLITERALS - ip
                while mlen < maxm and src[cand + mlen] == src[ip + mlen]:
                    mlen += 1
                lit, ml = ip - anchor, mlen - MIN_MATCH
                if max_out is not None:
                    # the kernel's own (slightly generous) size estimate
                    need = 1 + (1 + lit // 255 if lit >= 15 else 0) + lit + 2
                    need += 1 + ml // 255 if ml >= 15 else 0
                    if len(out) + need + 8 > max_out:
                        return b""
                out.append((min(lit, 15) << 4) | min(ml, 15))
                if lit >= 15:
                    out += _ext_len(lit)
                out += src[anchor:ip]
                off = ip - cand
                out.append(off & 0xFF)
                out.append(off >> 8)
                if ml >= 15:
                    out += _ext_len(ml)
                ip += mlen
                anchor = ip
            else:
                ip += 1 + (misses >> 6) if accel else 1
                misses += 1
    lit = n - anchor
    if max_out is not None:
        need = 1 + (1 + lit // 255 if lit >= 15 else 0) + lit
        if len(out) + need > max_out:
            return b""
    out.append(min(lit, 15) << 4)
    if lit >= 15:
        out += _ext_len(lit)
    out += src[anchor:]
    return bytes(out)


def decompress_block(comp: bytes, raw_len: int) -> bytes:
    """Standard LZ4 block decompression into exactly ``raw_len`` bytes.
    Every read is bounded; a malformed block raises ``ValueError``."""
    out = bytearray()
    ip = 0
    n = len(comp)

    def run_length(ip: int, base: int) -> tuple[int, int]:
        while True:
            if ip >= n:
                raise ValueError("LZ4: length run past the end of the block")
            b = comp[ip]
            ip += 1
            base += b
            if b != 255:
                return ip, base

    while ip < n:
        token = comp[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            ip, lit = run_length(ip, lit)
        if ip + lit > n:
            raise ValueError("LZ4: literals past the end of the block")
        if len(out) + lit > raw_len:
            raise ValueError(f"LZ4: literals past the {raw_len} raw bytes")
        out += comp[ip : ip + lit]
        ip += lit
        if ip >= n:
            break
        if ip + 2 > n:
            raise ValueError("LZ4: truncated offset")
        off = comp[ip] | (comp[ip + 1] << 8)
        ip += 2
        if off == 0 or off > len(out):
            raise ValueError("LZ4: bad offset")
        mlen = token & 0xF
        if mlen == 15:
            ip, mlen = run_length(ip, mlen)
        mlen += MIN_MATCH
        if len(out) + mlen > raw_len:
            raise ValueError(f"LZ4: match past the {raw_len} raw bytes")
        start = len(out) - off
        for i in range(mlen):  # overlap-safe forward copy
            out.append(out[start + i])
    if len(out) != raw_len:
        raise ValueError(f"LZ4: expected {raw_len} bytes, got {len(out)}")
    return bytes(out)

"""Conformance corpus for the LZ4 segment codec (ops/csrc/lz4.hip, the C++
core and utils/lz4ref.py). A plain helper module, written from the LZ4 block
format: pure Python + numpy, deterministic, reads nothing from disk.

  ``model_compress``  the exact model of the kernel's compressor
  ``strict_decode``   an independent decoder that also enforces the format's
                      end-of-block rules
  ``SEGMENTS``        named 4096-byte compressor inputs
  ``WELL_FORMED``     hand-assembled blocks with the bytes they decode to
  ``MALFORMED``       one block per rejection branch of a decoder

Block format, per sequence: token (literal length << 4 | match length - 4),
a 255-run extending a literal length of 15, the literals, a 2-byte LE offset,
a 255-run extending a match nibble of 15. The last sequence stops after its
literals.
"""

from __future__ import annotations

from typing import Optional

import numpy as np

from modal_amd.utils import lz4ref

SEG = 4096
SHORT_LENGTHS = (1, 4, 8, 9, 12, 13, 14, 16, 17, 100, 4095)


def model_compress(seg: bytes, max_out: Optional[int] = None) -> bytes:
    """What ``lz4_compress_segment`` emits for ``seg``, byte for byte: 7-bit
    hash, skip through miss runs, the ``cand < ip`` rule, the kernel's emit
    order. With ``max_out`` (the slot size), ``b""`` where the kernel bails
    out with 0."""
    return lz4ref.compress_block(bytes(seg), accel=True, max_out=max_out)


def strict_decode(block: bytes, raw_len: int) -> bytes:
    """Decode one LZ4 block to exactly ``raw_len`` bytes, enforcing the end
    rules on top of the bounds: where the block holds a match, its last
    sequence carries at least 5 literals and its last match starts at least
    12 bytes before the end. ``ValueError`` on anything else."""
    block = bytes(block)
    out = bytearray()
    pos = 0
    last_match_start = -1
    last_literals = 0

    def take(count: int) -> bytes:
        nonlocal pos
        if count < 0 or pos + count > len(block):
            raise ValueError(f"block ends inside a field at byte {pos}")
        piece = block[pos : pos + count]
        pos += count
        return piece

    def length(nibble: int) -> int:
        if nibble < 15:
            return nibble
        total = 15
        while True:
            byte = take(1)[0]
            total += byte
            if byte != 255:
                return total

    if not block:
        raise ValueError("empty block")
    while True:
        token = take(1)[0]
        last_literals = length(token >> 4)
        out += take(last_literals)
        if len(out) > raw_len:
            raise ValueError("literals overrun the destination")
        if pos == len(block):
            break
        offset = int.from_bytes(take(2), "little")
        if offset == 0 or offset > len(out):
            raise ValueError(f"offset {offset} at output position {len(out)}")
        mlen = length(token & 15) + 4
        if len(out) + mlen > raw_len:
            raise ValueError("match overruns the destination")
        last_match_start = len(out)
        for _ in range(mlen):
            out.append(out[-offset])
        if pos == len(block):
            raise ValueError("block ends on a match")
    if len(out) != raw_len:
        raise ValueError(f"decoded {len(out)} bytes, expected {raw_len}")
    if last_match_start >= 0:
        if last_literals < 5:
            raise ValueError(f"last sequence has {last_literals} literals")
        if last_match_start > raw_len - 12:
            raise ValueError("last match starts inside the final 12 bytes")
    return bytes(out)


# ---------------------------------------------------------------------------
# compressor inputs
# ---------------------------------------------------------------------------


def _rand(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _tile(unit: bytes, n: int = SEG) -> bytes:
    return (unit * (n // len(unit) + 1))[:n]


def _planted_repeats(seed: int) -> bytes:
    """Random bytes with about 40 earlier runs of 4..40 bytes copied forward."""
    rng = np.random.default_rng(seed)
    buf = bytearray(_rand(SEG, seed + 1))
    for _ in range(40):
        run = int(rng.integers(4, 41))
        dst = int(rng.integers(run + 1, SEG - run))
        src = int(rng.integers(max(0, dst - 300), dst - run + 1))
        buf[dst : dst + run] = buf[src : src + run]
    return bytes(buf)


def _ascii_text(seed: int) -> bytes:
    words = (
        b"snapshot block volume segment worker restore digest kernel stream "
        b"container payload offset literal match token the of and to in"
    ).split()
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < SEG:
        out += words[int(rng.integers(len(words)))]
        out += b"\n" if rng.random() < 0.1 else b" "
    return bytes(out[:SEG])


def _match_to_len_minus_5() -> bytes:
    """A 64-byte unit repeated up to byte ``SEG - 5``, then five bytes that
    break the period: the one long match ends exactly where the format's
    last-literals rule would cut it."""
    unit = _rand(64, 77)
    body = bytearray(_tile(unit, SEG))
    for i in range(SEG - 5, SEG):
        body[i] ^= 0xFF
    return bytes(body)


def _segments() -> dict:
    segs = {
        "zeros": bytes(SEG),
        "random": _rand(SEG, 1),
        "alphabet3": bytes(np.random.default_rng(2).integers(0, 3, SEG, dtype=np.uint8)),
    }
    for p in range(1, 18):
        segs[f"period{p}"] = _tile(_rand(p, 100 + p))
    segs["tiled_1k"] = _tile(_rand(1024, 3))
    segs["random_then_zeros"] = _rand(2048, 4) + bytes(2048)
    segs["zeros_then_random"] = bytes(2048) + _rand(2048, 5)
    segs["planted_repeats"] = _planted_repeats(6)
    segs["ascii_text"] = _ascii_text(7)
    segs["match_to_len_minus_5"] = _match_to_len_minus_5()
    assert all(len(s) == SEG for s in segs.values())
    return segs


SEGMENTS = _segments()


def variant(i: int) -> bytes:
    """The i-th of an endless family of distinct compressible 4096-byte
    segments (small alphabets, tiled units, text, zeros then text), to fill a
    launch up."""
    kind = i % 4
    if kind == 0:
        alphabet = 2 + i % 7
        return bytes(np.random.default_rng(1000 + i).integers(0, alphabet, SEG, dtype=np.uint8))
    if kind == 1:
        return _tile(_rand(24 + 5 * (i % 50), 2000 + i))
    if kind == 2:
        return _ascii_text(3000 + i)
    zeros = (37 * i) % 2000
    return bytes(zeros) + _ascii_text(4000 + i)[: SEG - zeros]


# ---------------------------------------------------------------------------
# hand-assembled blocks
# ---------------------------------------------------------------------------


def _length_run(n: int) -> bytes:
    rest = n - 15
    return b"\xff" * (rest // 255) + bytes([rest % 255])


class Block:
    """Sequence builder: keeps the encoded block and, separately, the bytes
    it must decode to (a match copies byte by byte from ``offset`` back)."""

    def __init__(self, seed: int) -> None:
        self.enc = bytearray()
        self.raw = bytearray()
        self._rng = np.random.default_rng(seed)

    def literals(self, n: int) -> bytes:
        return self._rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def seq(self, lits: "bytes | int", offset: Optional[int] = None, mlen: int = 0) -> "Block":
        """One sequence: literals (bytes, or a count of random ones), then a
        match of ``mlen`` bytes at ``offset``; no match when offset is None.
        Nothing is checked here, so malformed sequences can be built too."""
        if isinstance(lits, int):
            lits = self.literals(lits)
        token = min(len(lits), 15) << 4
        if offset is not None:
            token |= min(mlen - 4, 15)
        self.enc.append(token)
        if len(lits) >= 15:
            self.enc += _length_run(len(lits))
        self.enc += lits
        self.raw += lits
        if offset is not None:
            self.enc += offset.to_bytes(2, "little")
            if mlen - 4 >= 15:
                self.enc += _length_run(mlen - 4)
            if 0 < offset <= len(self.raw):
                for _ in range(mlen):
                    self.raw.append(self.raw[-offset])
        return self

    def pad(self, total: int = SEG) -> "Block":
        """Close with a literal run up to ``total`` decoded bytes."""
        return self.seq(total - len(self.raw))

    def done(self) -> tuple:
        return bytes(self.enc), bytes(self.raw)


def _shrink(b: Block) -> Block:
    """A long match up front, so that the finished block is shorter than its
    4096 raw bytes and a container can carry it."""
    return b.seq(32, 32, 2000)


def _well_formed() -> dict:
    out = {}
    seed = 500

    def new() -> Block:
        nonlocal seed
        seed += 1
        return _shrink(Block(seed))

    # every offset of the byte-wise overlap copy, the first 8-byte copy, 9, 16
    for off in (1, 2, 3, 4, 5, 6, 7, 8, 9, 16):
        out[f"offset{off}"] = new().seq(7, off, 61).seq(3, off, 8).pad().done()
    # offset == output position: the match starts at the block's first byte
    b = Block(600).seq(40, 40, 3000)
    out["offset_is_position"] = b.pad().done()
    b = new()
    out["offset_is_position_late"] = b.seq(9, len(b.raw) + 9, 100).pad().done()
    # match lengths either side of the nibble and of the first 255 run
    for mlen in (4, 18, 19, 273, 274):
        out[f"match{mlen}"] = new().seq(6, 5, mlen).seq(2, 11, mlen).pad().done()
    # literal lengths likewise, and a sequence with none
    for lit in (0, 14, 15, 16, 269, 270, 271):
        out[f"literals{lit}"] = new().seq(lit, 3, 12).seq(lit, 24, 5).pad().done()
    # a block whose last sequence is a match landing exactly on byte 4096:
    # the end rules forbid it, every decoder here accepts it
    b = new().seq(20, 13, 40)
    out["ends_on_match"] = b.seq(6, 9, SEG - len(b.raw) - 6).done()
    for name, (enc, raw) in out.items():
        assert len(raw) == SEG and 0 < len(enc) < SEG, name
    # a literals-only block is longer than what it decodes to, and a container
    # bounds comp_len below 4096: it can only be a short last segment
    out["literals_only"] = Block(700).seq(4000).done()
    return out


WELL_FORMED = _well_formed()

#: names whose block breaks an end-of-block rule (strict_decode refuses them)
BREAKS_END_RULES = ("ends_on_match",)

#: the literals-only block at full segment size: 4114 bytes for 4096, so no
#: container can carry it; only a direct kernel launch sees it
LITERALS_ONLY_FULL = Block(701).seq(SEG).done()


def _malformed() -> dict:
    """name -> (block, raw length of its segment). Each is well formed up to
    the one field that a decoder has to refuse."""
    out = {}

    def lead(seed: int) -> Block:  # 64 good bytes first
        return Block(seed).seq(16, 16, 48)

    # F0 FF FF: the literal-length run never ends
    out["literal_run_off_end"] = (bytes(lead(801).enc) + b"\xf0\xff\xff", SEG)
    # 12 literals announced, 3 present
    out["literals_overrun_source"] = (bytes(lead(802).enc) + b"\xc0abc", SEG)
    # 4086 good bytes, then 11 literals
    b = Block(803).seq(16, 16, 4070).seq(11)
    out["literals_overrun_destination"] = (bytes(b.enc), SEG)
    # one byte where the 2-byte offset belongs
    out["truncated_offset"] = (bytes(lead(804).seq(8).enc) + b"\x01", SEG)
    out["offset_zero"] = (bytes(lead(805).seq(4, 0, 8).seq(11).enc), SEG)
    # 64 + 4 bytes out, offset 69
    out["offset_past_start"] = (bytes(lead(806).seq(4, 69, 8).seq(11).enc), SEG)
    # zero literals, so the match sits at output position 0
    out["match_at_position_0"] = (bytes(Block(807).seq(0, 1, 8).seq(11).enc), SEG)
    # 4F .. offset FF FF: the match-length run never ends
    out["match_run_off_end"] = (bytes(lead(808).enc) + b"\x4fwxyz\x04\x00\xff\xff", SEG)
    # 16 + 4081 = 4097
    out["match_overruns_destination_by_1"] = (bytes(Block(809).seq(16, 16, 4081).enc), SEG)
    # a valid stream of 4095 bytes
    b = Block(810).seq(16, 16, 4068).seq(11)
    assert len(b.raw) == SEG - 1 and strict_decode(b.enc, SEG - 1) == bytes(b.raw)
    out["one_byte_short"] = (bytes(b.enc), SEG)
    # a valid stream of 101 bytes in a last segment of 100
    b = Block(811).seq(10, 10, 80).seq(11)
    assert len(b.raw) == 101 and strict_decode(b.enc, 101) == bytes(b.raw)
    out["short_segment_one_byte_over"] = (bytes(b.enc), 100)
    for name, (enc, raw_len) in out.items():
        assert 0 < len(enc) < SEG, name
    return out


MALFORMED = _malformed()

"""Corpus for the content-digest path (ops/csrc/sha256.hip, ops/hashing.py,
ops/pipeline.py) and the segment copy kernel (ops/csrc/pack.hip). A plain
helper module: numpy, hashlib and the host references only, deterministic,
reads nothing from disk, never touches a GPU.

  ``sha_edge_lengths``   message lengths either side of every SHA-256 padding
                         edge and of a tree leaf
  ``layout``             messages placed in one byte array at chosen
                         residues mod 16, never sharing a 16-byte packet
  ``tree_input``         random bytes whose full leaves are pairwise distinct
  ``pipeline_blocks``    the blocks of the batch and pipelined digest tests
  ``expected_digest``    hashlib below the threshold, the host tree above
  ``expected_container`` the MALZ41 container from the compressor's model
  ``unpack_tables``      scatter tables: every source x destination residue

Every input that stands for more than one leaf has pairwise distinct full
leaves (asserted where it is built): with equal leaves a kernel that hashed
leaf i from the wrong offset, or stored two lanes' digests crosswise, would
still give the right root.
"""

from __future__ import annotations

import functools
import hashlib
from typing import NamedTuple, Optional, Sequence

import numpy as np

import lz4_corpus
from modal_amd.ops.compress import SEG_SIZE, _header, effective_lens, worth_keeping
from modal_amd.ops.hashing import LEAF_SIZE, tree_sha256_cpu

CANARY = 0xA5
WINDOW = 64 * 1024  # the pipelined test's window
THRESHOLD = 2 * LEAF_SIZE  # and its plain/tree digest threshold


def rand_bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def full_leaves(data: bytes) -> list:
    return [data[o : o + LEAF_SIZE] for o in range(0, len(data) - LEAF_SIZE + 1, LEAF_SIZE)]


def assert_distinct_full_leaves(data: bytes, what: str = "input") -> None:
    leaves = full_leaves(data)
    assert len(set(leaves)) == len(leaves), f"{what}: two full leaves are equal"


# ---------------------------------------------------------------------------
# SHA-256 messages
# ---------------------------------------------------------------------------


def sha_edge_lengths() -> tuple:
    """0 and 1; 55/56 and 119/120, where ``rem + 9 <= 64`` flips between one
    padding chunk and two; the chunk edges 64 and 128; and a tree leaf."""
    near = (0, 1, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 121, 127, 128, 129)
    return near + (LEAF_SIZE - 1, LEAF_SIZE, LEAF_SIZE + 1)


class Layout(NamedTuple):
    data: np.ndarray  # uint8, random throughout, the gaps included
    offsets: list
    lengths: list

    def message(self, i: int) -> bytes:
        return self.data[self.offsets[i] : self.offsets[i] + self.lengths[i]].tobytes()


def layout(lengths: Sequence[int], residues: Sequence[int], seed: int = 0) -> Layout:
    """One byte array with message i at an offset that is ``residues[i]`` mod
    16. A message starts in the 16-byte packet after the one its predecessor
    ended in (or later), so at least one unused byte lies between two, and no
    two share a packet. The array is taken to start 16-aligned on the device
    (the GPU tests assert it)."""
    assert len(lengths) == len(residues)
    offsets, cursor = [], 0
    for n, r in zip(lengths, residues):
        start = -(-(cursor + 1) // 16) * 16 + r % 16
        offsets.append(start)
        cursor = start + n
    data = np.random.default_rng(seed).integers(0, 256, cursor + 64, dtype=np.uint8)
    out = Layout(data, offsets, [int(n) for n in lengths])
    check_layout(out, residues)
    return out


def check_layout(lay: Layout, residues: Sequence[int]) -> None:
    assert [o % 16 for o in lay.offsets] == [r % 16 for r in residues]
    ends = [o + n for o, n in zip(lay.offsets, lay.lengths)]
    for end, start in zip(ends, lay.offsets[1:]):
        assert start > end, "no unused byte between two messages"
        assert start // 16 > max(end - 1, 0) // 16 or end == 0, "two messages share a packet"
    assert ends[-1] <= len(lay.data)


def edge_cases() -> tuple:
    """(lengths, residues): every edge length at every residue, 19 x 16."""
    pairs = [(n, r) for r in range(16) for n in sha_edge_lengths()]
    return [n for n, _r in pairs], [r for _n, r in pairs]


def pair_position_lists() -> dict:
    """Length lists for the pair kernel: with the list as given, reversed,
    and shifted by a leading empty message, every edge length sits in an A
    slot (even index) and in a B slot (odd). The two alternating lists leave
    one chain of a lane with ~128 chunks to hash alone, A-only or B-only."""
    edges = list(sha_edge_lengths())
    long = LEAF_SIZE + 1
    return {
        "edges": edges,
        "reversed": edges[::-1],
        "shifted": [0] + edges,
        "empty_then_long": [0, long] * 3,
        "long_then_empty": [long, 0] * 3,
    }


def slots_of(lists: dict) -> tuple:
    """(lengths seen in an A slot, lengths seen in a B slot)."""
    a = {n for ls in lists.values() for n in ls[0::2]}
    b = {n for ls in lists.values() for n in ls[1::2]}
    return a, b


def grid_messages(n: int) -> Layout:
    """n messages back to back, message i of ``i % 131`` bytes."""
    lengths = [i % 131 for i in range(n)]
    offsets = (np.cumsum(lengths) - lengths).tolist()
    data = np.random.default_rng(31).integers(0, 256, sum(lengths) + 64, dtype=np.uint8)
    return Layout(data, offsets, lengths)


def arbitrary_table(size: int = 40_000) -> Layout:
    """Spans in no order: decreasing offsets, overlaps, one inside another,
    the same span twice (rows 1 and 6) and three times empty."""
    spans = [
        (30_000, 8193), (17, 120), (29_999, 56), (12_000, 20_000), (12_001, 55),
        (0, 64), (17, 120), (39_936, 64), (5, 0), (5, 0), (16, 119), (0, 0),
    ]
    assert all(o + n <= size for o, n in spans)
    data = np.random.default_rng(41).integers(0, 256, size, dtype=np.uint8)
    return Layout(data, [o for o, _n in spans], [n for _o, n in spans])


def sha_digests(lay: Layout) -> list:
    return [hashlib.sha256(lay.message(i)).digest() for i in range(len(lay.offsets))]


# ---------------------------------------------------------------------------
# far offsets: regions of one 2**32 + 2**20 byte device tensor
# ---------------------------------------------------------------------------

FAR_BYTES = 2**32 + 2**20
FAR_HALF = 16 * 1024  # a region is [edge - FAR_HALF, edge + FAR_HALF)
FAR_EDGES = (2**31, 2**32)
FAR_SHA_LENGTHS = (55, 64, LEAF_SIZE, LEAF_SIZE + 1)
FAR_SEGMENT_LENGTHS = (1, 17, 4096, 65537)


def far_region(edge: int) -> np.ndarray:
    return np.random.default_rng(edge % 1009).integers(0, 256, 2 * FAR_HALF, dtype=np.uint8)


def far_messages() -> list:
    """(absolute offset, length) of messages ending just below each edge,
    straddling it, and starting just above 2**32; starts at mixed residues."""
    spans = []
    for k, n in enumerate(FAR_SHA_LENGTHS):
        for edge in FAR_EDGES:
            spans.append((edge - n - k, n))  # ends k bytes below the edge
            spans.append((edge - n // 2 - 3 * k, n))  # straddles it
        spans.append((2**32 + 1 + 5 * k, n))
    for off, n in spans:
        assert any(e - FAR_HALF <= off and off + n <= e + FAR_HALF for e in FAR_EDGES)
    assert any(o + n <= 2**31 for o, n in spans) and any(o < 2**31 < o + n for o, n in spans)
    assert any(2**31 < o and o + n <= 2**32 for o, n in spans)
    assert any(o < 2**32 < o + n for o, n in spans) and any(o > 2**32 for o, n in spans)
    return spans


FAR_NEAR = 128 * 1024  # segments lie in [edge - FAR_NEAR, edge + FAR_NEAR)


def far_destinations() -> list:
    """Three scatter tables [(absolute offset, length)] of the segments of
    FAR_SEGMENT_LENGTHS, in that order. Over the three, each edge has a
    segment that ends within 64 bytes below it and segments that straddle
    it, the 65537-byte one among them; segments of a table keep GAP apart."""
    a, b, c, d = FAR_SEGMENT_LENGTHS
    lo, hi = FAR_EDGES
    tables = [
        [(lo - 40, a), (lo - 9, b), (hi - c - 3, c), (hi + 21, d)],
        [(hi - 40_001 - 20, a), (lo - 1001 - 16 - b, b), (lo - 1001, c), (hi - 40_001, d)],
        [(hi - 100, a), (hi - 5 - 16 - b, b), (hi - 5, c), (lo - 65_530, d)],
    ]
    spans = [s for t in tables for s in t]
    for edge in FAR_EDGES:
        assert any(0 <= edge - (o + n) < 64 for o, n in spans), "nothing ends just below"
        assert any(o < edge < o + n for o, n in spans if n == d), "the long one never straddles"
        assert sum(o < edge < o + n for o, n in spans) >= 2
    for t in tables:
        assert [n for _o, n in t] == list(FAR_SEGMENT_LENGTHS)
        ordered = sorted(t)
        for (o0, n0), (o1, _n1) in zip(ordered, ordered[1:]):
            assert o1 - (o0 + n0) >= GAP
        for o, n in t:
            assert any(e - FAR_NEAR + GAP <= o and o + n + GAP <= e + FAR_NEAR for e in FAR_EDGES)
    assert max(FAR_EDGES) + FAR_NEAR <= FAR_BYTES
    return tables


def far_image(table: list, packed: np.ndarray, edge: int) -> np.ndarray:
    """The bytes of [edge - FAR_NEAR, edge + FAR_NEAR) after ``table``'s
    scatter of ``packed`` into canary."""
    img = np.full(2 * FAR_NEAR, CANARY, dtype=np.uint8)
    base, pos = edge - FAR_NEAR, 0
    for o, n in table:
        if base <= o < base + 2 * FAR_NEAR:
            img[o - base : o - base + n] = packed[pos : pos + n]
        pos += n
    return img


# ---------------------------------------------------------------------------
# tree, batch and pipelined digests
# ---------------------------------------------------------------------------


def tree_sizes() -> tuple:
    """One leaf and less, and leaf counts either side of one and two
    256-lane workgroups, with and without a short last leaf."""
    L = LEAF_SIZE
    return (1, L - 1, L, L + 1, 255 * L, 256 * L, 256 * L + 1, 257 * L + L - 1, 513 * L + 7)


@functools.lru_cache(maxsize=None)
def tree_input(size: int) -> bytes:
    data = rand_bytes(size, 7000 + size % 997)
    assert_distinct_full_leaves(data, f"tree input of {size} bytes")
    return data


def swap_leaves(data: bytes, i: int, j: int) -> bytes:
    """``data`` with full leaves i and j exchanged."""
    L = LEAF_SIZE
    buf = bytearray(data)
    buf[i * L : (i + 1) * L], buf[j * L : (j + 1) * L] = data[j * L : (j + 1) * L], data[i * L : (i + 1) * L]
    return bytes(buf)


PIPELINE_SIZES = (0, 1, 4095, 4096, 4097, 8192, 16383, 16384, 16385, 40000, 65536, 65537, 100000, 0, 24576)


@functools.lru_cache(maxsize=None)
def pipeline_blocks() -> tuple:
    """Blocks of PIPELINE_SIZES: block k random when ``k % 3 == 0``, else
    compressible variants from lz4_corpus, no variant used twice. Read-only."""
    blocks, next_variant = [], 0
    for k, size in enumerate(PIPELINE_SIZES):
        if k % 3 == 0:
            block = rand_bytes(size, 9000 + k)
        else:
            n_seg = -(-size // lz4_corpus.SEG)
            segs = [lz4_corpus.variant(next_variant + s) for s in range(n_seg)]
            next_variant += n_seg
            block = b"".join(segs)[:size]
        assert len(block) == size
        assert_distinct_full_leaves(block, f"pipeline block {k}")
        blocks.append(block)
    return tuple(blocks)


def expected_digest(block: bytes, threshold: int) -> str:
    if len(block) < threshold:
        return hashlib.sha256(block).hexdigest()
    return tree_sha256_cpu(block).hex()


@functools.lru_cache(maxsize=None)
def expected_container(block: bytes) -> Optional[bytes]:
    """The MALZ41 container of ``block`` from the compressor's exact model,
    None where the keep rule drops it."""
    if not block:
        return None
    segs = [block[o : o + SEG_SIZE] for o in range(0, len(block), SEG_SIZE)]
    models = [lz4_corpus.model_compress(seg) for seg in segs]
    comp_lens = [len(m) if 0 < len(m) < len(seg) else 0 for seg, m in zip(segs, models)]
    eff = effective_lens(np.array(comp_lens, dtype=np.int32), len(block))
    if not worth_keeping(int(eff.sum()), len(block)):
        return None
    parts = [m if c else seg for seg, m, c in zip(segs, models, comp_lens)]
    return _header(len(block), comp_lens) + b"".join(parts)


def window_partition(sizes: Sequence[int], window: int) -> list:
    """Consecutive blocks, each rounded up to the larger of a segment and a
    leaf, up to ``window`` bytes; a block larger than that stands alone."""
    align = max(SEG_SIZE, LEAF_SIZE)
    windows, cur, cur_bytes = [], [], 0
    for i, size in enumerate(sizes):
        nb = -(-size // align) * align
        if cur and cur_bytes + nb > window:
            windows.append(cur)
            cur, cur_bytes = [], 0
        cur.append(i)
        cur_bytes += nb
    if cur:
        windows.append(cur)
    return windows


# ---------------------------------------------------------------------------
# segment pack / unpack
# ---------------------------------------------------------------------------

TILE = 64 * 1024  # pack.hip's TILE_BYTES
GAP = 16  # canary bytes at least, either side of every destination segment
SMALL_LENGTHS = (0, 1, 3, 15, 16, 17, 31, 32, 33)
TILE_LENGTHS = (TILE - 1, TILE, TILE + 1)
TILE_RESIDUES = (0, 1, 15)


class ScatterTable(NamedTuple):
    """Segments packed back to back in ``packed`` and their places in a
    destination of ``dst_size`` bytes. ``cases`` names the (source residue,
    destination residue, length) a segment is there for, None for a filler
    that only shifts the packed cursor."""

    packed: np.ndarray
    lengths: list
    dst_offsets: list
    dst_size: int
    cases: list

    def src_offsets(self) -> list:
        return (np.cumsum(self.lengths) - self.lengths).astype(np.int64).tolist()

    def image(self) -> np.ndarray:
        """What the destination must hold after the scatter."""
        img = np.full(self.dst_size, CANARY, dtype=np.uint8)
        for s, d, n in zip(self.src_offsets(), self.dst_offsets, self.lengths):
            img[d : d + n] = self.packed[s : s + n]
        return img


def scatter_table(lengths: Sequence[int], dst_residues: Sequence[int], cases: list, seed: int,
                  gap: int = GAP) -> ScatterTable:
    """Destination i starts ``dst_residues[i]`` mod 16, at least ``gap``
    bytes after its predecessor's end and after the buffer's start; ``gap``
    more follow the last one."""
    dst_offsets, cursor = [], 0
    for n, r in zip(lengths, dst_residues):
        start = -(-(cursor + gap) // 16) * 16 + r % 16
        dst_offsets.append(start)
        cursor = start + n
    packed = np.random.default_rng(seed).integers(0, 256, max(sum(lengths), 1), dtype=np.uint8)
    return ScatterTable(packed, [int(n) for n in lengths], dst_offsets, cursor + gap + 16, cases)


def check_gaps(table: ScatterTable, gap: int = GAP) -> None:
    """Segments in increasing order, disjoint, ``gap`` bytes clear around each."""
    end = 0
    for d, n in zip(table.dst_offsets, table.lengths):
        assert d - end >= gap, f"gap of {d - end} bytes before the segment at {d}"
        end = d + n
    assert table.dst_size - end >= gap


def _residue_table(wanted: list, seed: int, gap: int = GAP) -> ScatterTable:
    """A table that holds every (rs, rd, length) of ``wanted``: before each, a
    filler segment of 1..15 bytes brings the packed cursor to ``rs`` mod 16."""
    lengths, residues, cases, cursor = [], [], [], 0
    for k, (rs, rd, n) in enumerate(wanted):
        filler = (rs - cursor) % 16
        if filler:
            lengths.append(filler)
            residues.append((7 * k + 3) % 16)
            cases.append(None)
            cursor += filler
        lengths.append(n)
        residues.append(rd)
        cases.append((rs, rd, n))
        cursor += n
    return scatter_table(lengths, residues, cases, seed, gap)


@functools.lru_cache(maxsize=None)
def unpack_tables(gap: int = GAP) -> tuple:
    """One table per length below 64 with all 256 residue pairs, and one with
    the tile-edge lengths at residues 0, 1 and 15 on either side."""
    tables = []
    for i, n in enumerate(SMALL_LENGTHS):
        wanted = [(rs, rd, n) for rd in range(16) for rs in range(16)]
        tables.append(_residue_table(wanted, 100 + i, gap))
    wanted = [(rs, rd, n) for n in TILE_LENGTHS for rd in TILE_RESIDUES for rs in TILE_RESIDUES]
    tables.append(_residue_table(wanted, 200, gap))
    return tuple(tables)


def check_unpack_coverage(tables: Sequence[ScatterTable], gap: int = GAP) -> None:
    seen = set()
    for t in tables:
        assert 0 < len(t.lengths) < 1024
        check_gaps(t, gap)
        for s, d, n, case in zip(t.src_offsets(), t.dst_offsets, t.lengths, t.cases):
            seen.add((s % 16, d % 16, n))
            assert case is None or case == (s % 16, d % 16, n)
    for n in SMALL_LENGTHS:
        missing = [(rs, rd) for rs in range(16) for rd in range(16) if (rs, rd, n) not in seen]
        assert not missing, f"length {n}: residue pairs {missing[:4]} are missing"
    for n in TILE_LENGTHS:
        for rs in TILE_RESIDUES:
            for rd in TILE_RESIDUES:
                assert (rs, rd, n) in seen, (rs, rd, n)


def blocks_per_segment(n: int, max_len: int) -> int:
    """pack.hip's launch_segcopy: one block per segment from 1024 segments
    on; below, about 2048 blocks in all but no more than the longest
    segment's tiles."""
    if n >= 1024:
        return 1
    tiles = -(-max_len // TILE)
    want = -(-2048 // n)
    return max(1, min(tiles, want))


def many_segments_table() -> ScatterTable:
    """1500 segments of ``i % 97`` bytes, two of them 200 000: one block per
    segment, which walks four tiles."""
    lengths = [i % 97 for i in range(1500)]
    lengths[3] = lengths[1402] = 200_000
    residues = [(5 * i + 1) % 16 for i in range(1500)]
    return scatter_table(lengths, residues, [None] * 1500, 300)


def strided_table() -> ScatterTable:
    """1023 segments of 1..64 bytes and one of 300 000: five tiles over
    three blocks."""
    lengths = [1 + i % 64 for i in range(1023)]
    lengths[511] = 300_000
    residues = [(3 * i + 2) % 16 for i in range(1023)]
    return scatter_table(lengths, residues, [None] * 1023, 301)

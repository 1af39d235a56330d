"""Inputs of the wavefront LZ4 encoder's tests. A plain helper module."""

from __future__ import annotations

import functools

import numpy as np

from lz4_corpus import SEG, SEGMENTS
from modal_amd.utils import lz4ref

LENGTHS = (1, 8, 12, 13, 17, 4095, 4096)

#: two 4-byte sequences whose 12-bit hash is 1633, found once by a CPU search
COLLIDE_A, COLLIDE_B = b"A\x00\x00Z", b"A\x97\tZ"


def _collide() -> bytes:
    """The pair planted 100 apart in random bytes and repeated (each repeat's
    candidate is the OTHER sequence: no match), then 10 apart inside one
    round; zeros behind, so that the block is kept and compared."""
    buf = bytearray(np.random.default_rng(11).integers(0, 256, 2048, dtype=np.uint8).tobytes())
    for k, at in enumerate((500, 600, 700, 800, 900, 1000, 1540, 1550, 1560, 1570)):
        buf[at : at + 4] = COLLIDE_B if k % 2 else COLLIDE_A
    return bytes(buf) + bytes(SEG - len(buf))


CASES = {
    "zeros": bytes(SEG),  # offset 1, overlapping; every candidate inside its round
    "period3": (b"abc" * SEG)[:SEG],
    "period64": (SEGMENTS["random"][:64] * 64)[:SEG],  # candidates exactly a round back
    "collide": _collide(),
    "ascii_text": SEGMENTS["ascii_text"],
    "match_to_len_minus_5": SEGMENTS["match_to_len_minus_5"],
    "random": SEGMENTS["random"],
}


@functools.lru_cache(maxsize=None)
def model(seg: bytes, max_out: int = SEG + 256) -> bytes:
    return lz4ref.compress_block_wave(seg, max_out)


def comp_len(seg: bytes, max_out: int = SEG + 256) -> int:
    """What the kernel writes into comp_lens for ``seg``."""
    block = model(seg, max_out)
    return len(block) if 0 < len(block) < len(seg) else 0

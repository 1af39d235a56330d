"""Inputs of the MAFB10 byte-plane codec tests: named byte strings, built once,
at the smallest sizes at which the kernels of csrc/bytez.hip take another path."""

from __future__ import annotations

import functools

import numpy as np

from fp_corpus import random_bytes

SEG = 4096
HEADER = 6 + 8 + 1 + 1 + 4 + 256
#: lane_run changes at 513; lanes idle at the short ones; 4097 leaves a 1-byte raw tail
LENGTHS = (2, 3, 63, 64, 65, 512, 513, 4095, 4096, 4097, 2 * SEG + 100)
#: k distinct byte values, evenly spread, code at this width with no escape
DISTINCT_WIDTH = {1: 1, 3: 2, 7: 3, 15: 4, 31: 5, 63: 6, 127: 7}


def fp8(n: int, dtype: str, seed: int) -> bytes:
    import torch  # n seeded N(0,1) values cast to torch.<dtype>

    x = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    return x.to(getattr(torch, dtype)).view(torch.uint8).numpy().tobytes()


def _distinct() -> np.ndarray:
    """One segment per k: value 2j+1 is in every segment with k > j, so its
    rank in the block is j and segment k holds exactly the ranks 0..k-1."""
    return np.concatenate([(np.arange(SEG) % k) * 2 + 1 for k in DISTINCT_WIDTH]).astype(np.uint8)


def _sprinkled() -> bytes:
    """_distinct with rare (even) values that escape at every width: in the
    first lane's run, the last lane's, and on both sides of a lane boundary."""
    data = _distinct().reshape(-1, SEG).copy()
    data[:, [0, 5, 63, 64, 2047, 2048, SEG - 64, SEG - 1]] = np.arange(0xE0, 0xF0, 2, dtype=np.uint8)
    return data.tobytes()


@functools.lru_cache(maxsize=None)
def corpus() -> dict:
    """name -> bytes. Built once; nobody changes it."""
    c = {
        "e4m3_8k": fp8(2 * SEG, "float8_e4m3fn", 1),
        "e5m2_8k": fp8(2 * SEG, "float8_e5m2", 2),
        "distinct": _distinct().tobytes(),
        "sprinkled": _sprinkled(),
        # seg_len 0 between two coded segments
        "random_segment": fp8(SEG, "float8_e4m3fn", 3) + random_bytes(SEG, 4) + fp8(SEG, "float8_e5m2", 5),
        "random": random_bytes(2 * SEG, 6),  # not kept, between kept spans
    }
    for n in LENGTHS:
        c[f"len{n}"] = fp8(n, "float8_e4m3fn", 10 + n)
    return c


def segment_offsets(blob: bytes) -> list:
    """Offset in ``blob`` of every segment's payload (header fields only)."""
    raw_len = int.from_bytes(blob[6:14], "little")
    n_seg = int.from_bytes(blob[16:20], "little")
    offs, pos = [], HEADER + 4 * n_seg
    for s in range(n_seg):
        offs.append(pos)
        slen = int.from_bytes(blob[HEADER + 4 * s : HEADER + 4 * s + 4], "little")
        pos += slen or min(SEG, raw_len - s * SEG)
    return offs

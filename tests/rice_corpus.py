"""Inputs of the MARC10 tests (tests/test_ricecodec_cpu.py, _gpu.py): N(0,1)
through torch byte views, and the malformed containers, each a valid one with
one field patched."""

from __future__ import annotations

import numpy as np

SEG = 4096
MiB = 1024 * 1024
DTYPES = {1: "float8_e4m3fn", 2: "bfloat16", 4: "float32"}
LENGTHS = (3 * SEG, 2 * SEG + 1000, 2 * SEG + 1002, 40)


def gauss(dtype: str, n_bytes: int, seed: int = 3) -> bytes:
    """The first ``n_bytes`` bytes of N(0,1) cast to the torch dtype ``dtype``."""
    import torch

    x = torch.randn(n_bytes, generator=torch.Generator().manual_seed(seed))
    return x.to(getattr(torch, dtype)).view(torch.uint8).numpy().tobytes()[:n_bytes]


def constant(n_bytes: int = 2 * SEG + 1000) -> bytes:
    return bytes([0x3C]) * n_bytes


def hi_offsets(blob: bytes) -> list:
    """Offset in ``blob`` of every segment's k byte (of its bytes, where it is raw)."""
    from modal_amd.ops import container, ricecodec

    hdr = ricecodec.validate_container(blob)
    eff = container.effective_lens(hdr.seg_lens, hdr.raw_len)
    lo = (container.seg_raw_lens(len(eff), hdr.raw_len) // hdr.es) * (hdr.es - 1)
    return (hdr.payload_off + np.cumsum(eff) - eff + np.where(hdr.seg_lens != 0, lo, 0)).tolist()


def _end(bad: bytearray, at: int, j: int, delta: int) -> None:
    v = int.from_bytes(bad[at + 1 + 2 * j : at + 3 + 2 * j], "little") + delta
    bad[at + 1 + 2 * j : at + 3 + 2 * j] = v.to_bytes(2, "little")


def _drop(bad: bytearray, at: int) -> None:
    bad[at + 9 : at + 11] = bad[at + 7 : at + 9]  # end[4] = end[3] ...
    _end(bad, at, 4, -1)  # ... - 1


def _pad_bit(bad: bytearray, at: int) -> None:
    end0 = int.from_bytes(bad[at + 1 : at + 3], "little")
    bad[at + 33 + end0 - 1] |= 0x80


#: how -> (the input, its segment to patch, the patch at that segment's k byte,
#: whether the header fields alone give it away)
MALFORMED = {
    "k_8": ("gauss", 1, lambda bad, at: bad.__setitem__(at, 8), True),
    "end_decreases": ("gauss", 1, _drop, True),
    "end15_off_by_one": ("gauss", 1, lambda bad, at: _end(bad, at, 15, 1), True),
    "substream_too_short": ("gauss", 1, lambda bad, at: _end(bad, at, 3, -1), False),
    "substream_too_long": ("gauss", 1, lambda bad, at: _end(bad, at, 3, 1), False),
    # 63 one-bit codes to a sub-stream of the 1000-byte segment: bit 7 of its last byte is pad
    "pad_bit_set": ("constant", 2, _pad_bit, False),
}
INPUTS = {"gauss": lambda: gauss(DTYPES[1], 3 * SEG), "constant": constant}


def malformed(how: str) -> tuple:
    """(the valid container, the patched one, the segment patched, the raw
    bytes, whether ``validate_container`` must reject it)."""
    from modal_amd.ops import ricecodec

    name, seg, patch, in_header = MALFORMED[how]
    raw = INPUTS[name]()
    good = ricecodec.compress_buffer_cpu(raw, 1)
    bad = bytearray(good)
    patch(bad, hi_offsets(good)[seg])
    return good, bytes(bad), seg, raw, in_header

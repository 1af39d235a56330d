"""The segmented-container layer (ops/container.py) under both codecs, without
a GPU: the header checks the two validators share, held to the exact error
texts for either format; the order of the checks a format adds; the choice of
codec by magic; the segment-length helpers."""

from __future__ import annotations

import struct

import numpy as np
import pytest

import fp_corpus as fc
import lz4_corpus
from modal_amd.ops import compress, container, devcodec, fpcodec

MALZ_RAW = (
    bytes(4096)
    + lz4_corpus.SEGMENTS["ascii_text"]
    + np.random.default_rng(3).integers(0, 256, 100, dtype=np.uint8).tobytes()
)


@pytest.fixture(scope="module")
def malz() -> bytes:
    """A MALZ41 container from utils/lz4ref.py: 8292 raw bytes in three
    segments, the 100-byte last one stored raw; 2226 bytes."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(compress, "_native_core", lambda: None)
        blob = compress.compress_buffer_cpu(MALZ_RAW)
    assert blob is not None and len(blob) == 2226 and len(MALZ_RAW) == 8292
    assert struct.unpack_from("<QI", blob, 6) == (8292, 3)
    assert struct.unpack_from("<3I", blob, 18)[2] == 0
    return blob


def _set(blob: bytes, at: int, new: bytes) -> bytes:
    return blob[:at] + new + blob[at + len(new) :]


def _faults(blob: bytes, raw_len: int, n_seg: int, n_seg_at: int, header_fixed: int) -> dict:
    """name -> (blob, manifest raw_len or None): one fault per shared check."""
    return {
        "magic": (_set(blob, 0, b"MAXX99"), None),
        "short": (blob[: header_fixed - 1], None),
        "raw_len": (_set(blob, 6, struct.pack("<Q", raw_len + 1)), raw_len),
        "n_seg": (_set(blob, n_seg_at, struct.pack("<I", n_seg + 1)), None),
        "table": (blob[: header_fixed + 2], None),
        "cut": (blob[:-1], None),
        "appended": (blob + b"\x00", None),
    }


# the parent commit's texts, written out
MALZ_TEXTS = {
    "magic": "blk 7: not a MALZ41 container",
    "short": "blk 7: not a MALZ41 container",
    "raw_len": "blk 7: container raw_len 8293 != manifest 8292",
    "n_seg": "blk 7: container has 4 segments for 8292 bytes",
    "table": "blk 7: container truncated inside its segment table",
    "cut": "blk 7: container is 2225 bytes, header says 2226",
    "appended": "blk 7: container is 2227 bytes, header says 2226",
}
FP_TEXTS = {
    "magic": "blk 7: not a MAFP10 container",
    "short": "blk 7: not a MAFP10 container",
    "raw_len": "blk 7: container raw_len 129 != manifest 128",
    "n_seg": "blk 7: container has 2 segments for 128 bytes",
    "table": "blk 7: container truncated inside its segment table",
    "cut": "blk 7: container is 364 bytes, header says 365",
    "appended": "blk 7: container is 366 bytes, header says 365",
}


def _message(validate, blob: bytes, raw_len) -> str:
    with pytest.raises(ValueError) as err:
        validate(blob, raw_len, "blk 7")
    return str(err.value)


@pytest.mark.parametrize("fault", sorted(MALZ_TEXTS))
def test_shared_checks_malz41(malz, fault):
    assert compress.validate_container(malz, 8292, "blk 7")[0] == 8292
    blob, raw_len = _faults(malz, 8292, 3, 14, 18)[fault]
    assert _message(compress.validate_container, blob, raw_len) == MALZ_TEXTS[fault]


@pytest.mark.parametrize("fault", sorted(FP_TEXTS))
def test_shared_checks_mafp10(fault):
    assert len(fc.HAND_CONTAINER) == 365
    assert fpcodec.validate_container(fc.HAND_CONTAINER, 128, "blk 7").raw_len == 128
    blob, raw_len = _faults(fc.HAND_CONTAINER, 128, 1, 16, 276)[fault]
    assert _message(fpcodec.validate_container, blob, raw_len) == FP_TEXTS[fault]


def test_a_formats_own_checks_keep_their_place(malz):
    # MAFP10: the element size is looked at before raw_len is
    bad_es = _set(fc.HAND_CONTAINER, 14, b"\x03")
    assert _message(fpcodec.validate_container, bad_es, 127) == "blk 7: element size 3 is not 2 or 4"
    # and the order table before the segment table's bounds
    bad_order = _set(fc.HAND_CONTAINER, 21, b"\x3f")[:278]
    assert _message(fpcodec.validate_container, bad_order, None) == (
        "blk 7: order table is not a permutation"
    )
    # MALZ41: every comp_len before the container's size
    bad_len = _set(malz, 18, struct.pack("<I", 4096))[:-1]
    assert _message(compress.validate_container, bad_len, None) == (
        "blk 7: segment comp_len out of range"
    )


def test_codec_of_and_one_header_shape(malz):
    assert compress.codec_of(fc.HAND_CONTAINER) is fpcodec
    assert compress.codec_of(malz) is compress
    # whether a blob is compressed at all is out of band: anything else is MALZ41's
    assert compress.codec_of(MALZ_RAW) is compress and compress.codec_of(b"") is compress
    assert fpcodec.is_fp_container(fc.HAND_CONTAINER) and not fpcodec.is_fp_container(malz)
    for blob, raw_len, n_seg in ((malz, 8292, 3), (fc.HAND_CONTAINER, 128, 1)):
        hdr = devcodec.validate_container(blob, raw_len, 0)
        assert hdr[:3] == (hdr.raw_len, hdr.seg_lens, hdr.payload_off)
        assert hdr.raw_len == raw_len
        assert hdr.seg_lens.dtype == np.int32 and len(hdr.seg_lens) == n_seg
        payload = int(container.effective_lens(hdr.seg_lens, hdr.raw_len).sum())
        assert hdr.payload_off + payload == len(blob)
    raw_len, comp_lens, off = compress.validate_container(malz)  # still three values
    assert (raw_len, comp_lens.tolist(), off) == (8292, [26, 2070, 0], 30)
    assert compress.decompress_buffer_cpu(malz) == MALZ_RAW
    assert compress.decompress_buffer_cpu(fc.HAND_CONTAINER) == fc.HAND_RAW


SEG_RAW = {0: [], 1: [1], 4095: [4095], 4096: [4096], 4097: [4096, 1], 8192: [4096, 4096]}


@pytest.mark.parametrize("raw_len", sorted(SEG_RAW))
def test_segment_lengths(raw_len):
    want = SEG_RAW[raw_len]
    got = container.seg_raw_lens(len(want), raw_len)
    assert got.dtype == np.int64 and got.tolist() == want
    for eff in (container.effective_lens, compress.effective_lens):
        raw = eff(np.zeros(len(want), dtype=np.int32), raw_len)
        assert raw.dtype == np.int64 and raw.tolist() == want
        assert eff([7] * len(want), raw_len).tolist() == [7] * len(want)
        # the last segment raw, the others coded, and the other way round
        mixed = [9] * len(want)
        mixed[-1:] = [0] * len(want[-1:])
        assert eff(mixed, raw_len).tolist() == [9] * (len(want) - 1) + want[-1:]
        assert eff(mixed[::-1], raw_len).tolist() == (want[:1] + [9] * (len(want) - 1))[: len(want)]

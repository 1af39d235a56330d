"""The wavefront LZ4 encoder's model (utils/lz4ref.compress_block_wave) writes
valid blocks, no longer than the lane parse's where listed; ``lz_parser`` is
checked at every door."""

from __future__ import annotations

import pytest

import lz4_corpus as corpus
from lz4wave_cases import CASES, LENGTHS
from modal_amd.ops import compress, devcodec
from modal_amd.runtime import gpu_snapshot
from modal_amd.utils import lz4ref

INPUTS = {**corpus.SEGMENTS, **CASES, "text_variant": corpus.variant(2)}
# checked on the CPU: 1812 <= 2070, 3534 <= 3637, 1798 <= 2044, 1049 <= 1112, 2752 <= 2972
NO_LONGER_THAN_LANE = ("ascii_text", "planted_repeats", "text_variant", "tiled_1k", "alphabet3")


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_model_blocks_decode(name):
    for n in LENGTHS:
        seg = INPUTS[name][:n]
        block = lz4ref.compress_block_wave(seg)
        assert lz4ref.decompress_block(block, n) == seg
        assert corpus.strict_decode(block, n) == seg


@pytest.mark.parametrize("name", NO_LONGER_THAN_LANE)
def test_model_is_no_longer_than_the_lane_parse(name):
    seg = INPUTS[name]
    assert len(lz4ref.compress_block_wave(seg)) <= len(lz4ref.compress_block(seg))


def test_unknown_parser_is_refused():
    for call in (
        lambda: compress.compress_buffer(bytes(8192), lz_parser="bogus"),
        lambda: devcodec.encode_host(bytes(8192), lz_parser="bogus"),
        lambda: gpu_snapshot.capture_manifest(None, lz_parser="bogus"),
    ):
        with pytest.raises(ValueError, match="lz_parser"):
            call()


def test_encode_host_wave_round_trips():
    data = (CASES["ascii_text"] + CASES["random"] + CASES["zeros"]) * 90 + b"tail"
    blocks = devcodec.encode_host(data, lz_parser="wave")
    assert devcodec.decode_host(blocks) == data

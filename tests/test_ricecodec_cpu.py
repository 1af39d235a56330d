"""The MARC10 numpy codec (ops/ricecodec.py), the specification of the
format: round trips at every element size and tail, the segments whose coding
is known by hand, every malformation a reader rejects, its size against the
fixed-width codecs, and the block codec with ``rank_coding="rice"``."""

from __future__ import annotations

import numpy as np
import pytest

import rice_corpus as rc
from modal_amd.ops import bytecodec, compress, devcodec, fpcodec, ricecodec
from modal_amd.ops.hashing import content_digest


def _k_and_streams(z: bytes, s: int) -> tuple:
    """(k, the stream area) of coded segment ``s``."""
    at = rc.hi_offsets(z)[s]
    area = int.from_bytes(z[at + 31 : at + 33], "little")
    return z[at], z[at + 33 : at + 33 + area]


@pytest.mark.parametrize("n", rc.LENGTHS)
@pytest.mark.parametrize("es", [1, 2, 4])
def test_model_round_trip(es, n):
    raw = rc.gauss(rc.DTYPES[es], n)
    z = ricecodec.compress_buffer_cpu(raw, es)
    if n == 40:  # 33 bytes of k and end table: never coded
        assert z is None
        return
    hdr = ricecodec.validate_container(z, n)
    assert hdr.es == es and z[:6] == b"MARC10" and np.all(hdr.seg_lens[:2] > 0)
    # a tail that is not whole elements comes out raw
    assert (hdr.seg_lens[2] == 0) == ((n - 2 * rc.SEG) % es != 0)
    assert ricecodec.decompress_buffer_cpu(z) == raw


def test_constant_and_random_segments():
    raw = rc.constant(rc.SEG) + np.random.default_rng(5).integers(0, 256, rc.SEG, dtype=np.uint8).tobytes()
    z = ricecodec.compress_buffer_cpu(raw, 1)
    hdr = ricecodec.validate_container(z)
    k, streams = _k_and_streams(z, 0)
    # rank 0 at k = 0 is one zero bit: 256 bits to a sub-stream
    assert k == 0 and streams == bytes(16 * 32) and hdr.seg_lens.tolist() == [33 + 16 * 32, 0]
    assert ricecodec.decompress_buffer_cpu(z) == raw


def test_rare_top_bytes_take_the_escape():
    seg = np.full((2048, 2), 0x3F, dtype=np.uint8)
    seg[:, 0] = np.arange(2048) & 255
    seg[100:140, 1] = 0xA7 - np.arange(40)  # 40 top bytes seen once: 0xA7 has rank 40
    raw = seg.tobytes()
    z = ricecodec.compress_buffer_cpu(raw, 2)
    hdr = ricecodec.validate_container(z)
    k, streams = _k_and_streams(z, 0)
    assert k == 0 and hdr.order[40] == 0xA7 and 40 >> k >= ricecodec.Q_ESC
    # sub-stream 0: 100 elements of rank 0, then element 100 escaped
    bits = np.unpackbits(np.frombuffer(streams, dtype=np.uint8), bitorder="little")
    assert not bits[:100].any() and bits[100:112].all()
    assert np.packbits(bits[112:120], bitorder="little")[0] == 0xA7
    assert ricecodec.decompress_buffer_cpu(z) == raw


@pytest.mark.parametrize("how", sorted(rc.MALFORMED))
def test_readers_reject_malformed_segments(how):
    good, bad, seg, raw, in_header = rc.malformed(how)
    assert ricecodec.decompress_buffer_cpu(good) == raw
    with pytest.raises(ValueError, match=f"corrupt at segment {seg}"):
        ricecodec.decompress_buffer_cpu(bad)
    if in_header:
        with pytest.raises(ValueError, match=f"segment {seg}"):
            ricecodec.validate_container(bad)
    else:
        ricecodec.validate_container(bad)  # only the walk finds it


@pytest.mark.parametrize("dtype,es", [("bfloat16", 2), ("float8_e4m3fn", 1), ("float8_e5m2", 1)])
def test_smaller_than_the_fixed_width_container(dtype, es):
    raw = rc.gauss(dtype, rc.MiB)
    fixed = bytecodec.compress_buffer_cpu(raw) if es == 1 else fpcodec.compress_buffer_cpu(raw, es)
    rice = ricecodec.compress_buffer_cpu(raw, es)
    assert len(rice) < len(fixed)
    assert ricecodec.decompress_buffer_cpu(rice) == raw


def test_block_codec_takes_rank_coding_and_decodes_by_magic():
    a = rc.gauss("bfloat16", rc.MiB)
    rice = devcodec.encode_host(a, block_size=rc.MiB, elem_size=2, rank_coding="rice")
    fixed = devcodec.encode_host(a, block_size=rc.MiB, elem_size=2)
    assert rice[0].payload[:6] == b"MARC10" and fixed[0].payload[:6] == b"MAFP10"
    assert rice[0].digest == fixed[0].digest
    assert devcodec.decode_host([tuple(b) for b in rice]) == a
    tile = bytes(range(256)) * 256
    lz = devcodec.EncodedBlock(content_digest(tile), len(tile), compress.compress_buffer_cpu(tile), True)
    assert compress.is_compressed(lz.payload)
    assert compress.codec_of(rice[0].payload) is ricecodec
    assert devcodec.decode_host([tuple(b) for b in (lz, fixed[0], rice[0])]) == tile + a + a
    with pytest.raises(ValueError, match="rank_coding"):
        devcodec.encode_host(a, elem_size=2, rank_coding="huffman")


def test_scheduler_checks_rank_coding():
    import asyncio

    from modal_amd.exception import InvalidError
    from modal_amd.runtime import gpu_snapshot as gs
    from modal_amd.scheduler.core import Scheduler

    for kw in ({"float_codec": True, "rank_coding": "huffman"}, {"rank_coding": "rice"}):
        with pytest.raises(InvalidError, match="rank_coding"):
            asyncio.run(Scheduler.worker_snapshot(None, 0, block_addressed=True, **kw))
    with pytest.raises(ValueError, match="rank_coding"):
        gs.capture_manifest(None, float_codec=True, rank_coding="huffman")

"""The MAFP10 float-plane codec without a GPU: the numpy model
(ops/fpcodec.py) against the corpus and the independent strict decoder of
tests/fp_corpus.py, the validator's and decoder's rejections, the ratio on
bf16 weights, and the way up through the CAS and block-addressed snapshots."""

from __future__ import annotations

import os
import pickle

import pytest

import fp_corpus as fc

NAMES = sorted(fc.corpus())
#: inputs the 5 % rule must turn down
DECLINED = {"random_es2", "random_es4"}


@pytest.fixture(scope="module")
def containers() -> dict:
    from modal_amd.ops import fpcodec

    return {name: fpcodec.compress_buffer_cpu(data, es) for name, (data, es) in fc.corpus().items()}


@pytest.mark.parametrize("name", NAMES)
def test_numpy_codec_round_trips_and_strict_decoder_agrees(containers, name):
    from modal_amd.ops import fpcodec

    data, es = fc.corpus()[name]
    z = containers[name]
    if z is None:
        return  # test_what_is_kept says which may be None
    hdr = fpcodec.validate_container(z, len(data), name)
    assert (hdr.raw_len, hdr.es) == (len(data), es)
    assert fpcodec.is_fp_container(z)
    assert fpcodec.decompress_buffer_cpu(z) == data
    assert fc.strict_decode(z, len(data)) == data


def test_what_is_kept(containers):
    """Only what cannot save 5 % is turned down: random bytes, and inputs so
    short that a two-element tail or the raw segment rule leaves nothing."""
    from modal_amd.ops import compress

    for name, z in containers.items():
        data, _es = fc.corpus()[name]
        if name in DECLINED:
            assert z is None, name
        elif z is not None:
            payload = len(z) - (fc.HEADER + 4 * -(-len(data) // fc.SEG))
            assert compress.worth_keeping(payload, len(data)), name
    kept = {n for n, z in containers.items() if z is not None}
    assert {"bf16_n01_1m", "bf16_n002_1m", "fp32_n01", "fp16_n01", "zeros_es2",
            "constant_bf16", "escapes_es2", "escapes_es4", "nseg257_es2",
            "random_segment_es2", "random_segment_es4", "tail4095_es2"} <= kept
    assert {f"distinct{k}_es2" for k in fc.DISTINCT_WIDTH if k < 127} <= kept


def _width_of_segment(z: bytes, s: int) -> int:
    hdr_raw, es, _order, seg_lens, _off = fc.parse(z)
    if seg_lens[s] == 0:
        return 0
    L = min(fc.SEG, hdr_raw - s * fc.SEG)
    return z[fc.segment_offsets(z)[s] + (L // es) * (es - 1)]


@pytest.mark.parametrize("k", sorted(fc.DISTINCT_WIDTH))
def test_distinct_top_bytes_drive_every_width(k):
    """k = 2^b - 1 evenly spread top bytes code at width b with no escape; at
    b = 7 a bf16 segment still saves 6 %, so the container is kept."""
    from modal_amd.ops import fpcodec

    data, es = fc.corpus()[f"distinct{k}_es2"]
    z = fpcodec.compress_buffer_cpu(data, es)
    assert z is not None
    b = fc.DISTINCT_WIDTH[k]
    m = fc.SEG // es
    hdr = fpcodec.validate_container(z)
    assert [_width_of_segment(z, s) for s in range(4)] == [b] * 4
    assert hdr.seg_lens.tolist() == [m * (es - 1) + 1 + m * b // 8] * 4


def test_raw_segment_inside_a_kept_container(containers):
    for es in (2, 4):
        z = containers[f"random_segment_es{es}"]
        seg_lens = fc.parse(z)[3]
        assert seg_lens[5] == 0 and all(seg_lens[:5]) and all(seg_lens[6:])


def test_short_and_odd_tails(containers):
    """The last segment: coded when it is a whole number of elements and
    pays, raw when odd (4095; 4094 at es 4) or too short to pay (one element)."""
    for es, tails in fc.TAILS.items():
        for tail in tails:
            z = containers[f"tail{tail}_es{es}"]
            last = fc.parse(z)[3][-1]
            if tail % es or tail // es < 3:
                assert last == 0, (es, tail)
            else:
                assert 0 < last < tail, (es, tail)


def test_hand_assembled_container_pins_the_bit_order():
    from modal_amd.ops import fpcodec

    assert len(fc.HAND_RAW) == 128 and len(fc.HAND_CONTAINER) == fc.HEADER + 4 + 85
    assert fpcodec.compress_buffer_cpu(fc.HAND_RAW, 2) == fc.HAND_CONTAINER
    assert fpcodec.decompress_buffer_cpu(fc.HAND_CONTAINER) == fc.HAND_RAW
    assert fc.strict_decode(fc.HAND_CONTAINER) == fc.HAND_RAW


@pytest.mark.parametrize("case", fc.malformed(), ids=lambda c: c[0])
def test_malformed_containers_raise_value_error(case):
    from modal_amd.ops import compress, fpcodec

    name, blob, raw_len = case
    with pytest.raises(ValueError):
        fc.strict_decode(blob, raw_len)  # the corpus means what it says
    with pytest.raises(ValueError, match="^blk 7: " if not name.startswith(("b_", "escape")) else None):
        fpcodec.validate_container(blob, raw_len, what="blk 7")
        fpcodec.decompress_buffer_cpu(blob)
    if name != "magic" and raw_len is None:
        with pytest.raises(ValueError):
            compress.decompress_buffer_cpu(blob)  # the CAS's front door


def test_decoder_names_the_segment():
    from modal_amd.ops import fpcodec

    z = fpcodec.compress_buffer_cpu(*fc.corpus()["nseg5_es2"])
    with pytest.raises(ValueError, match="MAFP10 container corrupt at segment 3"):
        fpcodec.decompress_buffer_cpu(fc.break_segment(z, 3))


@pytest.mark.parametrize("name", ["bf16_n01_1m", "bf16_n002_1m"])
def test_bf16_gaussian_ratio(containers, name):
    """An independent script measured 0.7125 and 0.7126 for these
    distributions with all headers; 0.73 leaves about 2 % for the seed."""
    data, _es = fc.corpus()[name]
    ratio = len(containers[name]) / len(data)
    print(f"{name}: container/raw = {ratio:.4f}")
    assert ratio < 0.73


def test_random_bytes_are_declined(containers):
    assert containers["random_es2"] is None and containers["random_es4"] is None


def test_blobstore_returns_raw_bytes_of_a_float_container(tmp_path, containers):
    from modal_amd.ops.hashing import content_digest
    from modal_amd.scheduler.blobs import BlobStore

    data, _es = fc.corpus()["bf16_n01_1m"]
    store = BlobStore(str(tmp_path / "blobs"))
    digest = content_digest(data)
    assert store.put_prepared(digest, containers["bf16_n01_1m"], True)
    assert store.get_stored(digest) == (containers["bf16_n01_1m"], True)
    assert store.get(digest) == data


def test_encode_host_tries_lz4_first_and_digests_do_not_move():
    from modal_amd.ops import compress, devcodec, fpcodec

    MiB = fc.MiB
    gauss, _ = fc.corpus()["bf16_n01_1m"]
    data = bytes(MiB) + gauss + fc.random_bytes(MiB, seed=9) + gauss[: MiB // 2]
    plain = devcodec.encode_host(data, block_size=MiB)
    hinted = devcodec.encode_host(data, block_size=MiB, elem_size=2)
    assert [b.digest for b in hinted] == [b.digest for b in plain]
    assert [b.compressed for b in hinted] == [compress.gpu_available() or
                                              compress._native_core() is not None,
                                              True, False, False]
    assert fpcodec.is_fp_container(hinted[1].payload)
    assert not fpcodec.is_fp_container(hinted[0].payload)
    assert not plain[1].compressed
    assert devcodec.decode_host([tuple(b) for b in hinted]) == data
    bad = [tuple(b) for b in hinted]
    bad[1] = bad[1][:2] + (fc.break_segment(hinted[1].payload, 2), True)
    with pytest.raises(ValueError, match="corrupt at segment 2"):
        devcodec.decode_host(bad)
    with pytest.raises(ValueError):
        devcodec.encode_host(data, block_size=MiB, elem_size=3)


def _stored_bytes(root: str) -> int:
    return sum(os.path.getsize(os.path.join(d, f)) for d, _s, files in os.walk(root) for f in files)


def test_capture_manifest_float_codec_cpu_tensors(tmp_path):
    import torch

    from modal_amd.runtime import gpu_snapshot as gs
    from modal_amd.scheduler.blobs import BlobStore

    g = torch.Generator().manual_seed(5)
    state = {
        "w_bf16": torch.randn(3, 256 * 1024 + 7, generator=g).to(torch.bfloat16),
        "w_fp32": torch.randn(512 * 1024 + 3, generator=g),
        "ids": torch.randint(0, 1 << 40, (200 * 1024,), generator=g),  # not float: no hint
    }
    stores = {}
    manifests = {}
    try:
        for on in (False, True):
            gs._registered_tensors.clear()
            gs._restored_tensors.clear()
            for key, t in state.items():
                gs.register_tensor(key, t)
            stores[on] = BlobStore(str(tmp_path / f"blobs-{on}"))
            manifests[on] = gs.capture_manifest(stores[on], float_codec=on)
        off_m, on_m = pickle.loads(manifests[False]), pickle.loads(manifests[True])
        assert on_m["version"] == 2
        assert on_m["tensors"] == off_m["tensors"]  # same digests, same lengths
        raw = sum(t.numel() * t.element_size() for t in state.values())
        off_b, on_b = _stored_bytes(stores[False].root), _stored_bytes(stores[True].root)
        print(f"raw {raw}, stored without {off_b}, with the float codec {on_b}")
        assert on_b < off_b
        assert on_b < 0.9 * raw

        gs._registered_tensors.clear()
        gs._restored_tensors.clear()
        gs.restore_payload(manifests[True], stores[True])  # no flag on restore
        for key, t in state.items():
            out = gs.restored_tensor(key)
            assert out.dtype == t.dtype and out.shape == t.shape
            assert torch.equal(out.view(torch.uint8), t.view(torch.uint8))
    finally:
        gs._registered_tensors.clear()
        gs._restored_tensors.clear()


def test_float_codec_needs_block_addressed():
    import asyncio

    from modal_amd.exception import InvalidError
    from modal_amd.scheduler.core import Scheduler

    with pytest.raises(InvalidError, match="block_addressed"):
        asyncio.run(Scheduler.worker_snapshot(None, 0, float_codec=True))

"""The MAFB10 byte-plane codec without a GPU: the numpy model (ops/bytecodec.py)
on tests/byte_corpus.py, a container worked out by hand, the validator's
rejections, and the way up through the block codec and snapshots."""

from __future__ import annotations

import pickle
import struct

import pytest

import byte_corpus as bc
from fp_corpus import HAND_TOPS, MiB, random_bytes

# 64 elements: A 0x3F (40), B 0x40 (12), C 0xBF (8), D 0x00 (2), E 0xFF (2), so
# the ranks are A0 B1 C2 D3 E4 and every other byte follows ascending. Costs:
# b=1 1+8+24, b=2 1+16+4 = 21, b=3 1+24+0, so b = 2 and D, E escape (code 3).
HAND_RAW = bytes({"A": 0x3F, "B": 0x40, "C": 0xBF, "D": 0x00, "E": 0xFF}[t] for t in HAND_TOPS)
_USED = [0x3F, 0x40, 0xBF, 0x00, 0xFF]
HAND_CONTAINER = (
    bytes.fromhex("4d4146423130" "4000000000000000" "01" "00" "01000000")  # MAFB10, 64, es, 0, n_seg
    + bytes(_USED + [v for v in range(256) if v not in _USED])  # order
    + bytes.fromhex(
        "15000000"  # seg_len 21
        "02"  # b
        # four elements a byte, element 0 in bits 0-1: AAAA -> 00, ABAC -> 0 | 1<<2 | 0 | 2<<6 = 84
        "0084108c40b004201042432004230159"
        "00ffff00"  # escapes in element order: D E E D
    )
)


@pytest.fixture(scope="module")
def model() -> dict:
    from modal_amd.ops import bytecodec

    return {name: bytecodec.compress_buffer_cpu(data) for name, data in bc.corpus().items()}


@pytest.mark.parametrize("name", sorted(bc.corpus()))
def test_model_round_trips_what_it_keeps(model, name):
    from modal_amd.ops import bytecodec, compress

    data, z = bc.corpus()[name], model[name]
    assert (z is None) == (name in ("random", "len2"))
    if z is not None:
        assert bytecodec.validate_container(z, len(data), name).raw_len == len(data)
        assert compress.codec_of(z) is bytecodec
        assert bytecodec.decompress_buffer_cpu(z) == data
        assert compress.decompress_buffer_cpu(z) == data  # the GPU-less reader's door


def test_widths_raw_segments_and_the_keep_rule(model):
    from modal_amd.ops import bytecodec

    z = model["distinct"]
    assert [z[at] for at in bc.segment_offsets(z)] == list(bc.DISTINCT_WIDTH.values())
    want = [1 + bc.SEG * b // 8 for b in bc.DISTINCT_WIDTH.values()]
    assert bytecodec.validate_container(z).seg_lens.tolist() == want
    lens = bytecodec.validate_container(model["random_segment"]).seg_lens.tolist()
    assert lens[1] == 0 and lens[0] and lens[2]
    assert bytecodec.validate_container(model["len4097"]).seg_lens[1] == 0  # a 1-byte tail
    # the model gives 0.883 (e4m3) and 0.763 (e5m2) of raw at 8 KiB: kept
    for name in ("e4m3_8k", "e5m2_8k"):
        assert len(model[name]) < 0.95 * 2 * bc.SEG + bc.HEADER + 8


def test_hand_built_container_and_a_mafp10_reader_rejects_it():
    from modal_amd.ops import bytecodec, fpcodec

    assert bytecodec.compress_buffer_cpu(HAND_RAW) == HAND_CONTAINER
    assert bytecodec.decompress_buffer_cpu(HAND_CONTAINER) == HAND_RAW
    with pytest.raises(ValueError, match="not a MAFP10 container"):
        fpcodec.validate_container(HAND_CONTAINER)


def _with(at: int, new: bytes, size: int = len(HAND_CONTAINER)) -> bytes:
    z = HAND_CONTAINER[:at] + new + HAND_CONTAINER[at + len(new) :]
    return (z + bytes(size))[:size]


#: one container per rejection of the validator (test_rankcodec_cpu.py reads it too)
MALFORMED = {
    "es": _with(14, b"\x02"),
    "order": _with(21, b"\x3f"),  # order holds 0x3F twice
    "seg_len_1": _with(bc.HEADER, struct.pack("<I", 1), bc.HEADER + 4 + 1),
    "seg_len_L": _with(bc.HEADER, struct.pack("<I", 64), bc.HEADER + 4 + 64),  # seg_len == L
    "truncated": HAND_CONTAINER[:-1],
    "over_long": HAND_CONTAINER + b"\x00",
}


@pytest.mark.parametrize("blob", list(MALFORMED.values()), ids=list(MALFORMED))
def test_validator_rejects(blob):
    from modal_amd.ops import bytecodec

    with pytest.raises(ValueError, match="^blk 7: "):
        bytecodec.validate_container(blob, what="blk 7")


def test_encode_host_round_trips_an_e4m3_block():
    from modal_amd.ops import bytecodec, devcodec

    data = bc.fp8(MiB, "float8_e4m3fn", 7) + random_bytes(MiB, 8)
    blocks = devcodec.encode_host(data, block_size=MiB, elem_size=1)
    assert [b.compressed for b in blocks] == [True, False]
    assert bytecodec.is_byte_container(blocks[0].payload)
    assert [b.digest for b in blocks] == [b.digest for b in devcodec.encode_host(data, block_size=MiB)]
    assert devcodec.decode_host([tuple(b) for b in blocks]) == data


def test_capture_manifest_stores_an_fp8_tensor_as_mafb10(tmp_path):
    import torch

    from modal_amd.runtime import gpu_snapshot as gs
    from modal_amd.scheduler.blobs import BlobStore

    raw = bc.fp8(64 * 1024, "float8_e4m3fn", 9)
    t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(torch.float8_e4m3fn)
    stores, manifests = {}, {}
    try:
        for on in (False, True):
            gs._registered_tensors.clear()
            gs.register_tensor("w", t)
            stores[on] = BlobStore(str(tmp_path / f"blobs-{on}"))
            manifests[on] = gs.capture_manifest(stores[on], float_codec=on)
        entry = pickle.loads(manifests[True])["tensors"]["w"]
        assert entry == pickle.loads(manifests[False])["tensors"]["w"]
        stored, compressed = stores[True].get_stored(entry["blocks"][0])
        assert compressed and stored[:6] == b"MAFB10"
        assert stores[False].get_stored(entry["blocks"][0]) == (raw, False)
        gs._registered_tensors.clear()
        gs._restored_tensors.clear()
        gs.restore_payload(manifests[True], stores[True])  # no flag on restore
        out = gs.restored_tensor("w")
        assert out.dtype == t.dtype and out.view(torch.uint8).numpy().tobytes() == raw
    finally:
        gs._registered_tensors.clear()
        gs._restored_tensors.clear()

"""The layer MAFP10 and MAFB10 share (ops/rankcodec.py) without a GPU: both
formats still write the containers and raise the messages recorded from the
commit before that layer existed (tests/golden/rank_codecs_parent.json, which
names it), the GPU-less reader's door reads them back, and the byte-plane
model is the shared numpy encoder at element size 1."""

from __future__ import annotations

import hashlib
import json
import os

import pytest

import byte_corpus as bc
import fp_corpus as fc
import test_bytecodec_cpu as tb

WHAT = "blk 7"


@pytest.fixture(scope="module")
def golden() -> dict:
    path = os.path.join(os.path.dirname(__file__), "golden", "rank_codecs_parent.json")
    with open(path) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def containers() -> dict:
    """(format, name) -> (raw bytes, the numpy model's container or None)."""
    from modal_amd.ops import bytecodec, fpcodec

    made = {
        ("fp", name): (data, fpcodec.compress_buffer_cpu(data, es))
        for name, (data, es) in fc.corpus().items()
    }
    for name, data in bc.corpus().items():
        made["byte", name] = (data, bytecodec.compress_buffer_cpu(data))
    return made


def _sha(z) -> object:
    return None if z is None else hashlib.sha256(z).hexdigest()


def _message(call) -> str:
    with pytest.raises(ValueError) as err:
        call()
    return str(err.value)


def test_containers_are_the_parent_commits(golden, containers):
    got = {"fp": {}, "byte": {}}
    for (fmt, name), (_data, z) in containers.items():
        got[fmt][name] = {str(fc.corpus()[name][1]): _sha(z)} if fmt == "fp" else _sha(z)
    assert got["fp"] == golden["fp_containers"]
    assert got["byte"] == golden["byte_containers"]
    assert None in got["byte"].values() and {"2": None} in got["fp"].values()


def test_the_reader_s_door_returns_the_corpus_bytes(containers):
    from modal_amd.ops import compress

    for (fmt, name), (data, z) in containers.items():
        if z is not None:
            assert compress.decompress_buffer_cpu(z) == data, (fmt, name)


def test_messages_are_the_parent_commits(golden):
    from modal_amd.ops import bytecodec, fpcodec

    def fp_reader(blob: bytes, raw_len) -> None:
        fpcodec.validate_container(blob, raw_len, what=WHAT)
        fpcodec.decompress_buffer_cpu(blob)

    fp = {
        name: _message(lambda: fp_reader(blob, raw_len)) for name, blob, raw_len in fc.malformed()
    }
    assert fp == golden["fp_errors"]
    byte = {
        name: _message(lambda: bytecodec.validate_container(blob, what=WHAT))
        for name, blob in tb.MALFORMED.items()
    }
    assert len(byte) == 6 and byte == golden["byte_errors"]


def test_each_format_rejects_the_other_s_element_sizes_and_magic(golden):
    from modal_amd.ops import bytecodec, fpcodec

    fp_es1 = fc.HAND_CONTAINER[:14] + b"\x01" + fc.HAND_CONTAINER[15:]
    byte_es2 = tb.HAND_CONTAINER[:14] + b"\x02" + tb.HAND_CONTAINER[15:]
    got = {
        "mafp10_es1": _message(lambda: fpcodec.validate_container(fp_es1, what=WHAT)),
        "mafb10_es2": _message(lambda: bytecodec.validate_container(byte_es2, what=WHAT)),
        "mafb10_to_fpcodec": _message(
            lambda: fpcodec.validate_container(tb.HAND_CONTAINER, what=WHAT)
        ),
    }
    assert got == golden["cross_format"]
    assert got == {
        "mafp10_es1": "blk 7: element size 1 is not 2 or 4",
        "mafb10_es2": "blk 7: element size 2 is not 1",
        "mafb10_to_fpcodec": "blk 7: not a MAFP10 container",
    }


def test_the_byte_plane_model_is_the_shared_encoder_at_element_size_1(containers):
    from modal_amd.ops import bytecodec, rankcodec

    assert isinstance(bytecodec.FORMAT, rankcodec.Format)
    for (fmt, name), (data, z) in containers.items():
        if fmt == "byte":
            assert bytecodec.FORMAT.compress_buffer_cpu(data, 1) == z, name

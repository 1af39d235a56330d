"""The wavefront LZ4 encoder (ops/csrc/lz4w.hip) against its model, byte for
byte, slot and comp_len, and through the doors that take ``lz_parser``."""

from __future__ import annotations

import numpy as np
import pytest

from lz4_corpus import SEG
from lz4wave_cases import CASES, LENGTHS, comp_len, model
from modal_amd.ops import compress, devcodec

pytestmark = pytest.mark.gpu
CANARY = 0xA5
GUARD = 4096
STRIDE = compress.OUT_STRIDE


def _launch(data: bytes, span_off: int, out_stride: int):
    """One wave-encoder launch over ``data`` at ``span_off`` bytes past a
    16-byte boundary. Returns (comp_lens, slot bytes, canaries intact)."""
    import torch  # before the library: one HIP runtime in the process

    from modal_amd.ops import load_lib

    lib = load_lib(required=True)
    n_seg = -(-len(data) // SEG)
    src = torch.from_numpy(np.frombuffer(bytes(span_off) + data, dtype=np.uint8).copy()).cuda()
    assert src.data_ptr() % 16 == 0
    whole = torch.full((2 * GUARD + n_seg * out_stride,), CANARY, dtype=torch.uint8, device="cuda")
    lens = torch.full((n_seg,), -1, dtype=torch.int32, device="cuda")
    rc = lib.ma_lz4_compress_wave(
        src.data_ptr() + span_off, len(data), whole.data_ptr() + GUARD, lens.data_ptr(),
        out_stride, n_seg, torch.cuda.current_stream().cuda_stream,
    )
    assert rc == 0
    host = whole.cpu().numpy()
    intact = bool((host[:GUARD] == CANARY).all() and (host[-GUARD:] == CANARY).all())
    return lens.cpu().numpy().tolist(), host[GUARD:-GUARD], intact


def _assert_is_model(segs, comp_lens, slots, out_stride) -> None:
    assert comp_lens == [comp_len(s, out_stride) for s in segs]
    for i, (seg, clen) in enumerate(zip(segs, comp_lens)):
        got = slots[i * out_stride : i * out_stride + clen].tobytes()
        assert got == model(seg, out_stride)[:clen], f"segment {i}"
        # nothing but the block is written
        assert (slots[i * out_stride + clen : (i + 1) * out_stride] == CANARY).all(), f"segment {i}"


@pytest.mark.parametrize("span_off", (0, 1, 15))
@pytest.mark.parametrize("n", LENGTHS + (SEG + 1,))
def test_kernel_is_the_model(n, span_off):
    for name, case in CASES.items():
        data = (case + case)[:n]
        segs = [data[:SEG], data[SEG:]] if n > SEG else [data]
        comp_lens, slots, intact = _launch(data, span_off, STRIDE)
        _assert_is_model(segs, comp_lens, slots, STRIDE)
        assert intact, name
    if n == SEG:  # random bytes: kernel and model say 0; every other case is kept
        assert [k for k, case in CASES.items() if comp_len(case) == 0] == ["random"]


def test_many_segments_in_one_launch():
    segs = list(CASES.values()) * 40  # more segments than the chip runs at once per CU
    comp_lens, slots, intact = _launch(b"".join(segs), 4, STRIDE)
    _assert_is_model(segs, comp_lens, slots, STRIDE)
    assert intact


def test_small_slot_stores_raw_in_bounds():
    small = 64
    segs = list(CASES.values())
    comp_lens, slots, intact = _launch(b"".join(segs), 0, small)
    _assert_is_model(segs, comp_lens, slots, small)
    assert intact
    assert comp_lens[0] == len(model(CASES["zeros"])) and comp_lens[2] == 0  # period64: 90 > 64


def _mix() -> bytes:  # 1 MiB + 100 B
    return (b"".join(CASES.values()) * 37)[: 1024 * 1024] + CASES["ascii_text"][:100]


def test_compress_buffer_gpu_wave():
    data = _mix()
    z = compress.compress_buffer_gpu(data, lz_parser="wave")
    assert compress.decompress_buffer_gpu(z) == data
    assert compress.decompress_buffer_cpu(z) == data
    segs = [data[i : i + SEG] for i in range(0, len(data), SEG)]
    assert compress.parse_header(z)[1] == [comp_len(s) for s in segs]
    lane = compress.compress_buffer_gpu(data)
    assert lane == compress.compress_buffer_gpu(data, lz_parser="lane") and len(z) < len(lane)


def test_encode_tensor_wave():
    import torch

    t = torch.from_numpy(np.frombuffer(_mix(), dtype=np.uint8).copy()).cuda()
    blocks = devcodec.encode_tensor(t, lz_parser="wave")
    assert blocks[0].compressed
    assert blocks == devcodec.encode_tensor(t, lz_parser="wave")
    assert devcodec.encode_tensor(t) == devcodec.encode_tensor(t, lz_parser="lane")
    back = torch.zeros_like(t)
    devcodec.decode_tensor(blocks, back, verify=True)
    assert torch.equal(back, t)

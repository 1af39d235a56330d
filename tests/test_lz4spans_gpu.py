"""The span-table LZ4 encoder (ops/csrc/lz4s.hip), both parsers: its slots and
comp_lens against one per-span launch per span, byte for byte, and the
containers of ``compress_spans_gpu`` decoded on the host against the source."""

from __future__ import annotations

import numpy as np
import pytest

from modal_amd.ops import compress, container, devcodec

pytestmark = pytest.mark.gpu
SEG = compress.SEG_SIZE
STRIDE = compress.OUT_STRIDE
MiB = 1024 * 1024
# span lengths; "scattered" lies in descending address order with gaps, its span 1 is random
CASES = {
    "one_segment": [SEG],
    "tail_1": [SEG + 1],
    "tail_3": [SEG + 3],  # below the match limits
    "tail_12": [SEG + 12],  # at them
    "straddle": [100 * SEG, 60 * SEG],  # slot 100: inside a workgroup of 32, 64 or 128 slots
    "scattered": [5000, 2 * SEG, 3 * SEG + 7, 9 * SEG],
    "many_spans": [(1 + i % 3) * SEG - i % 7 for i in range(300)],  # more spans than lanes
}


def _data(n: int, seed) -> np.ndarray:
    """1 KiB random then 3 KiB zeros, tiled to n bytes; seed None: all random."""
    if seed is None:
        return np.random.default_rng(99).integers(0, 256, n, dtype=np.uint8)
    unit = np.zeros(SEG, dtype=np.uint8)
    unit[:1024] = np.random.default_rng(seed).integers(0, 256, 1024, dtype=np.uint8)
    return np.tile(unit, -(-n // SEG))[:n]


def _check(src: np.ndarray, spans: list, parser: str):
    """Both references for ``spans`` of ``src``. Returns (comp_lens, containers)."""
    import torch  # before the library: one HIP runtime in the process

    from modal_amd.ops import load_lib

    lib = load_lib(required=True)
    dev = torch.from_numpy(src).cuda()
    n_segs = [-(-ln // SEG) for _off, ln in spans]
    first = np.cumsum([0] + n_segs).tolist()
    stream = torch.cuda.current_stream().cuda_stream
    slots = torch.zeros((2, first[-1] * STRIDE), dtype=torch.uint8, device="cuda")
    lens = torch.full((2, first[-1]), -1, dtype=torch.int32, device="cuda")
    first_d, raw_d, off_d = container.span_tables(spans, first[:-1])
    rc = lib.ma_lz4_compress_spans(
        dev.data_ptr(), off_d.data_ptr(), raw_d.data_ptr(), first_d.data_ptr(), len(spans),
        first[-1], slots[0].data_ptr(), STRIDE, lens[0].data_ptr(),
        compress.LZ_PARSERS.index(parser), stream,
    )
    assert rc == 0
    per_span = lib.ma_lz4_compress_wave if parser == "wave" else lib.ma_lz4_compress
    for (off, ln), f, n in zip(spans, first, n_segs):
        rc = per_span(
            dev.data_ptr() + off, ln, slots[1].data_ptr() + f * STRIDE,
            lens[1].data_ptr() + f * 4, STRIDE, n, stream,
        )
        assert rc == 0
    assert torch.equal(lens[0], lens[1])
    assert torch.equal(slots[0], slots[1])
    ws = container.Workspace.for_lengths([ln for _off, ln in spans], compress.HEADER_FIXED)
    got = compress.compress_spans_gpu(lib, dev.data_ptr(), spans, ws, parser)
    for (off, ln), z in zip(spans, got):
        if z is not None:
            assert compress.decompress_buffer_cpu(bytes(z)) == src[off : off + ln].tobytes()
    return lens[0].cpu().numpy(), got


@pytest.mark.parametrize("parser", compress.LZ_PARSERS)
@pytest.mark.parametrize("case", CASES)
def test_spans_are_the_per_span_launches(case, parser):
    lengths = CASES[case]
    scattered = case == "scattered"
    offs, at = [0] * len(lengths), 0
    for i in reversed(range(len(lengths))) if scattered else range(len(lengths)):
        offs[i] = at
        at += lengths[i] + (SEG + 13 if scattered else 0)
    src = np.zeros(at, dtype=np.uint8)
    for i, (off, ln) in enumerate(zip(offs, lengths)):
        src[off : off + ln] = _data(ln, None if scattered and i == 1 else i)
    comp_lens, got = _check(src, list(zip(offs, lengths)), parser)
    kept = [z is not None for z in got]
    if scattered:  # the random span: every slot raw, no container
        assert kept == [True, False, True, True] and not comp_lens[2:4].any()
    else:
        assert all(kept) and comp_lens[0] > 0


@pytest.mark.parametrize("parser", compress.LZ_PARSERS)
def test_a_window_and_one_segment_more(parser):
    src = _data(MiB, 5)  # 64 spans over the same 1 MiB and one of a segment: 16384 + 1 slots
    comp_lens, got = _check(src, [(0, MiB)] * 64 + [(0, SEG)], parser)
    assert comp_lens.all() and all(z is not None for z in got)


def test_no_spans_launches_nothing_and_a_bad_parser_is_refused():
    import torch

    from modal_amd.ops import load_lib

    lib = load_lib(required=True)
    assert lib.ma_lz4_compress_spans(0, 0, 0, 0, 0, 0, 0, STRIDE, 0, 0, 0) == 0
    assert lib.ma_lz4_compress_spans(0, 0, 0, 0, 0, 0, 0, STRIDE, 0, 2, 0) == 1  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert compress.compress_spans_gpu(lib, 0, [], None) == []


@pytest.mark.parametrize("parser", compress.LZ_PARSERS)
@pytest.mark.parametrize("block_size", (64 * 1024, MiB))  # below COMPRESS_MIN: raw; at it: LZ4
def test_encode_tensor_round_trips(block_size, parser):
    import torch

    raw = _data(3 * block_size, 3)
    t = torch.from_numpy(raw).cuda()
    blocks = devcodec.encode_tensor(t, block_size=block_size, lz_parser=parser)
    assert [b.compressed for b in blocks] == [block_size == MiB] * 3
    host = devcodec.encode_host(raw.tobytes(), block_size=block_size, lz_parser=parser)
    assert devcodec.decode_host(blocks) == devcodec.decode_host(host) == raw.tobytes()
    assert [bytes(b.payload) for b in blocks] == [bytes(b.payload) for b in host]
    back = torch.zeros_like(t)
    devcodec.decode_tensor(blocks, back, verify=True)
    assert torch.equal(back, t)

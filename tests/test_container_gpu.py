"""The layer both codecs share (ops/container.py, csrc/malz_common.h) on the
GPU: grids of more rows than one launch takes, for either assemble kernel
and the MAFP10 histogram and encode kernels; the encoder's tail under either
header size with declined spans in the middle; runs of one codec in a
snapshot of mixed blocks. Every comparison is exact, against numpy models
that share no code with the kernels, in buffers with canaries around them."""

from __future__ import annotations

import hashlib
import struct

import numpy as np
import pytest

import digest_corpus
import fp_corpus as fc
import lz4_corpus

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 4096
N_ROWS = 65537  # MAX_GRID_Y + 2: a second launch of two rows
KiB = 1024


def _feature():
    """torch first (it brings the HIP runtime the library links against),
    then the library. Raises where either is missing."""
    import torch  # noqa: F401

    from modal_amd.ops import load_lib

    lib = load_lib(required=True)
    for symbol in ("ma_malz_plan", "ma_malz_assemble", "ma_fpz_encode", "ma_fpz_assemble"):
        getattr(lib, symbol)
    return lib


def _upload(parts: list, residue: int):
    """One device buffer with every part at an offset that is ``residue`` mod
    16; returns (tensor, [(offset, length)])."""
    import torch

    spans, end = [], 0
    for data in parts:
        off = -(-end // 16) * 16 + residue
        spans.append((off, len(data)))
        end = off + len(data)
    host = np.full(end + 16, CANARY, dtype=np.uint8)
    for (off, ln), data in zip(spans, parts):
        host[off : off + ln] = np.frombuffer(data, dtype=np.uint8)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf, spans


def test_malz_assemble_past_one_grid():
    """65 537 blocks of one raw 8-byte segment, every fifth one skipped, the
    last among them: the second launch assembles block 65 535 and nothing
    else, and the whole output image is as numpy builds it."""
    import torch

    lib = _feature()
    n = N_ROWS
    src = np.random.default_rng(21).integers(0, 256, 128, dtype=np.uint8)
    src_off = (np.arange(n, dtype=np.int64) * 7) % 113  # every residue mod 16
    assert set((src_off % 16).tolist()) == set(range(16)) and src_off.max() + 8 <= len(src)
    skipped = np.arange(n) % 5 == 1
    assert skipped[n - 1] and not skipped[n - 2]
    size = 18 + 4 + 8
    out_off = np.where(skipped, -1, GUARD + 3 + (np.cumsum(~skipped) - 1) * size).astype(np.int64)
    total = GUARD + 3 + int((~skipped).sum()) * size + GUARD
    kept = np.flatnonzero(~skipped)
    rows = np.empty((len(kept), size), dtype=np.uint8)
    rows[:, :22] = np.frombuffer(b"MALZ41" + struct.pack("<QII", 8, 1, 0), dtype=np.uint8)
    rows[:, 22:] = src[src_off[kept][:, None] + np.arange(8)]
    image = np.full(total, CANARY, dtype=np.uint8)
    image[out_off[kept][:, None] + np.arange(size)] = rows

    dev = {
        name: torch.from_numpy(arr).cuda()
        for name, arr in (
            ("src", src), ("src_off", src_off), ("out_off", out_off),
            ("comp_lens", np.zeros(n, dtype=np.int32)), ("first", np.arange(n, dtype=np.int32)),
            ("raw_lens", np.full(n, 8, dtype=np.int64)),
        )
    }
    stride_buf = torch.zeros(16, dtype=torch.uint8, device="cuda")  # nothing is compressed
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    seg_off = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    payload = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.ma_malz_plan(
        dev["comp_lens"].data_ptr(), dev["first"].data_ptr(), dev["raw_lens"].data_ptr(),
        seg_off.data_ptr(), payload.data_ptr(), n, stream,
    )
    assert rc == 0
    assert not seg_off.cpu().numpy().any() and (payload.cpu().numpy() == 8).all()
    rc = lib.ma_malz_assemble(
        dev["src"].data_ptr(), dev["src_off"].data_ptr(), stride_buf.data_ptr(), 4352,
        dev["comp_lens"].data_ptr(), seg_off.data_ptr(), dev["first"].data_ptr(),
        dev["raw_lens"].data_ptr(), out.data_ptr(), dev["out_off"].data_ptr(), n, stream,
    )
    assert rc == 0
    got = out.cpu().numpy()
    wrong = np.flatnonzero(got != image)
    assert len(wrong) == 0, f"first wrong byte at {wrong[0]}, block {(wrong[0] - GUARD - 3) // size} kept"


def test_fpz_encoder_past_one_grid():
    """One MAFP10 encoder call over 65 537 tiny spans, four patterns in
    rotation: the histogram, encode and assemble kernels each take a second
    launch, whose last span is kept."""
    from modal_amd.ops import fpcodec

    lib = _feature()

    def elems(tops: list) -> bytes:
        return bytes(x for i, t in enumerate(tops) for x in (0x10 + i, t))

    patterns = [
        elems([0x3F] * 4),  # 8 bytes, one top byte: b = 1, no escape
        elems([0x3F] * 7 + [0x40]),  # 16 bytes, two top values: b = 1, one escape
        elems(list(range(0x38, 0x40))),  # 16 bytes, eight distinct top bytes
        elems([0x3F] * 3) + b"\x3f",  # 7 bytes: no whole number of elements, stays raw
    ]
    models = [fpcodec.compress_buffer_cpu(p, 2) for p in patterns]
    # header 276 + table 4 + low bytes + (1 + code bytes + escapes)
    assert [z and len(z) for z in models] == [280 + 4 + 2, 280 + 8 + 3, 280 + 8 + 5, None]
    buf, placed = _upload(patterns, 2)
    spans = [placed[i % 4] for i in range(N_ROWS)]
    assert models[(N_ROWS - 1) % 4] is not None
    ws = fpcodec.Workspace.for_lengths([ln for _off, ln in spans], fpcodec.HEADER_FIXED)
    got = fpcodec.compress_spans_gpu(lib, buf.data_ptr(), spans, 2, ws)
    assert len(got) == N_ROWS
    for i, z in enumerate(got):
        want = models[i % 4]
        assert (z is None) == (want is None) and (want is None or bytes(z) == want), f"span {i}"


def _tail_inputs(gauss) -> list:
    """Five spans: 4097, 8192 and 12 290 bytes that compress, a 4096-byte and
    one more span of random bytes at 1 and 3 that must not."""
    return [
        gauss(4097), fc.random_bytes(4096, seed=91), gauss(8192),
        fc.random_bytes(5000, seed=92), gauss(12290),
    ]


def _assert_tail(got: list, want: list) -> None:
    assert [z is None for z in want] == [False, True, False, True, False]
    for j, (z, w) in enumerate(zip(got, want)):
        assert (z is None) == (w is None) and (w is None or bytes(z) == w), f"span {j}"


def test_shared_tail_under_both_codecs():
    """``finish_containers`` with either header size: ``out_off`` -1 in the
    middle, the sizes and the slices of the dense buffer, spans of 1, 2, 3
    and 4 segments with tails of 1 and 2 bytes."""
    from modal_amd.ops import compress, fpcodec

    lib = _feature()
    text = b"".join(lz4_corpus.SEGMENTS[k] for k in ("ascii_text", "tiled_1k", "period3", "ascii_text"))
    parts = _tail_inputs(lambda n: text[:n])
    buf, spans = _upload(parts, 1)
    ws = compress.Workspace.for_lengths([len(p) for p in parts], compress.HEADER_FIXED)
    got = compress.compress_spans_gpu(lib, buf.data_ptr(), spans, ws)
    _assert_tail(got, [digest_corpus.expected_container(p) for p in parts])

    parts = _tail_inputs(lambda n: fc.bf16_gauss(n, seed=n))
    buf, spans = _upload(parts, 2)
    ws = fpcodec.Workspace.for_lengths([len(p) for p in parts], fpcodec.HEADER_FIXED)
    got = fpcodec.compress_spans_gpu(lib, buf.data_ptr(), spans, 2, ws)
    _assert_tail(got, [fpcodec.compress_buffer_cpu(p, 2) for p in parts])


def test_decode_runs_of_one_codec_in_a_mixed_snapshot():
    """LZ4, LZ4, MAFP10, MAFP10, raw, LZ4: three runs, cut where the codec
    changes and at the raw block, decoded into a destination at 5 mod 16."""
    import torch

    from modal_amd.ops import compress, devcodec, fpcodec

    _feature()
    n = 64 * KiB
    unit = np.random.default_rng(5).integers(0, 256, 1024, dtype=np.uint8).tobytes()
    raws = [
        unit * 64, unit[::-1] * 64, fc.bf16_gauss(n, seed=81), fc.bf16_gauss(n, seed=82),
        fc.random_bytes(n, seed=83), (unit[:512] + bytes(512)) * 64,
    ]
    stored = [
        compress.compress_buffer_cpu(raws[0]), compress.compress_buffer_cpu(raws[1]),
        fpcodec.compress_buffer_cpu(raws[2], 2), fpcodec.compress_buffer_cpu(raws[3], 2),
        None, compress.compress_buffer_cpu(raws[5]),
    ]
    assert [z is None for z in stored] == [False, False, False, False, True, False]
    assert [z[:6] for z in stored if z] == [b"MALZ41"] * 2 + [b"MAFP10"] * 2 + [b"MALZ41"]
    blocks = [
        (hashlib.sha256(raw).hexdigest(), n, raw if z is None else z, z is not None)
        for raw, z in zip(raws, stored)
    ]
    whole = torch.full((GUARD + 6 * n + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    at = GUARD + 5
    devcodec.decode_to_device(blocks, whole.data_ptr() + at, 6 * n, verify=True)
    got = whole.cpu().numpy()
    assert got[at : at + 6 * n].tobytes() == b"".join(raws)
    assert (got[:at] == CANARY).all() and (got[at + 6 * n :] == CANARY).all()

    # 64 KiB is 16 segments and the run starts at block 2: segment 1 of block
    # 3 is number 17 of the run
    broken = list(blocks)
    broken[3] = blocks[3][:2] + (fc.break_segment(stored[3], 1), True)
    with pytest.raises(ValueError) as err:
        devcodec.decode_to_device(broken, whole.data_ptr() + at, 6 * n, verify=True)
    assert str(err.value) == "snapshot blocks 2..3: MAFP10 container corrupt at segment 17 of the run"

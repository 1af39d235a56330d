"""Conformance of the LZ4 segment codec and the MALZ41 assembly against the
corpus in tests/lz4_corpus.py: the compressor kernel against an exact model,
every decoder (kernel, C++ core, utils/lz4ref.py) on hand-assembled blocks
and on one malformed block per rejection branch, the first-corrupt-segment
report, and the assemble kernel's wave copy at every alignment. Every
comparison is exact, byte for byte."""

from __future__ import annotations

import functools
import struct
from typing import NamedTuple, Optional

import numpy as np
import pytest

import lz4_corpus as corpus
from lz4_corpus import MALFORMED, SEG, SEGMENTS, WELL_FORMED, model_compress, strict_decode
from modal_amd.ops import compress
from modal_amd.utils import lz4ref

CANARY = 0xA5
GUARD = 4096  # canary bytes either side of every device buffer under test
STRIDE = compress.OUT_STRIDE
SHORT_GPU_LENGTHS = (1, 4, 8, 9, 12, 13, 14, 16, 17, 4095)
FULL_BLOCKS = [name for name, (_enc, raw) in WELL_FORMED.items() if len(raw) == SEG]


class Seg(NamedTuple):
    """One segment of a container under test. ``raw`` is None for a corrupt
    one, whose decoded bytes are unspecified."""

    payload: bytes
    comp_len: int
    raw_len: int
    raw: Optional[bytes]


def _raw_seg(seed: int, n: int = SEG) -> Seg:
    data = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    return Seg(data, 0, n, data)


def _block_seg(name: str) -> Seg:
    enc, raw = WELL_FORMED[name]
    return Seg(enc, len(enc), len(raw), raw)


def _bad_seg(name: str) -> Seg:
    enc, raw_len = MALFORMED[name]
    return Seg(enc, len(enc), raw_len, None)


def _good_segs(n: int, seed: int) -> list:
    """n full segments: hand-assembled blocks and raw ones, alternating."""
    return [
        _raw_seg(seed + i) if i % 2 else _block_seg(FULL_BLOCKS[(seed + i // 2) % len(FULL_BLOCKS)])
        for i in range(n)
    ]


def _with_bad(name: str, index: int, n: int, seed: int) -> list:
    """n segments with the malformed block ``name`` at ``index``; a block for
    a short segment can only be the last one."""
    segs = _good_segs(n, seed)
    segs[index] = _bad_seg(name)
    assert all(s.raw_len == SEG for s in segs[:-1])
    return segs


def _container(segs: list) -> bytes:
    raw_len = sum(s.raw_len for s in segs)
    return compress._header(raw_len, [s.comp_len for s in segs]) + b"".join(
        s.payload for s in segs
    )


@pytest.fixture(params=["core", "python"])
def backend(request, monkeypatch):
    """decompress_buffer_cpu over the C++ core, then over utils/lz4ref.py."""
    if request.param == "python":
        monkeypatch.setattr(compress, "_native_core", lambda: None)
    else:
        assert compress._native_core() is not None, "the native core is not built"
    return request.param


# ---------------------------------------------------------------------------
# CPU: compressor model
# ---------------------------------------------------------------------------


def _model_inputs() -> dict:
    inputs = dict(SEGMENTS)
    for n in corpus.SHORT_LENGTHS:
        inputs[f"zeros[:{n}]"] = bytes(n)
    return inputs


def test_model_blocks_are_strictly_valid():
    for name, seg in _model_inputs().items():
        block = model_compress(seg)
        assert strict_decode(block, len(seg)) == seg, name
        assert lz4ref.decompress_block(block, len(seg)) == seg, name
        # the production slot never makes the parser give up, a small one
        # either does or changes nothing
        assert model_compress(seg, max_out=STRIDE) == block, name
        assert model_compress(seg, max_out=64) in (b"", block), name


def test_model_shapes_the_corpus_relies_on():
    # the one long match is cut by the data and by the last-literals rule at
    # the same byte: a literal run, one match, five literals
    block = model_compress(SEGMENTS["match_to_len_minus_5"])
    assert block[-6] == 0x50 and block[-5:] == SEGMENTS["match_to_len_minus_5"][-5:]
    assert len(block) < 128
    # below 13 bytes nothing may match; at 14 zeros the first match appears
    for n in (1, 4, 8, 9, 12, 13):
        assert model_compress(bytes(n)) == bytes([n << 4]) + bytes(n)
    assert model_compress(bytes(14)) == b"\x14\x00\x01\x00\x50" + bytes(5)
    # the skip through miss runs is part of the model: without it the parse
    # of these differs, so a model that steps by one is not the kernel
    for name in ("tiled_1k", "random_then_zeros", "planted_repeats"):
        seg = SEGMENTS[name]
        dense = lz4ref.compress_block(seg, accel=False)
        assert dense != model_compress(seg), name
        assert strict_decode(dense, SEG) == seg, name


# ---------------------------------------------------------------------------
# CPU: decoders on hand-assembled and malformed blocks
# ---------------------------------------------------------------------------


def test_corpus_covers_what_it_claims():
    """The well-formed blocks decode (strictly, where the end rules allow) to
    what their builder says, and every malformed one is refused."""
    for name, (enc, raw) in WELL_FORMED.items():
        if name in corpus.BREAKS_END_RULES:
            with pytest.raises(ValueError):
                strict_decode(enc, len(raw))
        else:
            assert strict_decode(enc, len(raw)) == raw, name
    enc, raw = corpus.LITERALS_ONLY_FULL
    assert strict_decode(enc, SEG) == raw and len(enc) > SEG
    for name, (enc, raw_len) in MALFORMED.items():
        with pytest.raises(ValueError):
            strict_decode(enc, raw_len)


def test_well_formed_blocks_decode(backend):
    from modal_amd.ops import devcodec

    for name in WELL_FORMED:
        seg = _block_seg(name)
        blob = _container([seg])
        compress.validate_container(blob)
        assert compress.decompress_buffer_cpu(blob) == seg.raw, name
        assert lz4ref.decompress_block(seg.payload, seg.raw_len) == seg.raw, name
        block = ("", seg.raw_len, blob, True)
        assert devcodec.decode_host([block], verify=False) == seg.raw, name
    # all of them in one container: the core decodes segments on threads
    segs = _good_segs(2 * len(FULL_BLOCKS), seed=0) + [_block_seg("literals_only")]
    assert compress.decompress_buffer_cpu(_container(segs)) == b"".join(s.raw for s in segs)


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_blocks_raise_value_error(backend, name):
    from modal_amd.ops import devcodec

    bad = _bad_seg(name)
    # alone, and late in a container long enough for the core's thread pool
    for segs in ([bad], _with_bad(name, 11, 12, seed=3)):
        blob = _container(segs)
        raw_len, comp_lens, _off = compress.validate_container(blob)  # reaches the codec
        assert raw_len == sum(s.raw_len for s in segs) and len(comp_lens) == len(segs)
        with pytest.raises(ValueError, match="LZ4 container corrupt"):
            compress.decompress_buffer_cpu(blob)
        with pytest.raises(ValueError, match="LZ4 container corrupt"):
            devcodec.decode_host([("", raw_len, blob, True)], verify=False)
    with pytest.raises(ValueError, match="^LZ4: "):
        lz4ref.decompress_block(bad.payload, bad.raw_len)


# ---------------------------------------------------------------------------
# CPU: the assemble test's layout
# ---------------------------------------------------------------------------

ASM_STRIDE = 4353  # odd, so slot addresses walk every residue mod 16
ASM_SEED = 1
SRC_RESIDUES = (5, 0, 10, 15, 4, 1)  # of blk_src_off and blk_out_off, mod 16
OUT_RESIDUES = (3, 0, 9, 14, 6, 13)


class AsmCase(NamedTuple):
    n_segs: list
    raw_lens: np.ndarray
    first: np.ndarray
    comp_lens: np.ndarray
    stride_buf: np.ndarray
    src: np.ndarray
    src_off: np.ndarray
    seg_off: np.ndarray
    payload: np.ndarray
    out_off: np.ndarray
    image: np.ndarray  # what the whole out buffer must hold afterwards
    copies: list  # (source address mod 16, destination address mod 16, length)


@functools.lru_cache(maxsize=None)
def _assemble_case(seed: int = ASM_SEED) -> AsmCase:
    """Synthetic plan/assemble inputs and their oracle, all numpy: device
    buffers are taken to start 16-aligned (the GPU test asserts it)."""
    rng = np.random.default_rng(seed)
    n_segs = [1, 7, 40, 16, 23, 12]
    tails = [1, 4095, SEG, 1, 4095, SEG]
    skipped = 3
    raw_lens = np.array([(n - 1) * SEG + t for n, t in zip(n_segs, tails)], dtype=np.int64)
    first = (np.cumsum(n_segs) - n_segs).astype(np.int32)
    total = int(sum(n_segs))
    special = np.array([0, 1, 2, 15, 16, 17, 31, 33, 4095])
    comp_lens = np.where(
        rng.random(total) < 0.6, rng.choice(special, total), rng.integers(1, SEG, total)
    ).astype(np.int32)
    for b in (0, 1, 4):  # raw last segments of 1 and 4095 bytes
        comp_lens[first[b] + n_segs[b] - 1] = 0
    stride_buf = rng.integers(0, 256, total * ASM_STRIDE + 64, dtype=np.uint8)

    src_off, cursor = [], 0
    for b in range(len(n_segs)):
        cursor += int(rng.integers(1, 64))
        cursor += (SRC_RESIDUES[b] - cursor) % 16
        src_off.append(cursor)
        cursor += int(raw_lens[b])
    src = rng.integers(0, 256, cursor + 64, dtype=np.uint8)

    seg_off = np.empty(total, dtype=np.int64)
    payload = np.empty(len(n_segs), dtype=np.int64)
    effs = []
    for b, n in enumerate(n_segs):
        eff = compress.effective_lens(comp_lens[first[b] : first[b] + n], int(raw_lens[b]))
        effs.append(eff)
        seg_off[first[b] : first[b] + n] = np.cumsum(eff) - eff
        payload[b] = eff.sum()

    out_off, cursor = [], 0
    sizes = [compress.HEADER_FIXED + 4 * n + int(p) for n, p in zip(n_segs, payload)]
    for b in range(len(n_segs)):
        cursor += int(rng.integers(1, 48))
        cursor += (OUT_RESIDUES[b] - cursor) % 16
        out_off.append(-1 if b == skipped else cursor)
        cursor += sizes[b]  # the skipped block's region stays untouched
    image = np.full(cursor + 100, CANARY, dtype=np.uint8)

    copies = []
    for b, n in enumerate(n_segs):
        if out_off[b] < 0:
            continue
        cl = comp_lens[first[b] : first[b] + n]
        parts = [b"MALZ41", struct.pack("<QI", int(raw_lens[b]), n), cl.astype("<u4").tobytes()]
        at = out_off[b] + compress.HEADER_FIXED + 4 * n
        for s in range(n):
            length = int(effs[b][s])
            start = (first[b] + s) * ASM_STRIDE if cl[s] else src_off[b] + s * SEG
            parts.append((stride_buf if cl[s] else src)[start : start + length].tobytes())
            copies.append((int(start % 16), int((at + seg_off[first[b] + s]) % 16), length))
        blob = b"".join(parts)
        assert len(blob) == sizes[b]
        compress.validate_container(blob)
        image[out_off[b] : out_off[b] + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    return AsmCase(
        n_segs, raw_lens, first, comp_lens, stride_buf, src, np.array(src_off, dtype=np.int64),
        seg_off, payload, np.array(out_off, dtype=np.int64), image, copies,
    )


def _check_copy_coverage(copies: list) -> None:
    """Every path of the kernel's wave copy is reached. After the byte lanes
    of the head (up to the destination's 16-byte boundary) the body is fed by
    dwordx4 loads, dword loads, or the funnel at a byte shift of 1, 2 or 3,
    by where the source then stands."""
    assert {s for s, _d, n in copies if n >= 32} == set(range(16))
    assert {d for _s, d, _n in copies} == set(range(16))
    assert any(n < (16 - d) % 16 for _s, d, n in copies)
    body_paths = set()
    for s, d, n in copies:
        head = min((16 - d) % 16, n)
        if (n - head) >= 16:
            at = (s + head) % 16
            body_paths.add("x4" if at == 0 else ("dword", "funnel1", "funnel2", "funnel3")[at % 4])
    assert body_paths == {"x4", "dword", "funnel1", "funnel2", "funnel3"}


def test_assemble_layout_covers_every_alignment():
    case = _assemble_case()
    _check_copy_coverage(case.copies)
    assert -1 in case.out_off and {int(r % SEG) for r in case.raw_lens} == {0, 1, 4095}
    assert tuple(int(o % 16) for o in case.src_off) == SRC_RESIDUES
    assert [int(o % 16) for o in case.out_off if o >= 0] == [3, 0, 9, 6, 13]


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------


def _feature():
    """The ops library with the kernels under test. Raises where it is
    missing, so a build without it fails these tests, not skips them."""
    # torch first: loaded after the library it brings a second HIP runtime
    # into the process, and the library's launches then find no device
    import torch  # noqa: F401

    from modal_amd.ops import load_lib

    lib = load_lib(required=True)
    for symbol in ("ma_lz4_compress", "ma_lz4_decompress", "ma_malz_plan", "ma_malz_assemble"):
        getattr(lib, symbol)
    return lib


def _guarded(nbytes: int, fill: int = CANARY):
    """A device buffer of nbytes inside a larger one, GUARD canary bytes
    either side. Returns (whole tensor, interior view)."""
    import torch

    whole = torch.full((GUARD + nbytes + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    inner = whole[GUARD : GUARD + nbytes]
    if fill != CANARY:
        inner.fill_(fill)
    return whole, inner


def _guards_intact(whole) -> bool:
    host = whole.cpu().numpy()
    return bool((host[:GUARD] == CANARY).all() and (host[-GUARD:] == CANARY).all())


def _gpu_decode(lib, segs: list):
    """One decompress launch over ``segs``. Returns (what decompress_run_gpu
    returned, the decoded bytes, whether the canaries around dst survived)."""
    import torch

    raw_len = sum(s.raw_len for s in segs)
    comp = torch.from_numpy(
        np.frombuffer(b"".join(s.payload for s in segs) + bytes(64), dtype=np.uint8).copy()
    ).cuda()
    whole, dst = _guarded(raw_len)
    status = compress.decompress_run_gpu(
        lib, comp.data_ptr(), [(raw_len, [s.comp_len for s in segs])], dst.data_ptr()
    )
    return status, dst.cpu().numpy().tobytes(), _guards_intact(whole)


def _assert_good_segments_exact(segs: list, got: bytes) -> None:
    pos = 0
    for i, s in enumerate(segs):
        if s.raw is not None:
            assert got[pos : pos + s.raw_len] == s.raw, f"segment {i}"
        pos += s.raw_len
    assert pos == len(got)


@pytest.mark.gpu
def test_gpu_decoder_well_formed():
    lib = _feature()
    segs = []
    for i, name in enumerate(FULL_BLOCKS):
        segs += [_block_seg(name), _raw_seg(900 + i)]
    enc, raw = corpus.LITERALS_ONLY_FULL  # too long for a container, fine for the kernel
    segs += [Seg(enc, len(enc), SEG, raw), _raw_seg(990, 1)]
    status, got, guards = _gpu_decode(lib, segs)
    assert status == 0
    _assert_good_segments_exact(segs, got)
    assert guards
    # the short literals-only block, as a container's last segment
    segs = _good_segs(3, seed=1) + [_block_seg("literals_only")]
    blob = _container(segs)
    assert compress.decompress_buffer_gpu(blob) == b"".join(s.raw for s in segs)


# index of the bad segment and segment count per malformed block; the short
# segment's block has to be the last one
BAD_PLACEMENT = {
    "literal_run_off_end": (0, 3),
    "literals_overrun_source": (1, 2),
    "literals_overrun_destination": (63, 70),
    "truncated_offset": (64, 65),
    "offset_zero": (255, 256),
    "offset_past_start": (256, 258),
    "match_at_position_0": (257, 258),
    "match_run_off_end": (5, 300),
    "match_overruns_destination_by_1": (129, 131),
    "one_byte_short": (2, 5),
    "short_segment_one_byte_over": (40, 41),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_gpu_decoder_names_the_malformed_segment(name):
    lib = _feature()
    index, n = BAD_PLACEMENT[name]
    segs = _with_bad(name, index, n, seed=index)
    status, got, guards = _gpu_decode(lib, segs)
    assert status == index + 1
    _assert_good_segments_exact(segs, got)
    assert guards


@pytest.mark.gpu
def test_gpu_corrupt_segment_through_the_public_api():
    import torch

    from modal_amd.ops import devcodec

    _feature()
    segs = _with_bad("offset_past_start", 6, 9, seed=2)
    blob = _container(segs)
    with pytest.raises(ValueError, match="corrupt at segment 6$"):
        compress.decompress_buffer_gpu(blob)
    with pytest.raises(ValueError, match="corrupt at segment 6$"):
        compress.decompress_buffer(blob)
    # as the second block of a snapshot: the run's segments count on from the
    # first block's four
    good = _good_segs(4, seed=5)
    blocks = [
        ("", 4 * SEG, _container(good), True),
        ("", sum(s.raw_len for s in segs), blob, True),
    ]
    out = torch.empty(13 * SEG, dtype=torch.uint8, device="cuda")
    with pytest.raises(
        ValueError, match=r"snapshot blocks 0\.\.1: LZ4 container corrupt at segment 10 of the run"
    ):
        devcodec.decode_tensor(blocks, out, verify=False)


@pytest.mark.gpu
def test_gpu_decoder_reports_the_first_corrupt_segment():
    """Bad segments at 3 and 300, in different workgroups: the answer is 4
    whichever lane reports last. A wave reports when its slowest lane is
    done, so the launch runs three times: as the segments come, with segment
    3's wave the quick one (long 8-byte match copies against byte-wise raw
    copies), and with segment 300's."""
    lib = _feature()
    quick = _block_seg("offset_is_position")
    for quick_wave in (None, range(0, 64), range(256, 302)):
        segs = _good_segs(302, seed=7)
        if quick_wave is not None:
            slow = [_raw_seg(2000 + i) for i in range(302)]
            segs = [quick if i in quick_wave else slow[i] for i in range(302)]
        segs[3] = _bad_seg("offset_zero")
        segs[300] = _bad_seg("offset_zero" if quick_wave else "one_byte_short")
        status, got, guards = _gpu_decode(lib, segs)
        assert status == 4
        assert compress.corrupt_message(status) == "LZ4 container corrupt at segment 3"
        _assert_good_segments_exact(segs, got)
        assert guards


@functools.lru_cache(maxsize=None)
def _compress_inputs() -> tuple:
    """Every corpus segment, filled up with variants to 131 so that a second
    workgroup (128 lanes each) holds compressible segments too; with every
    segment's model block. Computed once, read-only."""
    segs = list(SEGMENTS.values())
    while len(segs) < 131:
        segs.append(corpus.variant(len(segs)))
    assert len(set(segs[126:130])) == 4
    blocks = [model_compress(s) for s in segs]
    assert all(0 < len(blocks[i]) < SEG for i in (127, 128, 129))
    return tuple(segs), tuple(blocks)


def _gpu_compress(lib, data: bytes, out_stride: int, fill: int):
    """One compress launch over ``data`` from a source pointer misaligned by
    one. Returns (comp_lens, slot bytes, whether the slot canaries survived)."""
    import torch

    n_seg = -(-len(data) // SEG)
    src = torch.from_numpy(np.frombuffer(bytes(1) + data, dtype=np.uint8).copy()).cuda()[1:]
    assert src.data_ptr() % 4 == 1
    whole, slots = _guarded(n_seg * out_stride, fill)
    lens = torch.full((n_seg,), -1, dtype=torch.int32, device="cuda")
    rc = lib.ma_lz4_compress(
        src.data_ptr(), len(data), slots.data_ptr(), lens.data_ptr(), out_stride, n_seg,
        torch.cuda.current_stream().cuda_stream,
    )
    assert rc == 0
    return lens.cpu().numpy(), slots.cpu().numpy(), _guards_intact(whole)


def _assert_matches_model(segs, blocks, comp_lens, slots, out_stride) -> None:
    want = [len(b) if 0 < len(b) < len(s) else 0 for s, b in zip(segs, blocks)]
    assert comp_lens.tolist() == want
    for i, (block, clen) in enumerate(zip(blocks, want)):
        got = slots[i * out_stride : i * out_stride + clen].tobytes()
        assert got == block[:clen], f"segment {i}"


@pytest.mark.gpu
def test_gpu_compressor_matches_the_model():
    lib = _feature()
    segs, blocks = _compress_inputs()
    data = b"".join(segs)
    first = _gpu_compress(lib, data, STRIDE, 0x00)
    second = _gpu_compress(lib, data, STRIDE, 0xEE)
    for comp_lens, slots, guards in (first, second):
        # bytes past a slot's block are unspecified: only the defined ones count
        _assert_matches_model(segs, blocks, comp_lens, slots, STRIDE)
        assert guards
    assert any(c == 0 for c in first[0]) and sum(c > 0 for c in first[0]) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("n", SHORT_GPU_LENGTHS)
def test_gpu_compressor_short_last_segment(n):
    lib = _feature()
    for last in (bytes(n), SEGMENTS["period3"][:n], SEGMENTS["ascii_text"][:n]):
        segs = (SEGMENTS["ascii_text"], last)
        blocks = [model_compress(s) for s in segs]
        comp_lens, slots, guards = _gpu_compress(lib, b"".join(segs), STRIDE, 0x11)
        _assert_matches_model(segs, blocks, comp_lens, slots, STRIDE)
        assert guards


@pytest.mark.gpu
def test_gpu_compressor_small_slot_bails_out_in_bounds():
    lib = _feature()
    small = 64
    segs, blocks = _compress_inputs()
    comp_lens, slots, guards = _gpu_compress(lib, b"".join(segs), small, 0x22)
    assert guards
    for i, (block, clen) in enumerate(zip(blocks, comp_lens.tolist())):
        assert clen in (0, len(block)), f"segment {i}"
        if len(block) > small:
            assert clen == 0, f"segment {i}"
        assert slots[i * small : i * small + clen].tobytes() == block[:clen], f"segment {i}"
    assert comp_lens[0] == len(blocks[0]) and segs[0] == bytes(SEG)  # zeros fit
    # and exactly where the model of the kernel's size estimate gives up
    assert comp_lens.tolist() == [len(model_compress(s, max_out=small)) for s in segs]


@pytest.mark.gpu
def test_gpu_assemble_every_alignment():
    lib = _feature()
    import torch

    case = _assemble_case()
    _check_copy_coverage(case.copies)
    dev = {
        name: torch.from_numpy(getattr(case, name)).cuda()
        for name in ("comp_lens", "first", "raw_lens", "stride_buf", "src", "src_off", "out_off")
    }
    out = torch.full((len(case.image),), CANARY, dtype=torch.uint8, device="cuda")
    for name in ("stride_buf", "src"):
        assert dev[name].data_ptr() % 16 == 0
    assert out.data_ptr() % 16 == 0
    total = len(case.comp_lens)
    seg_off = torch.full((total,), -1, dtype=torch.int64, device="cuda")
    payload = torch.full((len(case.n_segs),), -1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.ma_malz_plan(
        dev["comp_lens"].data_ptr(), dev["first"].data_ptr(), dev["raw_lens"].data_ptr(),
        seg_off.data_ptr(), payload.data_ptr(), len(case.n_segs), stream,
    )
    assert rc == 0
    assert np.array_equal(seg_off.cpu().numpy(), case.seg_off)
    assert np.array_equal(payload.cpu().numpy(), case.payload)
    rc = lib.ma_malz_assemble(
        dev["src"].data_ptr(), dev["src_off"].data_ptr(), dev["stride_buf"].data_ptr(),
        ASM_STRIDE, dev["comp_lens"].data_ptr(), seg_off.data_ptr(), dev["first"].data_ptr(),
        dev["raw_lens"].data_ptr(), out.data_ptr(), dev["out_off"].data_ptr(),
        len(case.n_segs), stream,
    )
    assert rc == 0
    got = out.cpu().numpy()
    wrong = np.flatnonzero(got != case.image)
    assert wrong.size == 0, f"{wrong.size} bytes differ, the first at {wrong[:8].tolist()}"

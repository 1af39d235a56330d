"""The MAFB10 byte-plane codec on the GPU (ops/bytecodec.py +
csrc/bytez.hip): the encoder against the numpy model byte for byte on the
inputs of tests/byte_corpus.py at every source alignment, the decoder into
aligned and misaligned device memory, its status word, and the device block
codec with the hint on. Every comparison is exact."""

from __future__ import annotations

import numpy as np
import pytest

import byte_corpus as bc
from fp_corpus import MiB, random_bytes

pytestmark = pytest.mark.gpu

# whole segments first: their decoded runs stay 16-byte aligned at residue 0
NAMES = sorted(bc.corpus(), key=lambda n: (len(bc.corpus()[n]) % bc.SEG != 0, n))
CANARY = 0xA5


def _feature():
    import torch  # noqa: F401  (brings the HIP runtime the library links against)

    from modal_amd.ops import bytecodec, load_lib

    return bytecodec, load_lib(required=True)  # binds the ma_bytez_* entries or raises


@pytest.fixture(scope="module")
def model() -> dict:
    from modal_amd.ops import bytecodec

    return {name: bytecodec.compress_buffer_cpu(data) for name, data in bc.corpus().items()}


def _upload(parts: list, residue: int):
    """A canary-filled device buffer, every part at ``residue`` mod 16, and the spans."""
    import torch

    spans, end = [], 0
    for data in parts:
        off = -(-end // 16) * 16 + residue
        spans.append((off, len(data)))
        end = off + len(data)
    host = np.full(end + 32, CANARY, dtype=np.uint8)
    for (off, ln), data in zip(spans, parts):
        host[off : off + ln] = np.frombuffer(data, dtype=np.uint8)
    return torch.from_numpy(host).cuda(), spans


@pytest.mark.parametrize("residue", [0, 1, 5, 15])
def test_encoder_matches_the_model_byte_for_byte(model, residue):
    """Every input in ONE call, kept and declined spans side by side."""
    bytecodec, lib = _feature()
    buf, spans = _upload([bc.corpus()[n] for n in NAMES], residue)
    ws = bytecodec.Workspace.for_lengths([ln for _off, ln in spans], bytecodec.HEADER_FIXED)
    got = bytecodec.compress_spans_gpu(lib, buf.data_ptr(), spans, ws)
    assert model["random"] is None and model["e4m3_8k"] is not None
    for name, z in zip(NAMES, got):
        assert (z is None) == (model[name] is None), name
        if z is not None:
            assert bytes(z) == model[name], f"{name}: container differs from the model"


def _decode_run(blobs: list, residue: int):
    """Payloads back to back on the device, decoded to ``residue`` mod 16 in a
    canary buffer; returns (status, the buffer, the destination's index in it)."""
    import torch

    bytecodec, lib = _feature()
    headers = [bytecodec.validate_container(z) for z in blobs]
    comp, spans = _upload([b"".join(z[h.payload_off :] for z, h in zip(blobs, headers))], 5)
    total = sum(h.raw_len for h in headers)
    dst = torch.full((total + 64,), CANARY, dtype=torch.uint8, device="cuda")
    lo = 16 + residue
    status = bytecodec.decompress_run_gpu(
        lib, comp.data_ptr() + spans[0][0], headers, dst.data_ptr() + lo
    )
    return status, dst.cpu().numpy(), lo


@pytest.mark.parametrize("residue", [0, 5])
def test_decoder_writes_every_kept_container_in_one_run(model, residue):
    names = [n for n in NAMES if model[n] is not None]
    raw = b"".join(bc.corpus()[n] for n in names)
    status, out, lo = _decode_run([model[n] for n in names], residue)
    assert status == 0
    assert out[lo : lo + len(raw)].tobytes() == raw
    assert (out[:lo] == CANARY).all() and (out[lo + len(raw) :] == CANARY).all()


@pytest.mark.parametrize("how", ["width_0", "width_8", "one_escape_too_few"])
def test_decoder_reports_the_first_corrupt_segment_and_leaves_it_alone(model, how):
    """Element 0 of every segment of ``sprinkled`` is an escape: clearing its
    code leaves one escape fewer than seg_len holds."""
    names = ["e4m3_8k", "sprinkled", "len8292"]
    blobs = [model[n] for n in names]
    seg = 3  # of sprinkled; segments 0 and 1 of the run are e4m3_8k's
    at = bc.segment_offsets(blobs[1])[seg]
    bad = bytearray(blobs[1])
    if how == "one_escape_too_few":
        assert bad[at + 1] & (2 ** bad[at] - 1) == 2 ** bad[at] - 1
        bad[at + 1] &= 256 - 2 ** bad[at]
    else:
        bad[at] = 0 if how == "width_0" else 8
    later = bytearray(blobs[2])
    later[bc.segment_offsets(blobs[2])[0]] = 0  # a later corrupt segment must not win
    status, out, lo = _decode_run([blobs[0], bytes(bad), bytes(later)], 0)
    assert status == 1 + 2 + seg
    first = lo + 2 * bc.SEG + seg * bc.SEG
    assert (out[first : first + bc.SEG] == CANARY).all()
    good = bc.corpus()["e4m3_8k"] + bc.corpus()["sprinkled"][: seg * bc.SEG]
    assert out[lo:first].tobytes() == good


def test_device_codec_gives_byte_lz4_and_raw_blocks():
    import torch

    _feature()
    from modal_amd.ops import bytecodec, compress, devcodec

    unit = np.random.default_rng(11).integers(0, 256, 1024, dtype=np.uint8)
    raw = bc.fp8(MiB, "float8_e4m3fn", 7) + np.tile(unit, 1024).tobytes() + random_bytes(MiB, 8)
    raw += bc.fp8(64 * 1024, "float8_e5m2", 9)  # a short last block: too small for LZ4, not for MAFB10
    src = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    blocks = devcodec.encode_device(src.data_ptr(), len(raw), block_size=MiB, elem_size=1)
    assert [b.compressed for b in blocks] == [True, True, False, True]
    assert bytes(blocks[0].payload) == bytecodec.compress_buffer_cpu(raw[:MiB])
    assert bytes(blocks[3].payload) == bytecodec.compress_buffer_cpu(raw[3 * MiB :])
    assert compress.is_compressed(blocks[1].payload)
    assert bytes(blocks[2].payload) == raw[2 * MiB : 3 * MiB]
    host = devcodec.encode_host(raw, block_size=MiB, elem_size=1)
    assert [b.digest for b in blocks] == [b.digest for b in host]
    dst = torch.zeros(len(raw), dtype=torch.uint8, device="cuda")
    devcodec.decode_to_device([tuple(b) for b in blocks], dst.data_ptr(), len(raw), verify=True)
    assert dst.cpu().numpy().tobytes() == raw

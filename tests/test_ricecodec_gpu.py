"""The MARC10 kernels (csrc/ricez.hip) against the numpy model of
ops/ricecodec.py: the encoder byte for byte at every element size and source
alignment, the decoder over a run of containers, its status word on every
malformation, and the device block codec with ``rank_coding="rice"``. Every
comparison is exact."""

from __future__ import annotations

import numpy as np
import pytest

import rice_corpus as rc

pytestmark = pytest.mark.gpu

CANARY = 0xA5


def _feature():
    import torch  # noqa: F401  (brings the HIP runtime the library links against)

    from modal_amd.ops import load_lib, ricecodec

    return ricecodec, load_lib(required=True)  # binds the ma_ricez_* entries or raises


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
@pytest.mark.parametrize("es", [1, 2, 4])
def test_encoder_matches_the_model_byte_for_byte(es, residue):
    ricecodec, lib = _feature()
    parts = [rc.gauss(rc.DTYPES[es], n) for n in rc.LENGTHS] + [rc.constant()]
    buf, spans = _upload(parts, residue)
    ws = ricecodec.Workspace.for_lengths([ln for _off, ln in spans], ricecodec.HEADER_FIXED)
    got = ricecodec.compress_spans_gpu(lib, buf.data_ptr(), spans, es, ws)
    for data, z in zip(parts, got):
        model = ricecodec.compress_buffer_cpu(data, es)
        assert (z is None) == (model is None), len(data)
        if z is not None:
            assert bytes(z) == model, f"{len(data)} bytes: container differs from the model"


def _decode_run(blobs: list, headers: list, residue: int):
    """Payloads back to back on the device, decoded to ``residue`` mod 16 in a
    canary buffer; returns (status, the buffer, the destination's index in it)."""
    import torch

    ricecodec, lib = _feature()
    comp, spans = _upload([b"".join(z[h.payload_off :] for z, h in zip(blobs, headers))], 5)
    total = sum(h.raw_len for h in headers)
    dst = torch.full((total + 64,), CANARY, dtype=torch.uint8, device="cuda")
    lo = 16 + residue
    status = ricecodec.decompress_run_gpu(
        lib, comp.data_ptr() + spans[0][0], headers, dst.data_ptr() + lo
    )
    return status, dst.cpu().numpy(), lo


@pytest.mark.parametrize("residue", [0, 5])
def test_decoder_writes_a_run_of_containers_in_one_launch(residue):
    ricecodec, _lib = _feature()
    raws = [rc.gauss(rc.DTYPES[es], n) for es in (1, 2, 4) for n in rc.LENGTHS[:3]] + [rc.constant()]
    blobs = [ricecodec.compress_buffer_cpu(raw, es) for raw, es in zip(raws, [1] * 3 + [2] * 3 + [4] * 3 + [1])]
    status, out, lo = _decode_run(blobs, [ricecodec.validate_container(z) for z in blobs], residue)
    raw = b"".join(raws)
    assert status == 0
    assert out[lo : lo + len(raw)].tobytes() == raw
    assert (out[:lo] == CANARY).all() and (out[lo + len(raw) :] == CANARY).all()


@pytest.mark.parametrize("how", sorted(rc.MALFORMED))
def test_decoder_reports_the_first_corrupt_segment_and_leaves_it_alone(how):
    ricecodec, _lib = _feature()
    good, bad, seg, raw, _in_header = rc.malformed(how)
    later = bytearray(good)
    later[rc.hi_offsets(good)[0]] = 9  # a later corrupt segment must not win
    hdr = ricecodec.validate_container(good)  # the patches leave the header as it is
    status, out, lo = _decode_run([good, bad, bytes(later)], [hdr] * 3, 0)
    assert status == 1 + 3 + seg
    first = lo + len(raw) + seg * rc.SEG
    assert (out[first : first + min(rc.SEG, len(raw) - seg * rc.SEG)] == CANARY).all()
    assert out[lo:first].tobytes() == raw + raw[: seg * rc.SEG]


def test_device_codec_with_rank_coding_rice():
    import torch

    _feature()
    from modal_amd.ops import devcodec

    raw = rc.gauss("bfloat16", 2 * rc.MiB + 4096)
    t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    blocks = devcodec.encode_tensor(t, block_size=rc.MiB, elem_size=2, rank_coding="rice")
    host = devcodec.encode_host(raw, block_size=rc.MiB, elem_size=2, rank_coding="rice")
    assert [bytes(b.payload) for b in blocks] == [bytes(b.payload) for b in host]
    assert blocks[0].payload[:6] == b"MARC10" and not blocks[2].compressed
    assert devcodec.encode_tensor(t, block_size=rc.MiB, elem_size=2)[0].payload[:6] == b"MAFP10"
    dst = torch.zeros_like(t)
    devcodec.decode_tensor([tuple(b) for b in blocks], dst, verify=True)
    assert torch.equal(dst, t)


def test_auto_snapshot_of_a_raw_allocation_reaches_marc10_at_es_1(tmp_path):
    import pickle

    from modal_amd.ops import rawmem
    from modal_amd.runtime import gpu_snapshot as gs
    from modal_amd.scheduler.blobs import BlobStore

    ricecodec, _lib = _feature()
    key, want = "raw-fp8-rice", rc.gauss("float8_e4m3fn", rc.MiB)
    buf = rawmem.RawDeviceBuffer(key, len(want))
    try:
        buf.write(want)
        store = BlobStore(str(tmp_path / "blobs"))
        blob = gs.capture_manifest(store, float_codec="auto", rank_coding="rice")
        stored, compressed = store.get_stored(pickle.loads(blob)["raw"][key]["blocks"][0])
        assert compressed and stored[:6] == b"MARC10"
        assert ricecodec.validate_container(stored, rc.MiB).es == 1
        assert bytes(stored) == ricecodec.compress_buffer_cpu(want, 1)
        buf.free()
        gs.restore_payload(blob, store)
        assert rawmem.snapshot_all()[key] == want
    finally:
        rawmem.load_lib(required=True).ma_tracked_free(key.encode())

"""The MAFP10 float-plane codec on the GPU (ops/fpcodec.py + csrc/fpz.hip):
the encoder against the numpy model byte for byte on the corpus of
tests/fp_corpus.py, the decoder into misaligned device memory and its status
word, the device block codec with the option on, and a block-addressed
snapshot of a bf16 tensor end to end. Every comparison is exact."""

from __future__ import annotations

import os
import pickle
import signal

import numpy as np
import pytest

import fp_corpus as fc
import modal_amd as modal
from modal_amd._sync import synchronizer

pytestmark = pytest.mark.gpu

MiB = fc.MiB


def _feature():
    """torch first (it brings the HIP runtime the library links against),
    then the codec and the library with its kernels. Raises where either is
    missing, before the caller has touched the GPU or started a worker."""
    import torch  # noqa: F401

    from modal_amd.ops import devcodec, fpcodec, load_lib

    lib = load_lib(required=True)
    for symbol in ("ma_fpz_rank", "ma_fpz_encode", "ma_fpz_assemble", "ma_fpz_decode"):
        getattr(lib, symbol)
    return devcodec, fpcodec, lib


@pytest.fixture(scope="module")
def model() -> dict:
    """name -> the numpy model's container (or None), computed once."""
    from modal_amd.ops import fpcodec

    return {name: fpcodec.compress_buffer_cpu(data, es) for name, (data, es) in fc.corpus().items()}


def _names(es: int) -> list:
    return [name for name, (_data, e) in sorted(fc.corpus().items()) if e == es]


def _upload(parts: list, es: int):
    """One device buffer with every part at an offset that is es mod 16 (so
    element-aligned and nothing more); returns (tensor, [(offset, length)])."""
    import torch

    spans, end = [], 0
    for data in parts:
        off = -(-end // 16) * 16 + es
        spans.append((off, len(data)))
        end = off + len(data)
    host = np.full(end + 16, 0xA5, dtype=np.uint8)
    for (off, ln), data in zip(spans, parts):
        host[off : off + ln] = np.frombuffer(data, dtype=np.uint8)
    return torch.from_numpy(host).cuda(), spans


@pytest.mark.parametrize("es", [2, 4])
def test_encoder_matches_the_model_byte_for_byte(model, es):
    """The whole corpus of one element size in ONE call: kept and declined
    spans side by side, every source at base + (es mod 16)."""
    _devcodec, fpcodec, lib = _feature()
    names = _names(es)
    buf, spans = _upload([fc.corpus()[n][0] for n in names], es)
    ws = fpcodec.Workspace.for_lengths([ln for _off, ln in spans], fpcodec.HEADER_FIXED)
    got = fpcodec.compress_spans_gpu(lib, buf.data_ptr(), spans, es, ws)
    assert any(model[n] is None for n in names) and any(model[n] is not None for n in names)
    for name, z in zip(names, got):
        want = model[name]
        assert (z is None) == (want is None), name
        if want is not None:
            assert bytes(z) == want, f"{name}: container differs from the model"


def test_hand_assembled_container_from_the_kernels():
    _devcodec, fpcodec, lib = _feature()
    from modal_amd.ops import compress

    buf, spans = _upload([fc.HAND_RAW], 2)
    ws = fpcodec.Workspace.for_lengths([128], fpcodec.HEADER_FIXED)
    got = fpcodec.compress_spans_gpu(lib, buf.data_ptr(), spans, 2, ws)
    assert bytes(got[0]) == fc.HAND_CONTAINER
    assert compress.decompress_buffer_gpu(fc.HAND_CONTAINER) == fc.HAND_RAW
    assert compress.decompress_buffer(fc.HAND_CONTAINER) == fc.HAND_RAW


def _decode_run(fpcodec, lib, blobs: list, es: int):
    """Payloads back to back on the device, decoded to a destination at
    (es mod 16) inside a guarded buffer; returns (status, bytes, guards ok)."""
    import torch

    headers = [fpcodec.validate_container(z) for z in blobs]
    comp, spans = _upload([b"".join(z[h.payload_off :] for z, h in zip(blobs, headers))], es)
    total = sum(h.raw_len for h in headers)
    dst = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    status = fpcodec.decompress_run_gpu(
        lib, comp.data_ptr() + spans[0][0], headers, dst.data_ptr() + 16 + es
    )
    out = dst.cpu().numpy()
    lo, hi = 16 + es, 16 + es + total
    guards = bool((out[:lo] == 0xA5).all() and (out[hi:] == 0xA5).all())
    return status, out[lo:hi].tobytes(), guards


@pytest.mark.parametrize("es", [2, 4])
def test_decoder_round_trips_every_kept_container_in_one_run(model, es):
    _devcodec, fpcodec, lib = _feature()
    names = [n for n in _names(es) if model[n] is not None]
    status, out, guards = _decode_run(fpcodec, lib, [model[n] for n in names], es)
    assert status == 0
    assert guards, "the decoder wrote outside its destination"
    assert out == b"".join(fc.corpus()[n][0] for n in names)


@pytest.mark.parametrize("es", [2, 4])
def test_decoder_run_of_three_and_first_corrupt_segment(model, es):
    _devcodec, fpcodec, lib = _feature()
    names = [f"nseg5_es{es}", f"random_segment_es{es}", "tail4094_es2" if es == 2 else "tail4092_es4"]
    blobs = [model[n] for n in names]
    raw = b"".join(fc.corpus()[n][0] for n in names)
    status, out, guards = _decode_run(fpcodec, lib, blobs, es)
    assert (status, guards) == (0, True) and out == raw

    # segment 3 of the run (in the first container) and the run's last one
    n_last = len(fc.parse(blobs[2])[3])
    bad = [fc.break_segment(blobs[0], 3), blobs[1], fc.break_segment(blobs[2], n_last - 1)]
    status, _out, guards = _decode_run(fpcodec, lib, bad, es)
    assert guards
    assert status == 4
    assert fpcodec.corrupt_message(status) == "MAFP10 container corrupt at segment 3"
    only_last = [blobs[0], blobs[1], bad[2]]
    n_run = sum(len(fc.parse(z)[3]) for z in blobs)
    assert _decode_run(fpcodec, lib, only_last, es)[0] == n_run


def _pattern(n: int, seed: int = 11) -> bytes:
    unit = np.random.default_rng(seed).integers(0, 256, 1024, dtype=np.uint8)
    return np.tile(unit, -(-n // 1024))[:n].tobytes()


def test_device_codec_mixes_lz4_float_and_raw_blocks(model):
    import torch

    devcodec, fpcodec, _lib = _feature()
    from modal_amd.ops import compress

    gauss_a, gauss_b = fc.corpus()["bf16_n01_1m"][0], fc.corpus()["bf16_n002_1m"][0]
    raw = _pattern(MiB) + gauss_a + fc.random_bytes(MiB, seed=77) + gauss_b
    src = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()

    plain = devcodec.encode_device(src.data_ptr(), len(raw), block_size=MiB)
    blocks = devcodec.encode_device(src.data_ptr(), len(raw), block_size=MiB, elem_size=2)
    assert [b.compressed for b in plain] == [True, False, False, False]
    assert [b.compressed for b in blocks] == [True, True, False, True]
    assert [b.digest for b in blocks] == [b.digest for b in plain]
    assert compress.is_compressed(blocks[0].payload) and bytes(blocks[0].payload) == bytes(plain[0].payload)
    assert bytes(blocks[1].payload) == model["bf16_n01_1m"]
    assert bytes(blocks[3].payload) == model["bf16_n002_1m"]
    assert bytes(blocks[2].payload) == raw[2 * MiB : 3 * MiB]

    stored = [tuple(b) for b in blocks]
    dst = torch.zeros(len(raw), dtype=torch.uint8, device="cuda")
    devcodec.decode_to_device(stored, dst.data_ptr(), len(raw), verify=True)
    assert dst.cpu().numpy().tobytes() == raw
    assert devcodec.decode_host(stored) == raw

    # a flipped width byte: the kernel's status; a flipped mantissa byte: the digest
    z = bytes(blocks[1].payload)
    at = fc.segment_offsets(z)[1] + 5  # the low byte of element 5 of segment 1
    for flipped, why in (
        (fc.break_segment(z, 0), "snapshot blocks 1..1: MAFP10 container corrupt at segment 0"),
        (z[:at] + bytes([z[at] ^ 0x10]) + z[at + 1 :], "snapshot block 1 digest mismatch"),
    ):
        broken = list(stored)
        broken[1] = stored[1][:2] + (flipped, True)
        with pytest.raises(ValueError, match=why):
            devcodec.decode_to_device(broken, dst.data_ptr(), len(raw), verify=True)
    with pytest.raises(ValueError, match="snapshot block 3: "):
        broken = list(stored)
        broken[3] = stored[3][:2] + (bytes(blocks[3].payload)[:-1], True)
        devcodec.decode_to_device(broken, dst.data_ptr(), len(raw), verify=True)


def test_float_codec_snapshot_kill_restore_end_to_end(client):
    """A 2 MiB bf16 Gaussian CUDA tensor: snapshot block-addressed with the
    float codec, kill the worker, restore into a fresh process."""
    _feature()
    import torch

    n_elem = MiB  # 2 MiB of bf16
    app = modal.App("snap-float-codec-gpu")

    @app.function(gpu=1)
    def seed_gpu_state(n: int):
        import torch

        from modal_amd.runtime import gpu_snapshot as gs

        g = torch.Generator().manual_seed(1234)
        gs.register_tensor("weights", torch.randn(n, generator=g).to(torch.bfloat16).cuda())
        return True

    expected = torch.randn(n_elem, generator=torch.Generator().manual_seed(1234)).to(torch.bfloat16)
    with app.run(client=client):
        assert seed_gpu_state.remote(n_elem)
        svc = client.svc
        snaps, seeded = [], None
        for wid in list(svc.pool.workers):
            resp = synchronizer.run(
                svc.worker_snapshot(wid, block_addressed=True, float_codec=True)
            )
            m = pickle.loads(svc.blob_store.get(resp["snapshot_id"]))
            if "weights" in m["tensors"]:
                seeded = m
                snaps.append(resp["snapshot_id"])
        assert seeded is not None, "no worker carried the GPU state"
        entry = seeded["tensors"]["weights"]
        assert entry["block_lens"] == [2 * MiB]
        stored, compressed = svc.blob_store.get_stored(entry["blocks"][0])
        assert compressed and stored[:6] == b"MAFP10"
        held = sum(svc.blob_store.size(d) for d in entry["blocks"])
        print(f"tensor {2 * MiB} bytes, CAS holds {held}")
        assert held < 2 * MiB
        for proc in list(svc.pool._procs):
            try:
                os.kill(proc.pid, signal.SIGKILL)
            except OSError:
                pass
        restored_ids = []
        for snap_id in snaps:
            resp = synchronizer.run(svc.worker_restore(snap_id, gpu_index=0))
            assert resp["degraded"] is False
            restored_ids.append(resp["worker_id"])
        found = False
        for wid in restored_ids:
            resp = synchronizer.run(svc.worker_snapshot(wid))
            payload = pickle.loads(svc.blob_store.get(resp["snapshot_id"]))
            got = payload["tensors"].get("weights")
            if got is None:
                continue
            raw_bytes, dtype_s, shape, was_cuda = got
            assert was_cuda and dtype_s == "bfloat16" and shape == (n_elem,)
            assert torch.equal(torch.frombuffer(bytearray(raw_bytes), dtype=torch.bfloat16), expected)
            found = True
        assert found, "no restored worker carried the GPU state"

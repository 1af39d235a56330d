"""The element-size probe on the GPU (fpz_probe_kernel in csrc/fpz.hip and its
callers): both histograms against the numpy twin at every source alignment,
more spans than one grid holds, the encoder fed the probe's tables against
the numpy model byte for byte, ``fpcodec.AUTO`` through the device block
codec, and a block-addressed snapshot of untyped memory end to end. Every
comparison is exact."""

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
LENGTHS = (1, 2, 3, 4, 5, 7, 63, 64, 65, 4095, 4096, 4097, 262147, MiB)
ALL_FF = (4097, 262147)  # lengths whose data is one byte value: every lane on one bin


def _feature():
    """torch first (it brings the HIP runtime the library links against),
    then the codec and the library with the probe's entry points. Raises
    where either is missing, before the caller has touched the GPU."""
    import torch  # noqa: F401

    from modal_amd.ops import devcodec, fpcodec, load_lib

    lib = load_lib(required=True)
    for symbol in ("ma_fpz_probe", "ma_fpz_rank_counts"):
        getattr(lib, symbol)
    return devcodec, fpcodec, lib


def _probe(lib, buf, spans) -> np.ndarray:
    """One ma_fpz_probe call: (len(spans), 2, 256) counts on the host."""
    import torch

    counts = torch.zeros(len(spans), 2, 256, dtype=torch.int32, device="cuda")
    offs = torch.tensor([off for off, _ln in spans], dtype=torch.int64).cuda()
    lens = torch.tensor([ln for _off, ln in spans], dtype=torch.int64).cuda()
    rc = lib.ma_fpz_probe(
        buf.data_ptr(), offs.data_ptr(), lens.data_ptr(), counts.data_ptr(), len(spans),
        torch.cuda.current_stream().cuda_stream,
    )
    assert rc == 0
    return counts.cpu().numpy()


def test_probe_counts_at_every_alignment():
    """Every length at source residues 0..15 mod 16, the spans 16 to 31
    bytes of 0xA5 apart in one buffer: a byte counted from outside a span, or
    one of its own left out, changes a count."""
    import torch

    _devcodec, fpcodec, lib = _feature()
    gauss = fc.bf16_gauss(MiB + 16, seed=91)
    parts, spans, end = [], [], 0
    for n in LENGTHS:
        for r in range(16):
            data = b"\xff" * n if n in ALL_FF else gauss[r : r + n]
            off = -(-end // 16) * 16 + 16 + r
            parts.append(data)
            spans.append((off, n))
            end = off + n
    host = np.full(-(-end // 16) * 16 + 32, 0xA5, dtype=np.uint8)
    for (off, n), data in zip(spans, parts):
        host[off : off + n] = np.frombuffer(data, dtype=np.uint8)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0

    got = _probe(lib, buf, spans)
    for (off, n), data, g in zip(spans, parts, got):
        c2, c4 = fpcodec.probe_counts_cpu(data)
        where = f"length {n} at residue {off % 16}"
        assert np.array_equal(g[0], c2), f"es 2 table differs: {where}"
        assert np.array_equal(g[1], c4), f"es 4 table differs: {where}"
        if n in ALL_FF:
            assert g[0][0xFF] == n // 2 and g[1][0xFF] == n // 4, where


def test_probe_more_spans_than_one_grid():
    """65536 spans of 8 bytes, one past MAX_GRID_Y, starting 3 bytes into
    the buffer so the residues are 3 and 11."""
    import torch

    _devcodec, _fpcodec, lib = _feature()
    n_spans = 65536
    data = np.frombuffer(fc.bf16_gauss(8 * n_spans, seed=92), dtype=np.uint8)
    host = np.full(8 * n_spans + 32, 0xA5, dtype=np.uint8)
    host[3 : 3 + len(data)] = data
    buf = torch.from_numpy(host).cuda()
    got = _probe(lib, buf, [(3 + 8 * k, 8) for k in range(n_spans)])

    want = np.zeros((n_spans, 2, 256), dtype=np.int32)
    rows = data.reshape(n_spans, 8)
    k = np.arange(n_spans)
    for col in (1, 3, 5, 7):
        np.add.at(want, (k, 0, rows[:, col]), 1)
    for col in (3, 7):
        np.add.at(want, (k, 1, rows[:, col]), 1)
    assert np.array_equal(got[-1], want[-1]), "the span past the first grid"
    assert np.array_equal(got, want)


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
def test_encoder_on_the_probes_tables_matches_the_model(es):
    """The corpus of one element size (its 1 MiB inputs among them) in one
    call, the histogram launch replaced by the probe's tables."""
    _devcodec, fpcodec, lib = _feature()
    names = [name for name, (_d, e) in sorted(fc.corpus().items()) if e == es]
    assert es == 4 or {"bf16_n01_1m", "bf16_n002_1m"} <= set(names)
    buf, spans = _upload([fc.corpus()[n][0] for n in names], es)
    _found, tables = fpcodec.probe_spans_gpu(lib, buf.data_ptr(), spans)
    assert tables.shape == (len(spans), 2, 256)
    ws = fpcodec.Workspace.for_lengths([ln for _off, ln in spans], fpcodec.HEADER_FIXED)
    got = fpcodec.compress_spans_gpu(
        lib, buf.data_ptr(), spans, es, ws, counts=tables[:, es // 2 - 1].contiguous()
    )
    kept = 0
    for name, z in zip(names, got):
        want = fpcodec.compress_buffer_cpu(fc.corpus()[name][0], es)
        assert (z is None) == (want is None), name
        if want is not None:
            kept += 1
            assert bytes(z) == want, f"{name}: container differs from the model"
    assert 0 < kept < len(names)


def test_probe_spans_gpu_answers_as_the_host_rule():
    _devcodec, fpcodec, lib = _feature()
    parts = [
        fc.corpus()["bf16_n01_1m"][0], fc.fp32_gauss(MiB, seed=3), fc.random_bytes(MiB, seed=5),
        fc.fp16_gauss(MiB, seed=4),
    ]
    buf, spans = _upload(parts, 2)
    found, _tables = fpcodec.probe_spans_gpu(lib, buf.data_ptr(), spans)
    assert found == [2, 4, 0, 2]
    assert found == [
        fpcodec.choose_elem_size(*fpcodec.probe_counts_cpu(d), len(d))[0] for d in parts
    ]
    assert fpcodec.probe_spans_gpu(lib, buf.data_ptr(), [])[0] == []


def _pattern(n: int, seed: int = 11) -> bytes:
    unit = np.random.default_rng(seed).integers(0, 256, 1024, dtype=np.uint8)
    return np.tile(unit, -(-n // 1024))[:n].tobytes()


def test_device_codec_auto_finds_each_blocks_element_size():
    import torch

    devcodec, fpcodec, _lib = _feature()
    from modal_amd.ops import compress

    bf16, fp32 = fc.corpus()["bf16_n01_1m"][0], fc.fp32_gauss(MiB, seed=3)
    raw = _pattern(MiB) + bf16 + fc.random_bytes(MiB, seed=77) + fp32
    src = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()

    host = devcodec.encode_host(raw, block_size=MiB, elem_size=fpcodec.AUTO)
    blocks = devcodec.encode_device(src.data_ptr(), len(raw), block_size=MiB, elem_size=fpcodec.AUTO)
    assert [b.compressed for b in blocks] == [True, True, False, True]
    assert [b.compressed for b in blocks] == [b.compressed for b in host]
    assert [b.digest for b in blocks] == [b.digest for b in host]
    assert [bytes(b.payload) for b in blocks] == [bytes(b.payload) for b in host]
    assert compress.is_compressed(blocks[0].payload)
    assert bytes(blocks[1].payload) == fpcodec.compress_buffer_cpu(bf16, 2)
    assert bytes(blocks[3].payload) == fpcodec.compress_buffer_cpu(fp32, 4)
    assert [fpcodec.validate_container(blocks[i].payload).es for i in (1, 3)] == [2, 4]

    stored = [tuple(b) for b in blocks]
    dst = torch.zeros(len(raw), dtype=torch.uint8, device="cuda")
    devcodec.decode_to_device(stored, dst.data_ptr(), len(raw), verify=True)
    assert dst.cpu().numpy().tobytes() == raw

    # hinted and unhinted calls give what they gave
    for es in (2, 0):
        want = devcodec.encode_host(raw, block_size=MiB, elem_size=es)
        got = devcodec.encode_device(src.data_ptr(), len(raw), block_size=MiB, elem_size=es)
        assert [b.compressed for b in got][:3] == [True, es == 2, False]
        assert [tuple(b[:2]) + (bytes(b.payload), b.compressed) for b in got] == [
            tuple(b[:2]) + (bytes(b.payload), b.compressed) for b in want
        ]
    with pytest.raises(ValueError):
        devcodec.encode_device(src.data_ptr(), len(raw), block_size=MiB, elem_size=-2)


def test_auto_snapshot_of_untyped_memory_kill_restore_end_to_end(client):
    """A 2 MiB tracked raw allocation of bf16 Gaussian bytes and a 2 MiB uint8
    CUDA tensor of fp32 Gaussian bytes: snapshot block-addressed with
    float_codec="auto", kill the worker, restore into a fresh process."""
    _feature()
    import torch

    app = modal.App("snap-float-auto-gpu")

    @app.function(gpu=1)
    def seed_gpu_state(n_bytes: int):
        import torch

        from modal_amd.ops.rawmem import RawDeviceBuffer
        from modal_amd.runtime import gpu_snapshot as gs

        g = torch.Generator().manual_seed(4321)
        kv = torch.randn(n_bytes // 2, generator=g).to(torch.bfloat16).view(torch.uint8)
        packed = torch.randn(n_bytes // 4, generator=g).view(torch.uint8)
        buf = RawDeviceBuffer("raw-kv", n_bytes)
        buf.write(kv.numpy().tobytes())
        gs._keepalive_raw = buf  # hold the allocation
        gs.register_tensor("packed", packed.cuda())
        return True

    g = torch.Generator().manual_seed(4321)
    want_kv = torch.randn(MiB, generator=g).to(torch.bfloat16).view(torch.uint8).numpy().tobytes()
    want_packed = torch.randn(MiB // 2, generator=g).view(torch.uint8).numpy().tobytes()
    with app.run(client=client):
        assert seed_gpu_state.remote(2 * MiB)
        svc = client.svc
        from modal_amd.ops import fpcodec

        snaps, seeded = [], None
        for wid in list(svc.pool.workers):
            resp = synchronizer.run(
                svc.worker_snapshot(wid, block_addressed=True, float_codec="auto")
            )
            m = pickle.loads(svc.blob_store.get(resp["snapshot_id"]))
            if "packed" in m["tensors"]:
                seeded = m
                snaps.append(resp["snapshot_id"])
        assert seeded is not None, "no worker carried the GPU state"
        for entry, es in ((seeded["raw"]["raw-kv"], 2), (seeded["tensors"]["packed"], 4)):
            assert entry["block_lens"] == [2 * MiB]
            stored, compressed = svc.blob_store.get_stored(entry["blocks"][0])
            assert compressed and stored[:6] == b"MAFP10"
            assert fpcodec.validate_container(stored, 2 * MiB).es == es
            print(f"es {es}: {2 * MiB} bytes, CAS holds {len(stored)}")
        assert seeded["tensors"]["packed"]["dtype"] == "uint8"
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
            got = payload["tensors"].get("packed")
            if got is None:
                continue
            raw_bytes, dtype_s, shape, was_cuda = got
            assert was_cuda and dtype_s == "uint8" and shape == (2 * MiB,)
            assert raw_bytes == want_packed
            assert payload["raw"].get("raw-kv") == want_kv
            found = True
        assert found, "no restored worker carried the GPU state"

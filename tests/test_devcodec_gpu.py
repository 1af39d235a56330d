"""Device block codec (ops/devcodec.py + csrc/malz.hip) on the GPU: the plan
kernel against numpy, encode and both blob compress paths against a container
assembled on the host byte for byte, decode into device memory, digest
verification, and the block-addressed snapshot end to end. Every comparison
is exact."""

from __future__ import annotations

import os
import pickle
import signal
import struct

import numpy as np
import pytest

import modal_amd as modal
from modal_amd._sync import synchronizer

pytestmark = pytest.mark.gpu

MiB = 1024 * 1024
BLOCK = 8 * MiB
SEG = 4096


def _pattern(n: int, seed: int = 11) -> np.ndarray:
    unit = np.random.default_rng(seed).integers(0, 256, 1024, dtype=np.uint8)
    return np.tile(unit, -(-n // 1024))[:n].copy()


def _random(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _feature():
    """The device codec and the library with its kernels. Raises where
    either is missing, before the caller has touched the GPU or started a
    worker, so a build without the feature fails these tests at once."""
    from modal_amd.ops import devcodec, load_lib

    lib = load_lib(required=True)
    for symbol in ("ma_malz_plan", "ma_malz_assemble", "ma_malz_copy"):
        getattr(lib, symbol)
    return devcodec, lib


def _inputs() -> dict:
    mixed = np.empty(3 * MiB, dtype=np.uint8)
    pat, rnd = _pattern(64 * 1024, seed=5), _random(3 * MiB, seed=6)
    for k, off in enumerate(range(0, 3 * MiB, 64 * 1024)):
        mixed[off : off + 64 * 1024] = pat if k % 2 == 0 else rnd[off : off + 64 * 1024]
    return {
        "a_block_and_tail": _pattern(BLOCK + 12345),
        "b_random": _random(2 * MiB, seed=2),
        "c_mixed": mixed,
        "d_one_byte_segment": _pattern(MiB + 1),
        "e_unaligned": _pattern(MiB + 4093 + 3, seed=3),  # encoded as [3:]
        "f_zeros": np.zeros(BLOCK, dtype=np.uint8),
        "g_raw_then_run": np.concatenate(
            [_random(BLOCK, seed=9), _pattern(BLOCK, seed=4), _pattern(MiB + MiB // 2, seed=8)]
        ),
    }


@pytest.fixture(scope="module")
def encoded():
    """name -> (device source tensor, its bytes, encode result); computed
    once and shared, read-only."""
    devcodec, _lib = _feature()
    import torch

    out = {}
    for name, host in _inputs().items():
        dev = torch.from_numpy(host).cuda()
        if name == "e_unaligned":
            dev, host = dev[3:], host[3:]
            assert dev.data_ptr() % 16 == 3
        out[name] = (dev, host.tobytes(), devcodec.encode_tensor(dev))
    return out


def test_plan_kernel_matches_cumsum():
    _devcodec, lib = _feature()
    import torch

    rng = np.random.default_rng(1)
    n_segs = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 4097]
    tails = [1, 4095, 4096]
    raw_lens = np.array(
        [(n - 1) * SEG + tails[k % 3] for k, n in enumerate(n_segs)], dtype=np.int64
    )
    first = (np.cumsum(n_segs) - n_segs).astype(np.int32)
    total = int(sum(n_segs))
    comp_lens = rng.integers(1, SEG, total, dtype=np.int32)
    comp_lens[rng.random(total) < 0.25] = 0
    comp_lens[first[1]] = 0  # a raw FIRST segment and a raw partial LAST one
    comp_lens[first[3] + n_segs[3] - 1] = 0

    want_off = np.empty(total, dtype=np.int64)
    want_payload = np.empty(len(n_segs), dtype=np.int64)
    for b, n in enumerate(n_segs):
        cl = comp_lens[first[b] : first[b] + n].astype(np.int64)
        seg_raw = np.full(n, SEG, dtype=np.int64)
        seg_raw[-1] = raw_lens[b] - (n - 1) * SEG
        eff = np.where(cl == 0, seg_raw, cl)
        want_off[first[b] : first[b] + n] = np.cumsum(eff) - eff
        want_payload[b] = eff.sum()

    comp_d = torch.from_numpy(comp_lens).cuda()
    first_d = torch.from_numpy(first).cuda()
    raw_d = torch.from_numpy(raw_lens).cuda()
    seg_off = torch.full((total,), -1, dtype=torch.int64, device="cuda")
    payload = torch.full((len(n_segs),), -1, dtype=torch.int64, device="cuda")
    rc = lib.ma_malz_plan(
        comp_d.data_ptr(), first_d.data_ptr(), raw_d.data_ptr(), seg_off.data_ptr(),
        payload.data_ptr(), len(n_segs), torch.cuda.current_stream().cuda_stream,
    )
    assert rc == 0
    assert np.array_equal(payload.cpu().numpy(), want_payload)
    assert np.array_equal(seg_off.cpu().numpy().astype(np.int64), want_off)


ENCODE_CASES = {
    "a_block_and_tail": [True, False],
    "b_random": [False],
    "c_mixed": [True],
    "d_one_byte_segment": [True],
    "e_unaligned": [True],
    "f_zeros": [True],
    "g_raw_then_run": [False, True, True],
}


def _host_container(lib, dev, raw: bytes):
    """The oracle: LZ4 kernel on the device bytes ``dev`` into a strided
    tensor, everything else (keep/raw rule, header, table, compaction) with
    numpy and struct on the host, raw segments from the host copy ``raw``."""
    import torch

    stride, min_gain = SEG + 256, 0.95
    n = len(raw)
    n_seg = -(-n // SEG)
    out = torch.empty(n_seg * stride, dtype=torch.uint8, device="cuda")
    lens_d = torch.empty(n_seg, dtype=torch.int32, device="cuda")
    rc = lib.ma_lz4_compress(
        dev.data_ptr(), n, out.data_ptr(), lens_d.data_ptr(), stride, n_seg,
        torch.cuda.current_stream().cuda_stream,
    )
    assert rc == 0
    comp_lens = lens_d.cpu().numpy()
    slots = out.cpu().numpy()
    parts = [b"MALZ41", struct.pack("<QI", n, n_seg), comp_lens.astype("<u4").tobytes()]
    for s, clen in enumerate(comp_lens.tolist()):
        if clen:
            parts.append(slots[s * stride : s * stride + clen].tobytes())
        else:
            parts.append(raw[s * SEG : (s + 1) * SEG])
    if sum(len(p) for p in parts[3:]) >= n * min_gain:
        return None
    return b"".join(parts)


@pytest.mark.parametrize("name", sorted(ENCODE_CASES))
def test_encode_matches_existing_path(encoded, name):
    """The block codec, compress_buffer_gpu and compress_buffers_gpu share one
    device encoder, so all three are held to a container assembled on the
    host from the LZ4 kernel's raw output."""
    from modal_amd.ops.compress import (
        compress_buffer_gpu, compress_buffers_gpu, decompress_buffer_cpu, parse_header,
    )
    from modal_amd.ops.devcodec import COMPRESS_MIN
    from modal_amd.ops.hashing import content_digest

    _devcodec, lib = _feature()
    dev, raw, blocks = encoded[name]
    assert [b.compressed for b in blocks] == ENCODE_CASES[name]
    assert sum(b.raw_len for b in blocks) == len(raw)
    raw_blocks, oracles, off = [], [], 0
    for blk in blocks:
        raw_blocks.append(raw[off : off + blk.raw_len])
        oracles.append(_host_container(lib, dev[off : off + blk.raw_len], raw_blocks[-1]))
        off += blk.raw_len
    batched = compress_buffers_gpu(raw_blocks)
    for blk, block, oracle, from_batch in zip(blocks, raw_blocks, oracles, batched):
        assert blk.digest == content_digest(block)
        assert compress_buffer_gpu(block) == oracle
        assert from_batch == oracle
        if blk.compressed:
            assert blk.payload == oracle
            assert decompress_buffer_cpu(blk.payload) == block
        else:
            assert blk.payload == block
            assert oracle is None or blk.raw_len < COMPRESS_MIN
    if name == "c_mixed":
        _n, comp_lens, _off = parse_header(blocks[0].payload)
        assert any(c == 0 for c in comp_lens) and any(c != 0 for c in comp_lens)
    if name == "d_one_byte_segment":
        _n, comp_lens, _off = parse_header(blocks[0].payload)
        assert len(comp_lens) == 257


def test_batched_compress_staged_subset():
    """compress_buffers_gpu over a shared staging at 8 KiB-aligned offsets,
    compressing a strict subset: picked entries equal the oracle, the others
    are None."""
    from modal_amd.ops.compress import compress_buffers_gpu
    from modal_amd.ops.hashing import LEAF_SIZE
    from modal_amd.ops.staging import stage_many_to_gpu

    _devcodec, lib = _feature()
    buffers = [
        _pattern(MiB + 1, seed=31).tobytes(),
        _pattern(4096, seed=32).tobytes(),
        _pattern(2 * MiB, seed=33).tobytes(),
    ]
    src, offsets = stage_many_to_gpu(buffers, align=LEAF_SIZE)
    assert offsets == [0, MiB + LEAF_SIZE, MiB + 2 * LEAF_SIZE]
    got = compress_buffers_gpu(buffers, staged=(src, offsets), only=[0, 2])
    assert got[1] is None
    for i in (0, 2):
        oracle = _host_container(lib, src[offsets[i] : offsets[i] + len(buffers[i])], buffers[i])
        assert oracle is not None and got[i] == oracle


@pytest.mark.parametrize("name", sorted(ENCODE_CASES))
def test_decode_to_device_round_trip(encoded, name):
    import torch

    from modal_amd.ops import devcodec

    dev, _raw, blocks = encoded[name]
    out = torch.full_like(dev, 0xA5)
    devcodec.decode_tensor(blocks, out, verify=True)
    assert torch.equal(out, dev)


def test_decode_verification_names_the_block(encoded):
    import torch

    from modal_amd.ops import devcodec

    dev, _raw, blocks = encoded["g_raw_then_run"]
    first = blocks[0]
    assert not first.compressed  # only raw-stored bytes are damaged
    damaged = bytearray(first.payload)
    damaged[len(damaged) // 2] ^= 0x01
    bad = [first._replace(payload=bytes(damaged))] + list(blocks[1:])
    out = torch.empty_like(dev)
    with pytest.raises(ValueError, match="block 0 digest mismatch"):
        devcodec.decode_tensor(bad, out, verify=True)


def test_verify_device_batches_objects(encoded):
    from modal_amd.ops import devcodec

    names = ["a_block_and_tail", "g_raw_then_run", "e_unaligned"]
    objects = [
        (encoded[n][0].data_ptr(), [(b.digest, b.raw_len) for b in encoded[n][2]]) for n in names
    ]
    devcodec.verify_device(objects)
    wrong = encoded["b_random"][2][0].digest
    # a full (tree-hashed) block, a short tail, a run's tail, a lone block
    for oi, bi in [(0, 0), (0, 1), (1, 2), (2, 0)]:
        bad = [(ptr, list(blocks)) for ptr, blocks in objects]
        bad[oi][1][bi] = (wrong, bad[oi][1][bi][1])
        with pytest.raises(ValueError, match=f"block {bi} digest mismatch in object {oi}"):
            devcodec.verify_device(bad)


def test_known_blocks_are_skipped_and_no_scratch_stores_raw(encoded, monkeypatch):
    from modal_amd.ops import devcodec

    dev, raw, blocks = encoded["a_block_and_tail"]
    span = [(dev.data_ptr(), len(raw))]
    have = {blocks[0].digest}
    got = [b for _oi, b in devcodec.iter_encode_device(span, known=have.__contains__)]
    assert got[0] == blocks[0]._replace(payload=None, compressed=False)
    assert got[1] == blocks[1]
    # HBM too full for the scratch: same digests, raw payloads
    monkeypatch.setattr(devcodec, "_get_scratch", lambda: None)
    got = devcodec.encode_device(*span[0])
    assert [b.digest for b in got] == [b.digest for b in blocks]
    assert b"".join(b.payload for b in got) == raw
    assert not any(b.compressed for b in got)


def test_block_addressed_snapshot_kill_restore_end_to_end(client):
    """bf16 CUDA tensor of two blocks + a tracked raw allocation: snapshot
    block-addressed, kill the worker, restore into a fresh process."""
    import inspect

    from modal_amd.scheduler.core import Scheduler

    _feature()
    assert "block_addressed" in inspect.signature(Scheduler.worker_snapshot).parameters
    import torch

    n_elem = 4 * 1024 * 1024 + 3
    raw_pattern = _pattern(2 * MiB, seed=21).tobytes()
    app = modal.App("snap-blocks-gpu")

    @app.function(gpu=1)
    def seed_gpu_state(n: int, pattern: bytes):
        import torch

        from modal_amd.ops.rawmem import RawDeviceBuffer
        from modal_amd.runtime import gpu_snapshot as gs

        t = (torch.arange(n, device="cuda") % 251).to(torch.bfloat16)
        gs.register_tensor("gpu-weights", t)
        buf = RawDeviceBuffer("raw-scratch", len(pattern))
        buf.write(pattern)
        gs._keepalive_raw = buf  # hold the allocation
        return True

    expected = (torch.arange(n_elem) % 251).to(torch.bfloat16)
    with app.run(client=client):
        assert seed_gpu_state.remote(n_elem, raw_pattern)
        svc = client.svc
        snaps = []  # only the snapshot that carries the state is restored
        seeded = None
        for wid in list(svc.pool.workers):
            resp = synchronizer.run(svc.worker_snapshot(wid, block_addressed=True))
            m = pickle.loads(svc.blob_store.get(resp["snapshot_id"]))
            if "gpu-weights" in m["tensors"]:
                seeded = m
                snaps.append(resp["snapshot_id"])
        assert seeded is not None, "no worker carried the GPU state"
        assert seeded["tensors"]["gpu-weights"]["block_lens"] == [BLOCK, 6]
        assert seeded["raw"]["raw-scratch"]["block_lens"] == [2 * MiB]
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
        # re-read the restored workers' state out of fresh device memory in
        # the NEW processes (the byte-level v1 payload)
        found = False
        for wid in restored_ids:
            resp = synchronizer.run(svc.worker_snapshot(wid))
            payload = pickle.loads(svc.blob_store.get(resp["snapshot_id"]))
            entry = payload["tensors"].get("gpu-weights")
            if entry is None:
                continue
            raw_bytes, dtype_s, shape, was_cuda = entry
            assert was_cuda and dtype_s == "bfloat16" and shape == (n_elem,)
            got = torch.frombuffer(bytearray(raw_bytes), dtype=torch.bfloat16)
            assert torch.equal(got, expected)
            assert got.float().sum().item() == expected.float().sum().item()
            assert payload["raw"].get("raw-scratch") == raw_pattern
            found = True
        assert found, "no restored worker carried the GPU state"

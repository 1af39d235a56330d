"""Block-addressed (version 2) snapshots without a GPU: manifests through
the host codec, CAS dedup, incremental capture, container header validation
and the cross-process flow with CPU workers."""

from __future__ import annotations

import os
import pickle
import signal
import struct

import numpy as np
import pytest

import modal_amd as modal
from modal_amd._sync import synchronizer

BLOCK = 8 * 1024 * 1024


def _pattern(n: int, seed: int = 7) -> np.ndarray:
    unit = np.random.default_rng(seed).integers(0, 256, 1024, dtype=np.uint8)
    return np.tile(unit, -(-n // 1024))[:n].copy()


def _count_files(root) -> int:
    return sum(len(files) for _d, _s, files in os.walk(root))


@pytest.fixture()
def gs():
    from modal_amd.runtime import gpu_snapshot

    gpu_snapshot._registered_tensors.clear()
    gpu_snapshot._restored_tensors.clear()
    yield gpu_snapshot
    gpu_snapshot._registered_tensors.clear()
    gpu_snapshot._restored_tensors.clear()


def test_manifest_round_trip_host_codec(tmp_path, gs):
    import torch

    from modal_amd.ops.hashing import content_digest
    from modal_amd.scheduler.blobs import BlobStore

    big = torch.from_numpy(_pattern(BLOCK + 5))
    state = {
        "bf16": (torch.arange(15, dtype=torch.float32) * 0.5).to(torch.bfloat16).reshape(3, 5),
        "empty": torch.empty(0, dtype=torch.float32),
        "scalar": torch.tensor(-123456789012, dtype=torch.int64),
        "big": big,
    }
    for key, t in state.items():
        gs.register_tensor(key, t)
    store = BlobStore(str(tmp_path / "blobs"))
    manifest = gs.capture_manifest(store)

    m = pickle.loads(manifest)
    assert m["version"] == 2
    assert m["tensors"]["empty"]["blocks"] == []
    assert m["tensors"]["big"]["block_lens"] == [BLOCK, 5]
    for key, t in state.items():
        entry = m["tensors"][key]
        raw = t.reshape(-1).view(torch.uint8).numpy().tobytes()
        assert entry["nbytes"] == len(raw)
        off = 0
        for digest, ln in zip(entry["blocks"], entry["block_lens"]):
            assert digest == content_digest(raw[off : off + ln])
            assert store.has(digest)
            off += ln
        assert off == len(raw)

    gs._registered_tensors.clear()
    gs._restored_tensors.clear()
    gs.restore_payload(manifest, store)
    for key, t in state.items():
        out = gs.restored_tensor(key)
        assert out.dtype == t.dtype and out.shape == t.shape
        assert torch.equal(out, t)


def test_second_capture_adds_no_file(tmp_path, gs):
    import torch

    from modal_amd.scheduler.blobs import BlobStore

    gs.register_tensor("w", torch.from_numpy(_pattern(BLOCK + 4096)))
    gs.register_tensor("b", torch.arange(100, dtype=torch.float32))
    store = BlobStore(str(tmp_path / "blobs"))
    first = pickle.loads(gs.capture_manifest(store))
    n_files = _count_files(store.root)
    assert n_files == 3
    second = pickle.loads(gs.capture_manifest(store))
    assert _count_files(store.root) == n_files
    assert second["tensors"] == first["tensors"]


def test_incremental_capture_stores_one_block(tmp_path, gs):
    import torch

    from modal_amd.scheduler.blobs import BlobStore

    # three DIFFERENT blocks, so the count below is not hidden by dedup
    data = np.concatenate([_pattern(BLOCK, seed=s) for s in (1, 2, 3)])
    t = torch.from_numpy(data)
    gs.register_tensor("w", t)
    store = BlobStore(str(tmp_path / "blobs"))
    before = pickle.loads(gs.capture_manifest(store))["tensors"]["w"]["blocks"]
    assert len(before) == 3 and len(set(before)) == 3
    n_files = _count_files(store.root)
    t[BLOCK + BLOCK // 2] ^= 0xFF
    after = pickle.loads(gs.capture_manifest(store))["tensors"]["w"]["blocks"]
    assert _count_files(store.root) == n_files + 1
    assert [a != b for a, b in zip(before, after)] == [False, True, False]


def test_container_header_validation():
    from modal_amd.ops import devcodec
    from modal_amd.ops.compress import MAGIC

    data = _pattern(1024 * 1024 + 100).tobytes()
    (blk,) = devcodec.encode_host(data)
    assert blk.compressed and blk.raw_len == len(data)
    good = blk.payload
    assert devcodec.decode_host([blk]) == data
    devcodec.validate_container(good, blk.raw_len, 0)

    table = len(MAGIC) + 12
    (first_len,) = struct.unpack_from("<I", good, table)
    (raw_len,) = struct.unpack_from("<Q", good, len(MAGIC))
    mutations = {
        "truncated": good[:-1],
        "comp_len": good[:table] + struct.pack("<I", first_len + 1) + good[table + 4 :],
        "raw_len": good[: len(MAGIC)] + struct.pack("<Q", raw_len + 1) + good[len(MAGIC) + 8 :],
    }
    for name, bad in mutations.items():
        assert len(bad) in (len(good), len(good) - 1), name
        with pytest.raises(ValueError, match="block 3"):
            devcodec.validate_container(bad, blk.raw_len, 3)
        with pytest.raises(ValueError):
            devcodec.decode_host([(blk.digest, blk.raw_len, bad, True)])


def test_manifest_needs_store_and_v1_still_restores(tmp_path, gs):
    import torch

    from modal_amd.scheduler.blobs import BlobStore

    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    gs.register_tensor("w", t)
    v1 = gs.capture_payload()
    v2 = gs.capture_manifest(BlobStore(str(tmp_path / "blobs")))
    gs._registered_tensors.clear()
    gs._restored_tensors.clear()
    with pytest.raises(ValueError):
        gs.restore_payload(v2)
    assert gs.restored_tensor("w") is None
    gs.restore_payload(v1)
    assert torch.equal(gs.restored_tensor("w"), t)


def test_worker_snapshot_block_addressed_cross_process_cpu(client):
    """snapshot(block_addressed) -> kill -> restore into FRESH workers: the
    manifest is small, and the restored state re-encodes to the same blocks."""
    import inspect

    from modal_amd.runtime.gpu_snapshot import capture_manifest  # noqa: F401
    from modal_amd.scheduler.core import Scheduler

    # a build without the feature fails here, before any worker starts
    assert "block_addressed" in inspect.signature(Scheduler.worker_snapshot).parameters
    app = modal.App("snap-blocks")
    n_elem = 4 * 1024 * 1024 + 1

    @app.function()
    def seed_state(n: int):
        import torch

        from modal_amd.runtime import gpu_snapshot as gs

        gs.register_tensor("model-state", torch.arange(n, dtype=torch.float32))
        return True

    with app.run(client=client):
        assert seed_state.remote(n_elem)
        svc = client.svc
        snaps = {}
        for wid in list(svc.pool.workers):
            resp = synchronizer.run(svc.worker_snapshot(wid, block_addressed=True))
            snaps[wid] = resp["snapshot_id"]
        seeded = None
        for wid, snap_id in list(snaps.items()):
            assert svc.blob_store.size(snap_id) < 64 * 1024
            m = pickle.loads(svc.blob_store.get(snap_id))
            assert m["version"] == 2
            if "model-state" in m["tensors"]:
                seeded = m["tensors"]["model-state"]
            else:
                del snaps[wid]  # only the snapshot that carries the state is restored
        assert seeded is not None, "no worker carried the registered tensor"
        assert seeded["block_lens"] == [BLOCK, BLOCK, 4]
        assert all(svc.blob_store.has(d) for d in seeded["blocks"])

        for proc in list(svc.pool._procs):
            try:
                os.kill(proc.pid, signal.SIGKILL)
            except OSError:
                pass
        restored_ids = []
        for snap_id in snaps.values():
            resp = synchronizer.run(svc.worker_restore(snap_id))
            assert resp["degraded"] is False
            restored_ids.append(resp["worker_id"])
        found = False
        for wid in restored_ids:
            resp = synchronizer.run(svc.worker_snapshot(wid, block_addressed=True))
            m = pickle.loads(svc.blob_store.get(resp["snapshot_id"]))
            entry = m["tensors"].get("model-state")
            if entry is not None:
                assert entry["blocks"] == seeded["blocks"]
                assert entry["dtype"] == "float32" and entry["shape"] == (n_elem,)
                found = True
        assert found, "no restored worker carried the registered tensor"

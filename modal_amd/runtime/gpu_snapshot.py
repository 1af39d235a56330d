"""GPU memory snapshot/restore for ROCm (the cuda-checkpoint replacement).

The reference drives NVIDIA's external ``cuda-checkpoint`` binary to page a
PID's GPU memory to host RAM and back (/root/reference/py/modal/_runtime/
gpu_memory_snapshot.py:158-300, four-state machine :35-43, sentinel exit 222
:20-23), and restores a process via ``/__modal/restore-state.json``
(task_lifecycle_manager.py:146-215). ROCm has no cuda-checkpoint, so the
MI355X-native design snapshots at the framework level, in three layers:

1. torch tensors — every live CUDA tensor is paged D2H into pinned host
   buffers and re-paged on restore (in-process page-out for scaledown).
2. raw hipMalloc allocations — anything allocated through the tracked
   allocator (ops/rawmem.py, csrc/rawmem.hip) is paged by stable key and
   survives into a FRESH process.
3. RNG state — torch CPU+CUDA generators, python ``random``, numpy.

Cross-process restore follows the reference's restore-state contract: the
new worker busy-waits for a restore-state JSON (path in
$MODAL_AMD_RESTORE_STATE_PATH, defaulting to the reference's
``/__modal/restore-state.json``), applies env overrides, loads the snapshot
payload, and exits with the sentinel code 222 on failure so the supervisor
retries without snapshot.

Two payload versions restore through ``restore_payload``: version 1
(``capture_payload``) carries every byte inline in one pickle; version 2
(``capture_manifest``, opt-in) stores the state as content-addressed blocks
in a ``BlobStore``, encoded on the GPU for device memory (ops/devcodec.py),
and carries only their digests.
"""

from __future__ import annotations

import enum
import gc
import os
import pickle
import sys
import time
import warnings
from typing import Any, Optional

# parity: the runtime retries without snapshot when it sees this exit code
CUDA_CHECKPOINT_SENTINEL_EXIT = 222

RESTORE_STATE_PATH_DEFAULT = "/__modal/restore-state.json"


class CudaCheckpointState(enum.Enum):
    """Parity: reference gpu_memory_snapshot.py:35-43."""

    RUNNING = "running"
    CHECKPOINTED = "checkpointed"
    FAILED = "failed"
    LOCKED = "locked"


# ---------------------------------------------------------------------------
# snapshot-visible registries (cross-process survivors)
# ---------------------------------------------------------------------------

#: tensors user/framework code explicitly registered to survive a
#: cross-process restore: key -> tensor
_registered_tensors: dict[str, Any] = {}
#: state restored from a snapshot payload in THIS process
_restored_tensors: dict[str, Any] = {}


def register_tensor(key: str, tensor: Any) -> None:
    """Mark a tensor as snapshot-visible: it will be serialized into
    cross-process snapshots under this key."""
    _registered_tensors[key] = tensor


def restored_tensor(key: str) -> Any:
    """Fetch a tensor restored from a snapshot (falls back to the live
    registry so code is identical on first run and after restore)."""
    if key in _restored_tensors:
        return _restored_tensors[key]
    return _registered_tensors.get(key)


def _rng_capture() -> dict:
    state: dict[str, Any] = {}
    try:
        import random

        state["py"] = random.getstate()
    except Exception:
        pass
    try:
        import numpy as np

        state["np"] = np.random.get_state()
    except Exception:
        pass
    try:
        import torch

        state["torch_cpu"] = torch.get_rng_state()
        if torch.cuda.is_available():
            state["torch_cuda"] = torch.cuda.get_rng_state_all()
    except Exception:
        pass
    return state


def _rng_restore(state: dict) -> None:
    try:
        if "py" in state:
            import random

            random.setstate(state["py"])
    except Exception:
        pass
    try:
        if "np" in state:
            import numpy as np

            np.random.set_state(state["np"])
    except Exception:
        pass
    try:
        import torch

        if "torch_cpu" in state:
            torch.set_rng_state(state["torch_cpu"])
        if "torch_cuda" in state and torch.cuda.is_available():
            saved = state["torch_cuda"]
            n = min(len(saved), torch.cuda.device_count())
            for i in range(n):
                torch.cuda.set_rng_state(saved[i], i)
    except Exception:
        pass


# ---------------------------------------------------------------------------
# in-process page-out (scaledown) — tensors stay object-identical
# ---------------------------------------------------------------------------


class GPUMemorySnapshot:
    """Page all torch CUDA state + tracked raw allocations of this process
    to host memory, reversibly (the scaledown page-out)."""

    def __init__(self) -> None:
        self.state = CudaCheckpointState.RUNNING
        self._saved: list[tuple[Any, Any, Any]] = []  # (tensor, host_copy, device)
        self._raw: dict[str, bytes] = {}
        self._rng: dict = {}

    def checkpoint(self) -> None:
        if self.state is not CudaCheckpointState.RUNNING:
            raise RuntimeError(f"checkpoint() in state {self.state}")
        self.state = CudaCheckpointState.LOCKED
        try:
            import torch

            if not torch.cuda.is_available():
                self.state = CudaCheckpointState.CHECKPOINTED
                return
            self._rng = _rng_capture()
            stream = torch.cuda.Stream()
            seen_storages: set[int] = set()
            with torch.cuda.stream(stream), warnings.catch_warnings():
                # scanning gc objects trips deprecation warnings in
                # libraries' lazy attributes — silence the scan only
                warnings.simplefilter("ignore")
                for obj in gc.get_objects():
                    try:
                        if not isinstance(obj, torch.Tensor) or not obj.is_cuda:
                            continue
                    except Exception:
                        continue
                    storage_key = obj.untyped_storage().data_ptr()
                    if storage_key in seen_storages:
                        continue
                    seen_storages.add(storage_key)
                    host = torch.empty_like(obj, device="cpu", pin_memory=True)
                    host.copy_(obj, non_blocking=True)
                    self._saved.append((obj, host, obj.device))
            stream.synchronize()
            # release device memory: re-point tensors at empty storage
            for tensor, _host, _device in self._saved:
                tensor.data = torch.empty(0, dtype=tensor.dtype, device="cpu")
            # tracked raw hipMalloc allocations page out by key
            from ..ops import rawmem

            self._raw = rawmem.snapshot_all()
            rawmem.release_all()
            torch.cuda.empty_cache()
            self.state = CudaCheckpointState.CHECKPOINTED
        except BaseException:
            self.state = CudaCheckpointState.FAILED
            raise

    def restore(self) -> None:
        if self.state is not CudaCheckpointState.CHECKPOINTED:
            raise RuntimeError(f"restore() in state {self.state}")
        self.state = CudaCheckpointState.LOCKED
        try:
            import torch

            stream = torch.cuda.Stream() if torch.cuda.is_available() else None
            for tensor, host, device in self._saved:
                if stream is not None:
                    with torch.cuda.stream(stream):
                        tensor.data = host.to(device, non_blocking=True)
                else:
                    tensor.data = host
            if stream is not None:
                stream.synchronize()
            if self._raw:
                from ..ops import rawmem

                rawmem.restore_all(self._raw)
                self._raw = {}
            if self._rng:
                _rng_restore(self._rng)
                self._rng = {}
            self._saved.clear()
            self.state = CudaCheckpointState.RUNNING
        except BaseException:
            self.state = CudaCheckpointState.FAILED
            raise

    def fail_with_sentinel(self) -> None:
        """Exit so the supervisor retries without snapshotting
        (parity: exit-222 contract, reference :20-23,191)."""
        sys.exit(CUDA_CHECKPOINT_SENTINEL_EXIT)


# ---------------------------------------------------------------------------
# cross-process snapshot payloads (worker death / warm restore)
# ---------------------------------------------------------------------------


def capture_payload() -> bytes:
    """Serialize the snapshot-visible state of this process: registered
    tensors (paged D2H), tracked raw allocations, RNG. The result restores
    into a FRESH process (pointers re-allocated, keys preserved)."""
    from ..ops import rawmem

    tensors: dict[str, tuple] = {}
    if _registered_tensors:
        import torch

        for key, t in _registered_tensors.items():
            host = t.detach().cpu().contiguous()
            # byte-level extraction: numpy() would reject bf16/fp8 dtypes
            raw = host.reshape(-1).view(torch.uint8).numpy().tobytes() if host.numel() else b""
            tensors[key] = (
                raw,
                str(t.dtype).removeprefix("torch."),
                tuple(t.shape),
                t.is_cuda,
            )
    payload = {
        "version": 1,
        "tensors": tensors,
        "raw": rawmem.snapshot_all(),
        "rng": _rng_capture(),
        "fidelity": rawmem.fidelity_report(),
    }
    return pickle.dumps(payload, 4)


def restore_payload(data: bytes, store: Any = None) -> dict:
    """Rehydrate a capture_payload() or capture_manifest() blob into THIS
    process. A version-2 manifest names CAS blocks, so it needs the
    ``BlobStore`` that holds them. Returns the fidelity report recorded at
    capture time."""
    payload = pickle.loads(data)
    if payload.get("version") == 2:
        if store is None:
            raise ValueError("a version-2 snapshot manifest needs the blob store of its blocks")
        _restore_manifest(payload, store)
        _rng_restore(payload.get("rng", {}))
        return payload.get("fidelity", {})
    from ..ops import rawmem

    if payload.get("raw"):
        rawmem.restore_all(payload["raw"])
    try:
        import torch

        for key, (raw, dtype_s, shape, was_cuda) in payload.get("tensors", {}).items():
            dtype = getattr(torch, dtype_s)
            if raw:
                t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(dtype)
                t = t.reshape(shape) if shape else t.reshape(())
            else:
                t = torch.empty(shape or (0,), dtype=dtype)
            if was_cuda and torch.cuda.is_available():
                t = t.cuda()
            _restored_tensors[key] = t
            _registered_tensors[key] = t
    except Exception:
        if payload.get("tensors"):
            raise
    _rng_restore(payload.get("rng", {}))
    return payload.get("fidelity", {})


# ---------------------------------------------------------------------------
# version 2: block-addressed manifests (payload lives in the CAS)
# ---------------------------------------------------------------------------

#: blocks fetched and decoded per call on restore (bounds host memory)
_RESTORE_CHUNK_BLOCKS = 8


def capture_manifest(store: Any, float_codec: Any = False) -> bytes:
    """Block-addressed snapshot: every registered tensor and tracked raw
    allocation is cut into CAS blocks, hashed and compressed where it lives
    (CUDA memory on the GPU through ops/devcodec.py, CPU tensors on the
    host), each new block goes to ``store`` and only the digests are
    returned. Blocks the store already has are neither compressed nor
    copied, so a second snapshot of unchanged state costs its hashing.

    ``float_codec`` True offers the blocks of registered bf16/fp16/fp32
    tensors that LZ4 declined to the float-plane codec (ops/fpcodec.py);
    raw allocations carry no element type and are not offered. ``"auto"``
    also offers everything else, the other registered tensors (CUDA or CPU)
    and every tracked raw allocation, at the element size a probe of each
    block's bytes finds, or raw where it finds none. Digests are of the raw
    blocks, so the manifest is the same whatever the option, and restore
    needs no flag: a stored container names its codec."""
    from ..ops import devcodec, fpcodec, rawmem

    if float_codec not in (False, True, "auto"):
        raise ValueError(f'float_codec is False, True or "auto", got {float_codec!r}')
    untyped = fpcodec.AUTO if float_codec == "auto" else 0

    def hint(t: Any) -> int:
        fits = float_codec and t.dtype.is_floating_point and t.element_size() in (2, 4)
        return t.element_size() if fits else untyped

    def entry_for(nbytes: int, **extra: Any) -> dict:
        return {"blocks": [], "block_lens": [], "nbytes": nbytes, **extra}

    def add(entry: dict, blk: Any) -> None:
        if blk.payload is not None:
            store.put_prepared(blk.digest, blk.payload, blk.compressed)
        entry["blocks"].append(blk.digest)
        entry["block_lens"].append(blk.raw_len)

    tensors: dict[str, dict] = {}
    raw: dict[str, dict] = {}
    # (entry, ptr, nbytes, element size hint, keepalive)
    on_device: list[tuple[dict, int, int, int, Any]] = []
    if _registered_tensors:
        import torch

        for key, t in _registered_tensors.items():
            nbytes = t.numel() * t.element_size()
            entry = tensors[key] = entry_for(
                nbytes,
                dtype=str(t.dtype).removeprefix("torch."),
                shape=tuple(t.shape),
                was_cuda=t.is_cuda,
            )
            if nbytes == 0:
                continue
            src = t.detach().contiguous()
            if src.is_cuda:
                on_device.append((entry, src.data_ptr(), nbytes, hint(t), src))
            else:
                # byte-level view: numpy() would reject bf16/fp8 dtypes
                flat = src.reshape(-1).view(torch.uint8).numpy()
                for blk in devcodec.encode_host(flat, elem_size=hint(t)):
                    add(entry, blk)
    lib = rawmem.load_lib()
    if lib is not None:
        for key in rawmem._iter_keys(lib):
            found = rawmem.lookup(key)
            if found is None or (found[1] and not found[0]):
                continue  # released (paged out) rows have no device memory
            entry = raw[key] = entry_for(found[1])
            if found[1]:
                on_device.append((entry, found[0], found[1], untyped, None))
    if on_device:
        objects = [(ptr, nbytes) for _e, ptr, nbytes, _es, _k in on_device]
        hints = [es for _e, _ptr, _n, es, _k in on_device]
        for oi, blk in devcodec.iter_encode_device(objects, known=store.has, elem_sizes=hints):
            add(on_device[oi][0], blk)
    payload = {
        "version": 2,
        "tensors": tensors,
        "raw": raw,
        "rng": _rng_capture(),
        "fidelity": rawmem.fidelity_report(),
    }
    return pickle.dumps(payload, 4)


def _stored_chunks(entry: dict, store: Any):
    """(byte offset, [(digest, raw_len, payload, compressed)]) a few blocks
    at a time, in order."""
    off = 0
    digests, lens = entry["blocks"], entry["block_lens"]
    for i in range(0, len(digests), _RESTORE_CHUNK_BLOCKS):
        chunk = []
        for digest, raw_len in zip(
            digests[i : i + _RESTORE_CHUNK_BLOCKS], lens[i : i + _RESTORE_CHUNK_BLOCKS]
        ):
            stored, compressed = store.get_stored(digest)
            chunk.append((digest, raw_len, stored, compressed))
        yield off, chunk
        off += sum(b[1] for b in chunk)


def _decode_into(entry: dict, store: Any, ptr: int, decoded: list) -> None:
    """Decode an object's blocks into device memory at ptr, unverified;
    ``decoded`` collects what _restore_manifest verifies in one pass."""
    from ..ops import devcodec

    if sum(entry["block_lens"]) != entry["nbytes"]:
        raise ValueError("snapshot manifest block lengths do not add up")
    for off, chunk in _stored_chunks(entry, store):
        devcodec.decode_to_device(chunk, ptr + off, sum(b[1] for b in chunk), verify=False)
    decoded.append((ptr, list(zip(entry["blocks"], entry["block_lens"]))))


def _restore_manifest(payload: dict, store: Any) -> None:
    from ..ops import devcodec, rawmem

    decoded: list = []  # device objects: (ptr, [(digest, raw_len)])
    restored: dict[str, Any] = {}
    for key, entry in payload.get("raw", {}).items():
        ptr = rawmem.acquire(key, entry["nbytes"])
        _decode_into(entry, store, ptr, decoded)
    if payload.get("tensors"):
        import torch

        for key, entry in payload["tensors"].items():
            dtype = getattr(torch, entry["dtype"])
            nbytes = entry["nbytes"]
            if entry["was_cuda"] and torch.cuda.is_available():
                flat = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
                _decode_into(entry, store, flat.data_ptr(), decoded)
            else:
                data = bytearray()
                for _off, chunk in _stored_chunks(entry, store):
                    data += devcodec.decode_host(chunk)
                if len(data) != nbytes:
                    raise ValueError(f"snapshot tensor {key!r}: {len(data)} bytes, manifest {nbytes}")
                flat = (
                    torch.frombuffer(data, dtype=torch.uint8)
                    if nbytes
                    else torch.empty(0, dtype=torch.uint8)
                )
            restored[key] = flat.view(dtype).reshape(entry["shape"])
    if decoded:
        # every device object re-hashed against the manifest, the short
        # blocks of all of them in one dispatch
        devcodec.verify_device(decoded)
    _restored_tensors.update(restored)
    _registered_tensors.update(restored)


def wait_and_restore_from_state_file(path: Optional[str] = None, timeout: float = 60.0) -> Optional[dict]:
    """The restored-process half of the reference's restore contract
    (task_lifecycle_manager.py:146-193): busy-wait for the restore-state
    JSON, apply env overrides, load the snapshot payload. Returns the state
    dict, or None when no restore is configured. Exits 222 on failure."""
    path = path or os.environ.get("MODAL_AMD_RESTORE_STATE_PATH")
    if not path:
        if os.path.exists(RESTORE_STATE_PATH_DEFAULT):
            path = RESTORE_STATE_PATH_DEFAULT
        else:
            return None
    import json

    deadline = time.time() + timeout
    while not os.path.exists(path):
        if time.time() > deadline:
            sys.exit(CUDA_CHECKPOINT_SENTINEL_EXIT)
        time.sleep(0.05)
    try:
        with open(path) as f:
            state = json.load(f)
        for key, value in (state.get("env") or {}).items():
            os.environ[key] = str(value)
        blob_path = state.get("snapshot_path")
        if blob_path:
            store = None
            if state.get("blob_root"):
                from ..scheduler.blobs import BlobStore

                store = BlobStore(state["blob_root"])
            with open(blob_path, "rb") as f:
                restore_payload(f.read(), store)
        return state
    except BaseException:
        sys.exit(CUDA_CHECKPOINT_SENTINEL_EXIT)

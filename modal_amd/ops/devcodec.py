"""Block codec for device-resident state: hash, compress and frame on the GPU.

A GPU snapshot's payload already lives in HBM, and the SHA-256 and LZ4
kernels take device pointers, so an object (a tensor's storage, a tracked
raw allocation) is encoded where it is: split into CAS blocks of
``BLOCK_SIZE``, every block hashed in place, compressed into the strided
scratch, and finished into a MALZ41 container by the plan/assemble kernels
(csrc/malz.hip). Only the dense containers, or the raw bytes of blocks that
do not compress, cross to the host. Decoding validates every container
header on the host, stages the compressed bytes H2D and decompresses
straight into the destination allocation.

The low level works on ``(device pointer, nbytes)`` so torch tensors and
``rawmem`` allocations share it. ``encode_host``/``decode_host`` are the
GPU-less twins: same digests (``hashing.content_digest`` of the block), same
manifests, containers not necessarily byte-identical.

A kept block's container is byte-identical to ``compress_buffer_gpu(block)``:
same compress kernel, same keep/raw rule, same header. That is what lets the
CAS dedup between this path and ``BlobStore.put``.
"""

from __future__ import annotations

import hashlib
import struct
import threading
import time
from typing import Any, Callable, Iterator, NamedTuple, Optional, Sequence

import numpy as np

from ..scheduler.blobs import BLOCK_SIZE, BlobStore
from . import load_lib
from .compress import MAGIC, MIN_GAIN, OUT_STRIDE, SEG_SIZE
from .hashing import GPU_MIN_BYTES, LEAF_SIZE, _root_digest, content_digest, tree_sha256_cpu

WINDOW = 64 * 1024 * 1024  # source bytes encoded per plan/assemble round
HEADER_FIXED = len(MAGIC) + 12  # magic + u64 raw_len + u32 n_seg
COMPRESS_MIN = BlobStore.COMPRESS_MIN
RUN_MAX_BLOCKS = 128  # decode: blocks per decompress launch, at most
_TREE_GROUP = 8  # verify: full blocks whose leaves share one hash dispatch

_H2D, _D2H = 1, 2


class EncodedBlock(NamedTuple):
    digest: str  # content_digest of the RAW block
    raw_len: int
    payload: Optional[bytes]  # None only when ``known(digest)`` said skip
    compressed: bool


#: what the last encode measured, for scripts/prof_snapshot.py
last_stats: dict = {"tail_hash_s": 0.0, "tail_hash_max_len": 0}

_codec_lock = threading.Lock()  # the scratch below is shared
_scratch: Any = None


class _Scratch:
    """Strided compress output (1.0625x the window) + dense containers (the
    window) + per-segment tables: ~135 MiB of HBM, allocated once."""

    def __init__(self) -> None:
        import torch

        self.n_seg = WINDOW // SEG_SIZE
        self.stride = torch.empty(self.n_seg * OUT_STRIDE, dtype=torch.uint8, device="cuda")
        self.dense = torch.empty(WINDOW, dtype=torch.uint8, device="cuda")
        self.comp_lens = torch.empty(self.n_seg, dtype=torch.int32, device="cuda")
        self.seg_off = torch.empty(self.n_seg, dtype=torch.int32, device="cuda")


def _get_scratch() -> Optional[_Scratch]:
    """None when HBM cannot spare it: the caller then stores raw blocks."""
    global _scratch
    if _scratch is None:
        try:
            _scratch = _Scratch()
        except RuntimeError:  # torch.OutOfMemoryError is one
            return None
    return _scratch


def release_scratch() -> None:
    global _scratch
    with _codec_lock:
        _scratch = None


def _stream() -> int:
    import torch

    return torch.cuda.current_stream().cuda_stream


def _sync() -> None:
    import torch

    torch.cuda.current_stream().synchronize()


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed: hipError {rc}")


def _to_dev(arr: np.ndarray) -> Any:
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


def _d2h(lib: Any, dev_ptr: int, n: int) -> bytes:
    """Device bytes -> host bytes through the pinned arena."""
    if n == 0:
        return b""
    from . import staging

    with staging._lock:
        staging._ensure(n)
        _check(lib.ma_malz_copy(staging._pin_buf.data_ptr(), dev_ptr, n, _D2H, _stream()), "D2H copy")
        _sync()
        return staging._pin_np[:n].tobytes()


def _h2d(lib: Any, dev_ptr: int, parts: Sequence) -> None:
    """Host buffers, concatenated -> device memory through the pinned arena."""
    total = sum(len(p) for p in parts)
    if total == 0:
        return
    from . import staging

    with staging._lock:
        staging._ensure(total)
        pos = 0
        for p in parts:
            staging._pin_np[pos : pos + len(p)] = np.frombuffer(p, dtype=np.uint8)
            pos += len(p)
        _check(lib.ma_malz_copy(dev_ptr, staging._pin_buf.data_ptr(), total, _H2D, _stream()), "H2D copy")
        _sync()  # the arena is reused by the next caller


def _sha_dispatch(lib: Any, base: int, offsets: np.ndarray, lengths: np.ndarray) -> np.ndarray:
    """One ma_sha256_many over (base + offsets[i], lengths[i]); [n, 32] on host."""
    import torch

    n = len(offsets)
    off_d = _to_dev(offsets.astype(np.int64))
    len_d = _to_dev(lengths.astype(np.int64))
    out = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    _check(
        lib.ma_sha256_many(base, off_d.data_ptr(), len_d.data_ptr(), out.data_ptr(), n, _stream()),
        "sha256 kernel",
    )
    return out.cpu().numpy()


def _short_digests(lib: Any, items: Sequence[tuple[int, int]]) -> list[str]:
    """Plain SHA-256 of many (absolute pointer, length) messages in ONE
    dispatch, one message per lane."""
    if not items:
        return []
    base = min(p for p, _n in items)
    offsets = np.array([p - base for p, _n in items], dtype=np.int64)
    lengths = np.array([n for _p, n in items], dtype=np.int64)
    import torch

    torch.cuda.current_stream().synchronize()
    t0 = time.perf_counter()
    dig = _sha_dispatch(lib, base, offsets, lengths)
    dt = time.perf_counter() - t0
    if dt > last_stats["tail_hash_s"]:
        last_stats["tail_hash_s"] = dt
        last_stats["tail_hash_max_len"] = int(lengths.max())
    return [dig[i].tobytes().hex() for i in range(len(items))]


def _tree_digests(lib: Any, ptr: int, spans: Sequence[tuple[int, int]]) -> list[str]:
    """Tree digests of blocks (offset, length) of the object at ptr: all
    leaves in one dispatch, roots on the host as hashing._root_digest."""
    if not spans:
        return []
    offs, lens, counts = [], [], []
    for off, ln in spans:
        n_leaves = -(-ln // LEAF_SIZE)
        o = off + np.arange(n_leaves, dtype=np.int64) * LEAF_SIZE
        l = np.full(n_leaves, LEAF_SIZE, dtype=np.int64)
        if ln % LEAF_SIZE:
            l[-1] = ln % LEAF_SIZE
        offs.append(o)
        lens.append(l)
        counts.append(n_leaves)
    leaves = _sha_dispatch(lib, ptr, np.concatenate(offs), np.concatenate(lens))
    out, first = [], 0
    for (_off, ln), n_leaves in zip(spans, counts):
        out.append(_root_digest(ln, leaves[first : first + n_leaves].tobytes()).hex())
        first += n_leaves
    return out


def verify_device(objects: Sequence[tuple[int, Sequence[tuple[str, int]]]]) -> None:
    """Re-hash decoded device memory against its manifest. ``objects`` is
    ``[(ptr, [(digest, raw_len), ...])]``, the blocks of each object in
    order. Every short block of the call shares ONE dispatch (a single lane
    takes ~0.5 s for a message just under 8 MiB, so a restore verifies all
    its objects in one call); full blocks hash a few blocks' leaves at a time.
    Raises ``ValueError("snapshot block <i> digest mismatch")``."""
    lib = load_lib(required=True)

    def mismatch(oi: int, bi: int) -> ValueError:
        where = f" in object {oi}" if len(objects) > 1 else ""
        return ValueError(f"snapshot block {bi} digest mismatch{where}")

    short_keys, short_items = [], []
    for oi, (ptr, blocks) in enumerate(objects):
        full: list[tuple[int, int, int]] = []  # (block index, offset, length)
        off = 0
        for bi, (_digest, ln) in enumerate(blocks):
            if ln < GPU_MIN_BYTES:
                short_keys.append((oi, bi))
                short_items.append((ptr + off, ln))
            else:
                full.append((bi, off, ln))
            off += ln
        for g in range(0, len(full), _TREE_GROUP):
            group = full[g : g + _TREE_GROUP]
            got = _tree_digests(lib, ptr, [(o, n) for _b, o, n in group])
            for (bi, _o, _n), d in zip(group, got):
                if d != blocks[bi][0]:
                    raise mismatch(oi, bi)
    for (oi, bi), d in zip(short_keys, _short_digests(lib, short_items)):
        if d != objects[oi][1][bi][0]:
            raise mismatch(oi, bi)


def _spans(nbytes: int, block_size: int) -> list[tuple[int, int]]:
    return [(off, min(block_size, nbytes - off)) for off in range(0, nbytes, block_size)]


def _check_block_size(block_size: int) -> None:
    if block_size <= 0 or block_size % SEG_SIZE or block_size > WINDOW:
        raise ValueError(
            f"block_size must be a multiple of {SEG_SIZE} and at most {WINDOW}, got {block_size}"
        )


# ---------------------------------------------------------------------------
# encode
# ---------------------------------------------------------------------------


def _encode_window(
    lib: Any, sc: _Scratch, ptr: int, spans: Sequence[tuple[int, int]],
    digests: list, known: Optional[Callable[[str], bool]],
) -> list[EncodedBlock]:
    """Blocks of one window (<= WINDOW source bytes) of the object at ptr.
    ``digests`` holds the short blocks' digests; full blocks are None."""
    tree = [i for i, d in enumerate(digests) if d is None]
    for i, d in zip(tree, _tree_digests(lib, ptr, [spans[i] for i in tree])):
        digests[i] = d
    skip = [known is not None and known(d) for d in digests]
    cand = [i for i, (_o, ln) in enumerate(spans) if ln >= COMPRESS_MIN and not skip[i]]
    containers: dict[int, bytes] = {}
    if cand:
        stream = _stream()
        first_seg, n_segs, sb = [], [], 0
        for i in cand:
            off, ln = spans[i]
            n_seg = -(-ln // SEG_SIZE)
            if sb + n_seg > sc.n_seg:
                raise RuntimeError("encode window exceeds the scratch")
            _check(
                lib.ma_lz4_compress(
                    ptr + off, ln, sc.stride.data_ptr() + sb * OUT_STRIDE,
                    sc.comp_lens.data_ptr() + sb * 4, OUT_STRIDE, n_seg, stream,
                ),
                "lz4 compress kernel",
            )
            first_seg.append(sb)
            n_segs.append(n_seg)
            sb += n_seg
        import torch

        first_d = _to_dev(np.array(first_seg, dtype=np.int32))
        raw_d = _to_dev(np.array([spans[i][1] for i in cand], dtype=np.int64))
        src_off_d = _to_dev(np.array([spans[i][0] for i in cand], dtype=np.int64))
        payload_d = torch.empty(len(cand), dtype=torch.int64, device="cuda")
        _check(
            lib.ma_malz_plan(
                sc.comp_lens.data_ptr(), first_d.data_ptr(), raw_d.data_ptr(),
                sc.seg_off.data_ptr(), payload_d.data_ptr(), len(cand), stream,
            ),
            "malz plan kernel",
        )
        totals = payload_d.cpu().numpy()  # the one sync of the window
        out_off, sizes, pos = [], [], 0
        for j, i in enumerate(cand):
            n = spans[i][1]
            total = int(totals[j])
            if total >= n * MIN_GAIN:  # the rule of compress.py, unchanged
                out_off.append(-1)
                sizes.append(0)
                continue
            size = HEADER_FIXED + 4 * n_segs[j] + total
            out_off.append(pos)
            sizes.append(size)
            pos += size
        if pos:
            if pos > sc.dense.numel():
                raise RuntimeError("dense containers exceed the scratch")
            out_off_d = _to_dev(np.array(out_off, dtype=np.int64))
            _check(
                lib.ma_malz_assemble(
                    ptr, src_off_d.data_ptr(), sc.stride.data_ptr(), OUT_STRIDE,
                    sc.comp_lens.data_ptr(), sc.seg_off.data_ptr(), first_d.data_ptr(),
                    raw_d.data_ptr(), sc.dense.data_ptr(), out_off_d.data_ptr(),
                    len(cand), stream,
                ),
                "malz assemble kernel",
            )
            dense = _d2h(lib, sc.dense.data_ptr(), pos)
            for j, i in enumerate(cand):
                if out_off[j] >= 0:
                    containers[i] = dense[out_off[j] : out_off[j] + sizes[j]]
    blocks = []
    for i, (off, ln) in enumerate(spans):
        if skip[i]:
            blocks.append(EncodedBlock(digests[i], ln, None, False))
        elif i in containers:
            blocks.append(EncodedBlock(digests[i], ln, containers[i], True))
        else:
            blocks.append(EncodedBlock(digests[i], ln, _d2h(lib, ptr + off, ln), False))
    return blocks


def _host_digest(data: bytes) -> str:
    """content_digest without touching the GPU (the no-scratch path)."""
    if len(data) < GPU_MIN_BYTES:
        return hashlib.sha256(data).hexdigest()
    return tree_sha256_cpu(data).hex()


def iter_encode_device(
    objects: Sequence[tuple[int, int]], *, block_size: int = BLOCK_SIZE,
    known: Optional[Callable[[str], bool]] = None,
) -> Iterator[tuple[int, EncodedBlock]]:
    """Encode several device objects ``(ptr, nbytes)``; yields
    ``(object index, block)`` in object then block order, a window at a time,
    so a consumer that stores each block holds at most a window of payload.

    Every short block (< 8 MiB: each object's tail, every small object) of
    the whole call hashes in ONE dispatch. ``known(digest)`` True means the
    caller already has the block: it is yielded with ``payload=None`` and is
    neither compressed nor copied."""
    _check_block_size(block_size)
    lib = load_lib(required=True)
    all_spans = [_spans(nbytes, block_size) for _ptr, nbytes in objects]
    with _codec_lock:
        sc = _get_scratch()
        short_keys, short_items = [], []
        if sc is not None:
            for oi, ((ptr, _n), spans) in enumerate(zip(objects, all_spans)):
                for bi, (off, ln) in enumerate(spans):
                    if ln < GPU_MIN_BYTES:
                        short_keys.append((oi, bi))
                        short_items.append((ptr + off, ln))
        short = dict(zip(short_keys, _short_digests(lib, short_items)))
    per = max(1, WINDOW // block_size)
    for oi, ((ptr, _n), spans) in enumerate(zip(objects, all_spans)):
        for w0 in range(0, len(spans), per):
            wspans = spans[w0 : w0 + per]
            with _codec_lock:
                if sc is None:
                    # HBM too full for the scratch: raw blocks, host digests
                    blocks = []
                    for off, ln in wspans:
                        data = _d2h(lib, ptr + off, ln)
                        blocks.append(EncodedBlock(_host_digest(data), ln, data, False))
                else:
                    digests = [short.get((oi, w0 + k)) for k in range(len(wspans))]
                    blocks = _encode_window(lib, sc, ptr, wspans, digests, known)
            for blk in blocks:
                yield oi, blk


def encode_device(ptr: int, nbytes: int, *, block_size: int = BLOCK_SIZE) -> list[EncodedBlock]:
    """CAS blocks of the ``nbytes`` at device pointer ``ptr``."""
    return [blk for _oi, blk in iter_encode_device([(ptr, nbytes)], block_size=block_size)]


def _tensor_span(t: Any) -> tuple[int, int]:
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError("device codec needs a contiguous CUDA tensor")
    return t.data_ptr(), t.numel() * t.element_size()


def encode_tensor(t: Any, *, block_size: int = BLOCK_SIZE) -> list[EncodedBlock]:
    ptr, nbytes = _tensor_span(t)
    return encode_device(ptr, nbytes, block_size=block_size)


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------


def validate_container(payload: bytes, raw_len: int, index: int) -> tuple[np.ndarray, np.ndarray, int]:
    """Bound everything a decompress launch will index with, on the host:
    magic, raw_len and n_seg against the manifest, every comp_len < 4096,
    header + sum(eff) == len(payload). Returns (comp_lens int32, eff int64,
    payload offset); raises ValueError naming block ``index``."""

    def bad(why: str) -> ValueError:
        return ValueError(f"snapshot block {index}: {why}")

    n = len(payload)
    if n < HEADER_FIXED or bytes(payload[: len(MAGIC)]) != MAGIC:
        raise bad("not a MALZ41 container")
    hdr_raw, n_seg = struct.unpack_from("<QI", payload, len(MAGIC))
    if hdr_raw != raw_len:
        raise bad(f"container raw_len {hdr_raw} != manifest {raw_len}")
    if n_seg != -(-raw_len // SEG_SIZE):
        raise bad(f"container has {n_seg} segments for {raw_len} bytes")
    off = HEADER_FIXED + 4 * n_seg
    if n < off:
        raise bad("container truncated inside its segment table")
    comp_lens = np.frombuffer(payload, dtype="<u4", count=n_seg, offset=HEADER_FIXED)
    if n_seg and int(comp_lens.max()) >= SEG_SIZE:
        raise bad("segment comp_len out of range")
    seg_raw = np.full(n_seg, SEG_SIZE, dtype=np.int64)
    if n_seg:
        seg_raw[-1] = raw_len - (n_seg - 1) * SEG_SIZE
    eff = np.where(comp_lens == 0, seg_raw, comp_lens.astype(np.int64))
    if off + int(eff.sum()) != n:
        raise bad(f"container is {n} bytes, header says {off + int(eff.sum())}")
    return comp_lens.astype(np.int32), eff, off


def _check_layout(blocks: Sequence, nbytes: int) -> None:
    total = 0
    for i, (_d, raw_len, payload, compressed) in enumerate(blocks):
        if raw_len <= 0 or (i < len(blocks) - 1 and raw_len % SEG_SIZE):
            raise ValueError(f"snapshot block {i}: bad raw_len {raw_len}")
        if not compressed and len(payload) != raw_len:
            raise ValueError(f"snapshot block {i}: {len(payload)} raw bytes, manifest {raw_len}")
        total += raw_len
    if total != nbytes:
        raise ValueError(f"snapshot blocks hold {total} bytes, destination {nbytes}")


def decode_to_device(blocks: Sequence, ptr: int, nbytes: int, *, verify: bool = True) -> None:
    """Decode ``[(digest, raw_len, payload, compressed)]`` into the ``nbytes``
    of device memory at ``ptr``. Every container header is validated against
    the manifest before anything is launched."""
    _check_layout(blocks, nbytes)
    parsed: dict[int, tuple] = {}
    for i, (_d, raw_len, payload, compressed) in enumerate(blocks):
        if compressed:
            parsed[i] = validate_container(payload, raw_len, i)
    if not blocks:
        return
    lib = load_lib(required=True)
    import torch

    offs = np.concatenate([[0], np.cumsum([b[1] for b in blocks])]).astype(np.int64)
    # maximal runs of consecutive compressed blocks, cut to the staging window
    runs: list[list[int]] = []
    staged = 0
    for i in range(len(blocks)):
        if i not in parsed:
            continue
        size = len(blocks[i][2]) - parsed[i][2]
        if runs and runs[-1][-1] == i - 1 and len(runs[-1]) < RUN_MAX_BLOCKS and staged + size <= WINDOW:
            runs[-1].append(i)
            staged += size
        else:
            runs.append([i])
            staged = size
    with _codec_lock:
        stream = _stream()
        status = torch.zeros(max(len(runs), 1), dtype=torch.int32, device="cuda")
        for r, run in enumerate(runs):
            comp_lens = np.concatenate([parsed[i][0] for i in run])
            eff = np.concatenate([parsed[i][1] for i in run])
            comp_offs = np.cumsum(eff) - eff  # exclusive
            parts = [memoryview(blocks[i][2])[parsed[i][2] :] for i in run]
            comp = torch.empty(int(eff.sum()), dtype=torch.uint8, device="cuda")
            _h2d(lib, comp.data_ptr(), parts)
            offs_d = _to_dev(comp_offs.astype(np.int64))
            lens_d = _to_dev(comp_lens)
            run_raw = int(offs[run[-1] + 1] - offs[run[0]])
            _check(
                lib.ma_lz4_decompress(
                    comp.data_ptr(), offs_d.data_ptr(), lens_d.data_ptr(),
                    ptr + int(offs[run[0]]), run_raw, status.data_ptr() + 4 * r,
                    len(comp_lens), stream,
                ),
                "lz4 decompress kernel",
            )
            _sync()  # comp and the tables are freed on the next iteration
        for i, (_d, raw_len, payload, compressed) in enumerate(blocks):
            if not compressed:
                _h2d(lib, ptr + int(offs[i]), [payload])
        bad = status.cpu().numpy()
        for r, run in enumerate(runs):
            if bad[r]:
                raise ValueError(
                    f"snapshot blocks {run[0]}..{run[-1]}: LZ4 container corrupt "
                    f"at segment {int(bad[r]) - 1} of the run"
                )
    if verify:
        verify_device([(ptr, [(b[0], b[1]) for b in blocks])])


def decode_tensor(blocks: Sequence, t: Any, *, verify: bool = True) -> None:
    ptr, nbytes = _tensor_span(t)
    decode_to_device(blocks, ptr, nbytes, verify=verify)


# ---------------------------------------------------------------------------
# GPU-less twins
# ---------------------------------------------------------------------------


def encode_host(data: Any, *, block_size: int = BLOCK_SIZE) -> list[EncodedBlock]:
    """Same manifest from host bytes (CPU tensors, CPU-only processes)."""
    _check_block_size(block_size)
    from .compress import compress_buffer

    view = memoryview(data).cast("B")
    blocks = []
    for off, ln in _spans(len(view), block_size):
        block = bytes(view[off : off + ln])
        z = compress_buffer(block) if ln >= COMPRESS_MIN else None
        if z is not None:
            blocks.append(EncodedBlock(content_digest(block), ln, z, True))
        else:
            blocks.append(EncodedBlock(content_digest(block), ln, block, False))
    return blocks


def decode_host(blocks: Sequence, *, verify: bool = True) -> bytes:
    from .compress import decompress_buffer_cpu

    _check_layout(blocks, sum(b[1] for b in blocks))
    out = []
    for i, (digest, raw_len, payload, compressed) in enumerate(blocks):
        if compressed:
            validate_container(payload, raw_len, i)
            data = decompress_buffer_cpu(payload)
            if len(data) != raw_len:
                raise ValueError(f"snapshot block {i}: decoded {len(data)} bytes, manifest {raw_len}")
        else:
            data = bytes(payload)
        if verify and content_digest(data) != digest:
            raise ValueError(f"snapshot block {i} digest mismatch")
        out.append(data)
    return b"".join(out)

"""Block codec for device-resident state: hash, compress and frame on the GPU.

A GPU snapshot's payload already lives in HBM, and the SHA-256 and LZ4
kernels take device pointers, so an object (a tensor's storage, a tracked
raw allocation) is encoded where it is: split into CAS blocks of
``BLOCK_SIZE``, every block hashed in place, and a window of blocks at a time
handed to ``compress.compress_spans_gpu``, the one device encoder, which also
serves ``BlobStore.put``. Only the dense containers, or the raw bytes of
blocks that do not compress, cross to the host. Decoding validates every
container header on the host, stages the compressed bytes H2D and decompresses
straight into the destination allocation, with ``validate_container`` and
``decompress_run_gpu`` of the codec the magic selects (``compress.codec_of``).

An object the caller hints as float data (``elem_size`` 2 or 4) offers the
blocks LZ4 declined to the float-plane codec (ops/fpcodec.py, MAFP10); an
object of no known element type (``fpcodec.AUTO``) has those blocks probed on
the device for the element size at which the codec pays, if any. Both
codecs stand on ops/container.py and both validators return headers that
begin (raw_len, seg lens, payload offset): nothing here tells them apart.

What this module adds to those is the block layer: digests, skipping blocks
the CAS already has, the cached 64 MiB scratch with its out-of-memory
fallback, runs of consecutive compressed blocks on decode, verification.

The low level works on ``(device pointer, nbytes)`` so torch tensors and
``rawmem`` allocations share it. ``encode_host``/``decode_host`` are the
GPU-less twins: same digests (``hashing.content_digest`` of the block), same
manifests, containers not necessarily byte-identical.
"""

from __future__ import annotations

import threading
import time
from typing import Any, Callable, Iterator, NamedTuple, Optional, Sequence

import numpy as np

from ..scheduler.blobs import BLOCK_SIZE, BlobStore
from . import compress, fpcodec, load_lib
from .container import SEG_SIZE, Workspace
from .hashing import GPU_MIN_BYTES, content_digest, leaf_table, sha256_leaves_gpu, tree_roots
from .staging import copy_from_device, copy_to_device

WINDOW = 64 * 1024 * 1024  # source bytes encoded per plan/assemble round
COMPRESS_MIN = BlobStore.COMPRESS_MIN
RUN_MAX_BLOCKS = 128  # decode: blocks per decompress launch, at most
_ELEM_SIZES = (0, *fpcodec.ELEM_SIZES, fpcodec.AUTO)  # what an element size hint may be
_TREE_GROUP = 8  # verify: full blocks whose leaves share one hash dispatch


class EncodedBlock(NamedTuple):
    digest: str  # content_digest of the RAW block
    raw_len: int
    payload: Optional[bytes]  # None only when ``known(digest)`` said skip
    compressed: bool


#: what the last encode measured, for scripts/prof_snapshot.py
last_stats: dict = {"tail_hash_s": 0.0, "tail_hash_max_len": 0}

_codec_lock = threading.Lock()  # the scratch below is shared
_scratch: Any = None


def _get_scratch() -> Optional[Workspace]:
    """Strided compress output (1.0625x the window) + dense containers (the
    window) + per-segment tables: ~135 MiB of HBM, allocated once. None when
    HBM cannot spare it: the caller then stores raw blocks."""
    global _scratch
    if _scratch is None:
        try:
            _scratch = Workspace(WINDOW // SEG_SIZE, WINDOW)
        except RuntimeError:  # torch.OutOfMemoryError is one
            return None
    return _scratch


def release_scratch() -> None:
    global _scratch
    with _codec_lock:
        _scratch = None


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
    dig = sha256_leaves_gpu(lib, base, offsets, lengths)
    dt = time.perf_counter() - t0
    if dt > last_stats["tail_hash_s"]:
        last_stats["tail_hash_s"] = dt
        last_stats["tail_hash_max_len"] = int(lengths.max())
    return [dig[i].tobytes().hex() for i in range(len(items))]


def _tree_digests(lib: Any, ptr: int, spans: Sequence[tuple[int, int]]) -> list[str]:
    """Tree digests of blocks (offset, length) of the object at ptr: all
    leaves in one dispatch, roots on the host (hashing.tree_roots)."""
    if not spans:
        return []
    offsets, lengths, counts = leaf_table(spans)
    leaves = sha256_leaves_gpu(lib, ptr, offsets, lengths)
    return [root.hex() for root in tree_roots(spans, counts, leaves.tobytes())]


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
    lib: Any, sc: Workspace, ptr: int, spans: Sequence[tuple[int, int]],
    digests: list, known: Optional[Callable[[str], bool]], elem_size: int = 0,
) -> list[EncodedBlock]:
    """Blocks of one window (<= WINDOW source bytes) of the object at ptr.
    ``digests`` holds the short blocks' digests; full blocks are None. With
    ``elem_size`` 2 or 4 the blocks LZ4 declined go through the float-plane
    codec on the same scratch (LZ4 first: a zero-filled float tensor is 0.4 %
    under LZ4 and 56 % under MAFP10). With ``fpcodec.AUTO`` they are probed
    first and each goes through it at the element size the probe found, or
    stays raw where it found none."""
    tree = [i for i, d in enumerate(digests) if d is None]
    for i, d in zip(tree, _tree_digests(lib, ptr, [spans[i] for i in tree])):
        digests[i] = d
    skip = [known is not None and known(d) for d in digests]
    cand = [i for i, (_o, ln) in enumerate(spans) if ln >= COMPRESS_MIN and not skip[i]]
    containers = dict(
        zip(cand, compress.compress_spans_gpu(lib, ptr, [spans[i] for i in cand], sc))
    )
    left = [i for i in cand if containers[i] is None] if elem_size else []
    if elem_size == fpcodec.AUTO and left:
        # one probe of all of them, then one encode per element size it
        # found, each on its rows of the probe's tables
        found, tables = fpcodec.probe_spans_gpu(lib, ptr, [spans[i] for i in left])
        for col, es in enumerate(fpcodec.ELEM_SIZES):
            rows = [k for k, e in enumerate(found) if e == es]
            if rows:
                # the usual window is of one kind: no index tensor to upload
                mine = tables if len(rows) == len(found) else tables[rows]
                z = fpcodec.compress_spans_gpu(
                    lib, ptr, [spans[left[k]] for k in rows], es, sc,
                    counts=mine[:, col].contiguous(),
                )
                containers.update(zip([left[k] for k in rows], z))
    elif left:
        containers.update(
            zip(left, fpcodec.compress_spans_gpu(lib, ptr, [spans[i] for i in left], elem_size, sc))
        )
    blocks = []
    for i, (off, ln) in enumerate(spans):
        if skip[i]:
            blocks.append(EncodedBlock(digests[i], ln, None, False))
        elif containers.get(i) is not None:
            blocks.append(EncodedBlock(digests[i], ln, containers[i], True))
        else:
            blocks.append(EncodedBlock(digests[i], ln, copy_from_device(ptr + off, ln), False))
    return blocks


def iter_encode_device(
    objects: Sequence[tuple[int, int]], *, block_size: int = BLOCK_SIZE,
    known: Optional[Callable[[str], bool]] = None,
    elem_sizes: Optional[Sequence[int]] = None,
) -> Iterator[tuple[int, EncodedBlock]]:
    """Encode several device objects ``(ptr, nbytes)``; yields
    ``(object index, block)`` in object then block order, a window at a time,
    so a consumer that stores each block holds at most a window of payload.

    Every short block (< 8 MiB: each object's tail, every small object) of
    the whole call hashes in ONE dispatch. ``known(digest)`` True means the
    caller already has the block: it is yielded with ``payload=None`` and is
    neither compressed nor copied. ``elem_sizes`` has one entry per object:
    2 or 4 offers the blocks LZ4 declined to the float-plane codec
    (ops/fpcodec.py), ``fpcodec.AUTO`` offers them at the element size a
    probe of their bytes finds (per block; none: raw), 0 does not; digests
    are of the RAW block either way."""
    _check_block_size(block_size)
    if elem_sizes is None:
        elem_sizes = [0] * len(objects)
    if len(elem_sizes) != len(objects) or any(es not in _ELEM_SIZES for es in elem_sizes):
        raise ValueError("elem_sizes needs one of 0, 2, 4, fpcodec.AUTO per object")
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
                        data = copy_from_device(ptr + off, ln)
                        blocks.append(EncodedBlock(content_digest(data, gpu=False), ln, data, False))
                else:
                    digests = [short.get((oi, w0 + k)) for k in range(len(wspans))]
                    blocks = _encode_window(lib, sc, ptr, wspans, digests, known, elem_sizes[oi])
            for blk in blocks:
                yield oi, blk


def encode_device(
    ptr: int, nbytes: int, *, block_size: int = BLOCK_SIZE, elem_size: int = 0
) -> list[EncodedBlock]:
    """CAS blocks of the ``nbytes`` at device pointer ``ptr``."""
    it = iter_encode_device([(ptr, nbytes)], block_size=block_size, elem_sizes=[elem_size])
    return [blk for _oi, blk in it]


def _tensor_span(t: Any) -> tuple[int, int]:
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError("device codec needs a contiguous CUDA tensor")
    return t.data_ptr(), t.numel() * t.element_size()


def encode_tensor(
    t: Any, *, block_size: int = BLOCK_SIZE, elem_size: int = 0
) -> list[EncodedBlock]:
    """``elem_size`` is the caller's to give: it is not inferred from t's
    dtype (``fpcodec.AUTO`` infers it from the bytes)."""
    ptr, nbytes = _tensor_span(t)
    return encode_device(ptr, nbytes, block_size=block_size, elem_size=elem_size)


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------


def validate_container(payload: bytes, raw_len: int, index: int, codec: Any = None) -> tuple:
    """The header of a stored container, (raw_len, seg lens, payload offset,
    ...), from the validator of ``codec`` (``compress.codec_of`` when not
    given) against the manifest's raw_len; the ValueError names block ``index``."""
    codec = codec or compress.codec_of(payload)
    return codec.validate_container(payload, raw_len, f"snapshot block {index}")


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
    parsed: dict[int, tuple] = {}  # block -> (codec, header)
    for i, (_d, raw_len, payload, compressed) in enumerate(blocks):
        if compressed:
            codec = compress.codec_of(payload)
            parsed[i] = codec, validate_container(payload, raw_len, i, codec)
    if not blocks:
        return
    lib = load_lib(required=True)
    import torch

    offs = np.concatenate([[0], np.cumsum([b[1] for b in blocks])]).astype(np.int64)
    # maximal runs of consecutive compressed blocks of one codec, cut to the
    # staging window
    runs: list[list[int]] = []
    staged = 0
    for i in range(len(blocks)):
        if i not in parsed:
            continue
        size = len(blocks[i][2]) - parsed[i][1].payload_off
        if (
            runs and runs[-1][-1] == i - 1 and parsed[i - 1][0] is parsed[i][0]
            and len(runs[-1]) < RUN_MAX_BLOCKS and staged + size <= WINDOW
        ):
            runs[-1].append(i)
            staged += size
        else:
            runs.append([i])
            staged = size
    with _codec_lock:
        for run in runs:
            codec = parsed[run[0]][0]
            parts = [memoryview(blocks[i][2])[parsed[i][1].payload_off :] for i in run]
            comp = torch.empty(sum(len(p) for p in parts), dtype=torch.uint8, device="cuda")
            copy_to_device(comp.data_ptr(), parts)
            headers = [parsed[i][1] for i in run]
            bad = codec.decompress_run_gpu(lib, comp.data_ptr(), headers, ptr + int(offs[run[0]]))
            if bad:
                raise ValueError(
                    f"snapshot blocks {run[0]}..{run[-1]}: {codec.corrupt_message(bad)} of the run"
                )
        for i, (_d, raw_len, payload, compressed) in enumerate(blocks):
            if not compressed:
                copy_to_device(ptr + int(offs[i]), [payload])
    if verify:
        verify_device([(ptr, [(b[0], b[1]) for b in blocks])])


def decode_tensor(blocks: Sequence, t: Any, *, verify: bool = True) -> None:
    ptr, nbytes = _tensor_span(t)
    decode_to_device(blocks, ptr, nbytes, verify=verify)


# ---------------------------------------------------------------------------
# GPU-less twins
# ---------------------------------------------------------------------------


def encode_host(
    data: Any, *, block_size: int = BLOCK_SIZE, elem_size: int = 0
) -> list[EncodedBlock]:
    """Same manifest from host bytes (CPU tensors, CPU-only processes).
    ``fpcodec.AUTO`` runs the probe's numpy twin on every block LZ4 declined."""
    _check_block_size(block_size)
    if elem_size not in _ELEM_SIZES:
        raise ValueError("elem_size is one of 0, 2, 4, fpcodec.AUTO")
    from .compress import compress_buffer

    view = memoryview(data).cast("B")
    blocks = []
    for off, ln in _spans(len(view), block_size):
        block = bytes(view[off : off + ln])
        z = compress_buffer(block) if ln >= COMPRESS_MIN else None
        es = elem_size
        if z is None and es == fpcodec.AUTO and ln >= COMPRESS_MIN:
            es = fpcodec.choose_elem_size(*fpcodec.probe_counts_cpu(block), ln)[0]
        if z is None and es and ln >= COMPRESS_MIN:
            z = fpcodec.compress_buffer(block, es)
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

"""Content hashing: plain SHA-256 for small payloads, GPU tree-SHA-256 above.

The reference hashes every blob/Volume block with streaming SHA-256 on the
CPU (/root/reference/py/modal/_utils/hash_utils.py:68; 8 MiB Volume blocks
blob_utils.py:63). SHA-256 of one message is inherently serial, so the GPU
design re-shapes the problem: a buffer is split into 64 KiB leaves, every
leaf hashed by one CDNA4 lane (csrc/sha256.hip), and the content digest is
SHA-256 over the concatenated leaf digests with a domain separator. The CPU
reference implementation below produces bit-identical digests, so the CAS is
consistent across GPU-ful and GPU-less processes, and kernel correctness is
testable against hashlib.

Small payloads bypass the GPU entirely (SURVEY.md §7 hard part 7: keep
``.remote()`` p50 low — the crossover is config ``gpu_hash_threshold``).
"""

from __future__ import annotations

import hashlib
import struct
from typing import Any, Optional, Sequence, Union

from . import gpu_available, load_lib

# Leaf size trades tree overhead against GPU parallelism: SHA-256 is serial
# within a leaf, so leaves are the unit of parallelism. Swept 4/8/16/32 KiB
# on MI355X (profiles/README.md): 8 KiB wins (911 GiB/s at 512 MiB) — enough
# waves to hide the round-dependency chain, padding overhead still small.
LEAF_SIZE = 8 * 1024
TREE_DOMAIN = b"modal-amd-tree-v1"
GPU_MIN_BYTES = 8 * 1024 * 1024  # below this, CPU wins (kernel+copy overhead)

Buffer = Union[bytes, bytearray, memoryview]


def _root_digest(total_len: int, leaf_digests: bytes) -> bytes:
    h = hashlib.sha256()
    h.update(TREE_DOMAIN)
    h.update(struct.pack("<Q", total_len))
    h.update(leaf_digests)
    return h.digest()


def tree_sha256_cpu(data: Buffer) -> bytes:
    data = memoryview(data)
    digests = bytearray()
    for off in range(0, len(data), LEAF_SIZE):
        digests += hashlib.sha256(data[off : off + LEAF_SIZE]).digest()
    return _root_digest(len(data), bytes(digests))


def leaf_table(spans: Sequence[tuple[int, int]]) -> tuple:
    """The tree hash's leaves for buffers ``[(base_offset, length)]`` laid
    out in one address space: (offsets int64, lengths int64, leaves per
    span), span after span, every leaf LEAF_SIZE long but a span's last."""
    import numpy as np

    base = np.array([off for off, _n in spans], dtype=np.int64)
    size = np.array([n for _off, n in spans], dtype=np.int64)
    counts = -(-size // LEAF_SIZE)
    # offset of every leaf inside its span: 0, LEAF_SIZE, ... per span. All
    # in place: `temporary - x` on arrays this size makes numpy look for an
    # elidable temporary with backtrace(), whose first call in a process
    # that has torch loaded costs 0.1-0.3 s
    within = np.arange(int(counts.sum()), dtype=np.int64)
    within -= np.repeat(np.cumsum(counts) - counts, counts)
    within *= LEAF_SIZE
    offsets = np.repeat(base, counts)
    offsets += within
    lengths = np.repeat(size, counts)
    lengths -= within
    np.minimum(lengths, LEAF_SIZE, out=lengths)
    return offsets, lengths, counts


def tree_roots(spans: Sequence[tuple[int, int]], counts: Any, leaf_digests: bytes) -> list[bytes]:
    """Root digests of the spans of a ``leaf_table`` from its leaves' digests."""
    roots, first = [], 0
    for (_off, n), n_leaves in zip(spans, counts):
        roots.append(_root_digest(n, leaf_digests[first * 32 : (first + int(n_leaves)) * 32]))
        first += int(n_leaves)
    return roots


def sha256_leaves_gpu(lib: Any, base: int, offsets: Any, lengths: Any) -> Any:
    """One ma_sha256_many over (base + offsets[i], lengths[i]), numpy int64
    tables, on the current stream; [n, 32] uint8 on the host."""
    import torch

    n = len(offsets)
    off_d = torch.from_numpy(offsets).cuda()
    len_d = torch.from_numpy(lengths).cuda()
    out = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    rc = lib.ma_sha256_many(
        base, off_d.data_ptr(), len_d.data_ptr(), out.data_ptr(), n,
        torch.cuda.current_stream().cuda_stream,
    )
    if rc != 0:
        raise RuntimeError(f"sha256 kernel failed: hipError {rc}")
    return out.cpu().numpy()


def _tree_sha256_gpu(data: Buffer) -> Optional[bytes]:
    lib = load_lib(required=True)
    from .staging import stage_to_gpu

    src = stage_to_gpu(data)  # pinned arena + side-stream hipMemcpyAsync
    offsets, lengths, _counts = leaf_table([(0, len(data))])
    leaves = sha256_leaves_gpu(lib, src.data_ptr(), offsets, lengths)
    return _root_digest(len(data), leaves.tobytes())


def sha256_many_gpu(
    buf: "object", offsets: "object", lengths: "object", ilp: int = 1
) -> "object":
    """Hash arbitrary (offset, length) slices of a GPU-resident uint8 tensor.

    Returns an [n, 32] uint8 CUDA tensor of standard SHA-256 digests.
    ilp=2 uses the dual-chain kernel (two messages per lane, interleaved
    rounds) — wins when occupancy is low (few messages).
    """
    lib = load_lib(required=True)
    import torch

    assert buf.dtype == torch.uint8 and buf.is_cuda
    n = len(offsets)
    offsets_d = offsets.to(device="cuda", dtype=torch.int64)
    lengths_d = lengths.to(device="cuda", dtype=torch.int64)
    out = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    fn = lib.ma_sha256_many2 if ilp == 2 else lib.ma_sha256_many
    rc = fn(
        buf.data_ptr(), offsets_d.data_ptr(), lengths_d.data_ptr(), out.data_ptr(),
        n, torch.cuda.current_stream().cuda_stream,
    )
    if rc != 0:
        raise RuntimeError(f"sha256 kernel failed: hipError {rc}")
    return out


def tree_sha256(data: Buffer) -> bytes:
    """GPU when it pays, CPU otherwise; identical digests either way."""
    if len(data) >= GPU_MIN_BYTES and gpu_available():
        return _tree_sha256_gpu(data)
    return tree_sha256_cpu(data)


def content_digests_batch(
    buffers: list, gpu_threshold: int = GPU_MIN_BYTES, staged: "object" = None
) -> list[str]:
    """CAS keys for many buffers with ONE kernel launch over all leaves.

    This is the volume-upload hot path: a multi-GiB file's 8 MiB blocks hash
    in a single batched dispatch (thousands of leaves -> full chip), instead
    of one under-occupied launch per block.
    """
    total = sum(len(b) for b in buffers)
    if total < gpu_threshold or not gpu_available():
        return [content_digest(b, gpu_threshold) for b in buffers]
    lib = load_lib(required=True)
    # digest form must depend only on the buffer's own size so every path
    # (single, batch, CPU, GPU) computes the same CAS key
    results: list = [
        content_digest(b, gpu_threshold) if len(b) < gpu_threshold else None for b in buffers
    ]
    big = [i for i, d in enumerate(results) if d is None]
    if not big:
        return results
    if staged is not None:
        # caller pre-staged ALL buffers (one pinned H2D shared with the
        # compression pass, blobs.put_many)
        src, all_offsets = staged
        bases = [all_offsets[i] for i in big]
    else:
        from .staging import stage_many_to_gpu

        # one pinned H2D for all large buffers (no concat bytearray pass)
        src, bases = stage_many_to_gpu([buffers[i] for i in big], align=LEAF_SIZE)
    spans = [(base, len(buffers[i])) for base, i in zip(bases, big)]
    offsets, lengths, counts = leaf_table(spans)
    leaves = sha256_leaves_gpu(lib, src.data_ptr(), offsets, lengths)
    for i, root in zip(big, tree_roots(spans, counts, leaves.tobytes())):
        results[i] = root.hex()
    return results


def content_digest(data: Buffer, gpu_threshold: int = GPU_MIN_BYTES, *, gpu: bool = True) -> str:
    """The CAS key: plain SHA-256 below the threshold, tree digest above.

    Deterministic for a given payload size, so every process computes the
    same key regardless of whether it has a GPU; ``gpu=False`` keeps the
    tree hash on the host whatever the machine has.
    """
    if len(data) < gpu_threshold:
        return hashlib.sha256(data).hexdigest()
    return (tree_sha256(data) if gpu else tree_sha256_cpu(data)).hex()

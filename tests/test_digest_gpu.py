"""The content-digest path and the segment copy kernel on the GPU against
references they do not share: the SHA-256 kernels against hashlib, the tree,
batch and pipelined digests against the host tree hash, the pipelined
containers against the compressor's model, pack/unpack against numpy. The
inputs and expectations come from tests/digest_corpus.py, whose self-checks
are tests/test_digest_corpus_cpu.py. Every comparison is exact."""

from __future__ import annotations

import functools
import hashlib
import threading

import numpy as np
import pytest

import digest_corpus as corpus
from digest_corpus import CANARY, THRESHOLD, WINDOW, expected_container, expected_digest
from modal_amd.ops.hashing import LEAF_SIZE

pytestmark = pytest.mark.gpu

GUARD = 4096  # canary bytes either side of an output a raw library call writes
ILP = (1, 2)
SHA_SYMBOL = {1: "ma_sha256_many", 2: "ma_sha256_many2"}


def _feature():
    """The ops library with the kernels under test. Raises where it is
    missing, so a build without it fails these tests, not skips them."""
    # torch first: loaded after the library it brings a second HIP runtime
    # into the process, and the library's launches then find no device
    import torch  # noqa: F401

    from modal_amd.ops import load_lib

    lib = load_lib(required=True)
    for symbol in (
        "ma_sha256_many", "ma_sha256_many2", "ma_pack_segments", "ma_unpack_segments",
        "ma_lz4_compress",
    ):
        getattr(lib, symbol)
    return lib


def _guarded(nbytes: int, fill: int = CANARY):
    """A device buffer of nbytes inside a larger one, GUARD canary bytes
    either side. Returns (whole tensor, interior view)."""
    import torch

    whole = torch.full((GUARD + nbytes + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    inner = whole[GUARD : GUARD + nbytes]
    if fill != CANARY:
        inner.fill_(fill)
    return whole, inner


def _guards_intact(whole) -> bool:
    host = whole.cpu().numpy()
    return bool((host[:GUARD] == CANARY).all() and (host[-GUARD:] == CANARY).all())


def _to_device(array: np.ndarray):
    """A host array on the device, its base 16-aligned: the residues of the
    corpus are residues of device addresses."""
    import torch

    dev = torch.from_numpy(np.ascontiguousarray(array)).cuda()
    assert dev.data_ptr() % 16 == 0
    return dev


def _i64(values):
    import torch

    return torch.tensor(list(values), dtype=torch.int64)


def _digest_rows(out) -> list:
    host = out.cpu().numpy().tobytes()
    return [host[i : i + 32] for i in range(0, len(host), 32)]


def _hash_layout(lay: corpus.Layout, ilp: int) -> list:
    from modal_amd.ops.hashing import sha256_many_gpu

    buf = _to_device(lay.data)
    out = sha256_many_gpu(buf, _i64(lay.offsets), _i64(lay.lengths), ilp=ilp)
    assert tuple(out.shape) == (len(lay.offsets), 32)
    return _digest_rows(out)


# ---------------------------------------------------------------------------
# SHA-256 kernels against hashlib
# ---------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _edge_layout() -> tuple:
    lay = corpus.layout(*corpus.edge_cases(), seed=1)
    return lay, tuple(corpus.sha_digests(lay))


@pytest.mark.parametrize("ilp", ILP)
def test_sha256_every_edge_length_at_every_residue(ilp):
    _feature()
    lay, want = _edge_layout()
    got = _hash_layout(lay, ilp)
    assert len(got) == 19 * 16
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"length {lay.lengths[i]} at residue {lay.offsets[i] % 16}"


@pytest.mark.parametrize("ilp", ILP)
@pytest.mark.parametrize("name", sorted(corpus.pair_position_lists()))
def test_sha256_pair_positions(ilp, name):
    _feature()
    lengths = corpus.pair_position_lists()[name]
    lay = corpus.layout(lengths, [(5 * i) % 16 for i in range(len(lengths))], seed=2)
    got = _hash_layout(lay, ilp)
    for i, (g, w) in enumerate(zip(got, corpus.sha_digests(lay))):
        assert g == w, f"message {i} of {lengths[i]} bytes, slot {'AB'[i % 2]}"


GRID_N = (1, 2, 255, 256, 257, 511, 512, 513, 514, 1025)


@functools.lru_cache(maxsize=None)
def _grid_messages() -> tuple:
    lay = corpus.grid_messages(max(GRID_N))
    return lay, b"".join(corpus.sha_digests(lay))


@pytest.mark.parametrize("ilp", ILP)
def test_sha256_grid_edges(ilp):
    """n either side of one and two workgroups of 256 lanes (512 and 1024
    messages for the pair kernel), odd n across those edges: n rows right,
    and nothing written before row 0 or from row n on."""
    import torch

    lib = _feature()
    fn = getattr(lib, SHA_SYMBOL[ilp])
    lay, want = _grid_messages()
    buf = _to_device(lay.data)
    offsets, lengths = _i64(lay.offsets).cuda(), _i64(lay.lengths).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for n in GRID_N:
        whole, out = _guarded(n * 32)
        rc = fn(buf.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), out.data_ptr(), n, stream)
        assert rc == 0
        got = out.cpu().numpy().tobytes()
        for i in range(n):
            assert got[i * 32 : (i + 1) * 32] == want[i * 32 : (i + 1) * 32], f"n={n}: row {i}"
        assert _guards_intact(whole), f"n={n}"
    whole, out = _guarded(64)
    assert fn(buf.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), out.data_ptr(), 0, stream) == 0
    assert bool((whole.cpu() == CANARY).all())


@pytest.mark.parametrize("ilp", ILP)
def test_sha256_arbitrary_table(ilp):
    _feature()
    table = corpus.arbitrary_table()
    got = _hash_layout(table, ilp)
    for i, (g, w) in enumerate(zip(got, corpus.sha_digests(table))):
        assert g == w, f"row {i}: span {(table.offsets[i], table.lengths[i])}"
    assert got[1] == got[6] and got[8] == got[9] == got[11] == hashlib.sha256(b"").digest()


# ---------------------------------------------------------------------------
# tree, batch and pipelined digests against the host references
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("size", corpus.tree_sizes())
def test_tree_sha256_gpu_small_sizes(size):
    """_tree_sha256_gpu has no threshold of its own, so small inputs reach the
    kernel. The expectation, at threshold 1, is tree_sha256_cpu's."""
    from modal_amd.ops.hashing import _tree_sha256_gpu

    _feature()
    data = corpus.tree_input(size)
    assert _tree_sha256_gpu(data).hex() == expected_digest(data, 1)


def test_swapped_leaves_change_the_host_tree_digest():
    """The negative control, on the host: the reference sees two full leaves
    exchanged, so the comparisons above see a kernel that exchanges them."""
    from modal_amd.ops.hashing import tree_sha256_cpu

    data = corpus.tree_input(256 * LEAF_SIZE + 1)
    assert tree_sha256_cpu(corpus.swap_leaves(data, 0, 255)) != tree_sha256_cpu(data)


@functools.lru_cache(maxsize=None)
def _pipeline_expectations() -> tuple:
    blocks = corpus.pipeline_blocks()
    return (
        tuple(expected_digest(b, THRESHOLD) for b in blocks),
        tuple(expected_container(b) for b in blocks),
    )


@pytest.mark.parametrize("staging", ["unstaged", "leaf_aligned", "byte_aligned"])
def test_content_digests_batch_against_host(staging):
    from modal_amd.ops.hashing import content_digests_batch
    from modal_amd.ops.staging import stage_many_to_gpu

    _feature()
    buffers = list(corpus.pipeline_blocks())
    staged = None
    if staging == "leaf_aligned":  # what BlobStore.put_many passes
        staged = stage_many_to_gpu(buffers, align=LEAF_SIZE)
    elif staging == "byte_aligned":  # leaves at every residue: placement must not matter
        staged = stage_many_to_gpu(buffers, align=1)
        assert any(o % 16 for o, b in zip(staged[1], buffers) if len(b) >= THRESHOLD)
    got = content_digests_batch(buffers, gpu_threshold=THRESHOLD, staged=staged)
    assert got == list(_pipeline_expectations()[0])


class _Recorder:
    """The ``store`` callback: called from the pipeline's worker threads."""

    def __init__(self) -> None:
        self.calls: list = []
        self._lock = threading.Lock()

    def __call__(self, index, digest, payload, compressed) -> None:
        with self._lock:
            self.calls.append((index, digest, bytes(payload), compressed))


def _check_pipeline_run(pipeline, order: list) -> None:
    """One hash_compress_blocks call over the corpus blocks ``order``."""
    all_blocks = corpus.pipeline_blocks()
    want_digests, want_containers = _pipeline_expectations()
    blocks = [all_blocks[k] for k in order]
    record = _Recorder()
    digests, containers = pipeline.hash_compress_blocks(blocks, compress=True, store=record)
    assert len(digests) == len(containers) == len(blocks)
    for i, k in enumerate(order):
        assert digests[i] == want_digests[k], f"block {k} of {len(blocks[i])} bytes"
        assert containers[i] == want_containers[k], f"block {k} of {len(blocks[i])} bytes"
    assert sorted(c[0] for c in record.calls) == list(range(len(blocks)))
    for i, digest, payload, compressed in record.calls:
        k = order[i]
        assert digest == want_digests[k]
        if want_containers[k] is not None:
            assert compressed is True and payload == want_containers[k], f"block {k}"
        else:
            assert compressed is False and payload == blocks[i], f"block {k}"
    # the pipeline cut the windows where the test thinks it did: its two
    # slots still hold the last two
    windows = corpus.window_partition([len(b) for b in blocks], WINDOW)
    slots = pipeline._cached["state"][0]
    assert len(windows) >= 2
    for w in (len(windows) - 1, len(windows) - 2):
        assert slots[w % 2].meta[0] == windows[w]


def test_hash_compress_blocks_small_windows(monkeypatch):
    from modal_amd.ops import pipeline

    _feature()
    monkeypatch.setattr(pipeline, "WINDOW_BYTES", WINDOW)
    monkeypatch.setattr(pipeline, "GPU_MIN_BYTES", THRESHOLD)
    blocks = corpus.pipeline_blocks()
    sizes = [len(b) for b in blocks]
    windows = corpus.window_partition(sizes, WINDOW)
    assert len(windows) >= 6
    assert any(len(w) == 1 and sizes[w[0]] > WINDOW for w in windows)
    assert sum(sizes[w[-1]] % LEAF_SIZE != 0 for w in windows) >= 3

    _check_pipeline_run(pipeline, list(range(len(blocks))))
    # again over the slots' leftovers: other lengths, other payloads
    largest = max(range(len(blocks)), key=lambda k: sizes[k])
    _check_pipeline_run(pipeline, [k for k in reversed(range(len(blocks))) if k != largest])

    empty = hashlib.sha256(b"").hexdigest()
    assert pipeline.hash_compress_blocks([b"", b""]) == ([empty, empty], [None, None])
    digests, containers = pipeline.hash_compress_blocks(list(blocks), compress=False)
    assert digests == list(_pipeline_expectations()[0])
    assert containers == [None] * len(blocks)


# ---------------------------------------------------------------------------
# segment pack / unpack
# ---------------------------------------------------------------------------


def _check_scatter_gather(table: corpus.ScatterTable) -> None:
    """unpack_gpu scatters into canary: the whole destination equals the
    image, so every byte outside the segments is still canary. pack_gpu
    gathers the image back: the host concatenation."""
    import torch

    from modal_amd.ops.packing import pack_gpu, unpack_gpu

    corpus.check_gaps(table)
    packed = _to_device(table.packed)
    dst = torch.full((table.dst_size,), CANARY, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 16 == 0
    total = sum(table.lengths)
    unpack_gpu(packed[:total], dst, _i64(table.dst_offsets), _i64(table.lengths))
    image = table.image()
    got = dst.cpu().numpy()
    wrong = np.flatnonzero(got != image)
    assert wrong.size == 0, f"unpack: {wrong.size} bytes differ, the first at {wrong[:8].tolist()}"

    src = _to_device(image)
    gathered, offsets = pack_gpu(src, _i64(table.dst_offsets), _i64(table.lengths))
    assert offsets.tolist() == table.src_offsets()
    got = gathered.cpu().numpy()
    assert got.shape == (total,)
    wrong = np.flatnonzero(got != table.packed[:total])
    assert wrong.size == 0, f"pack: {wrong.size} bytes differ, the first at {wrong[:8].tolist()}"


@pytest.mark.parametrize("index", range(len(corpus.SMALL_LENGTHS) + 1))
def test_unpack_pack_alignment_matrix(index):
    _feature()
    tables = corpus.unpack_tables()
    corpus.check_unpack_coverage(tables)
    _check_scatter_gather(tables[index])


def test_pack_nothing():
    import torch

    from modal_amd.ops.packing import pack_gpu, unpack_gpu

    _feature()
    src = torch.full((256,), 7, dtype=torch.uint8, device="cuda")
    gathered, offsets = pack_gpu(src, _i64([]), _i64([]))
    assert gathered.numel() == 0 and offsets.numel() == 0
    gathered, offsets = pack_gpu(src, _i64([3, 100, 255]), _i64([0, 0, 0]))
    assert gathered.numel() == 0 and offsets.tolist() == [0, 0, 0]
    dst = torch.full((256,), CANARY, dtype=torch.uint8, device="cuda")
    unpack_gpu(gathered, dst, _i64([3, 100, 255]), _i64([0, 0, 0]))
    unpack_gpu(gathered, dst, _i64([]), _i64([]))
    assert bool((dst.cpu() == CANARY).all()) and bool((src.cpu() == 7).all())


def test_unpack_pack_1500_segments():
    """From 1024 segments on one block serves a segment and walks its tiles."""
    _feature()
    table = corpus.many_segments_table()
    assert corpus.blocks_per_segment(len(table.lengths), max(table.lengths)) == 1
    assert -(-max(table.lengths) // corpus.TILE) == 4
    _check_scatter_gather(table)


def test_unpack_pack_strided_tiles():
    """Fewer blocks than tiles: a block takes every third tile of five."""
    _feature()
    table = corpus.strided_table()
    tiles = -(-max(table.lengths) // corpus.TILE)
    bps = corpus.blocks_per_segment(len(table.lengths), max(table.lengths))
    assert 1 < bps < tiles and (bps, tiles) == (3, 5)
    _check_scatter_gather(table)


# ---------------------------------------------------------------------------
# offsets at and above 2**31 and 2**32
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def far_tensor():
    """One uninitialised device tensor of 2**32 + 2**20 bytes, in a list, for
    the tests below; freed after the last of them."""
    import torch

    _feature()
    free, _total = torch.cuda.mem_get_info()
    if free < 16 * 2**30:
        pytest.skip(f"{free / 2**30:.1f} GiB of device memory free, the far-offset tests want 16")
    holder = [torch.empty(corpus.FAR_BYTES, dtype=torch.uint8, device="cuda")]
    assert holder[0].data_ptr() % 16 == 0
    yield holder  # a list, so that emptying it here drops the last reference
    holder.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("ilp", ILP)
def test_sha256_far_offsets(far_tensor, ilp):
    import torch

    from modal_amd.ops.hashing import sha256_many_gpu

    far_tensor = far_tensor[0]
    regions = {edge: corpus.far_region(edge) for edge in corpus.FAR_EDGES}
    for edge, region in regions.items():
        far_tensor[edge - corpus.FAR_HALF : edge + corpus.FAR_HALF].copy_(torch.from_numpy(region))
    spans = corpus.far_messages()
    out = sha256_many_gpu(
        far_tensor, _i64(o for o, _n in spans), _i64(n for _o, n in spans), ilp=ilp
    )
    got = _digest_rows(out)
    for (off, n), g in zip(spans, got):
        edge = min(corpus.FAR_EDGES, key=lambda e: abs(e - off))
        at = off - (edge - corpus.FAR_HALF)
        want = hashlib.sha256(regions[edge][at : at + n].tobytes()).digest()
        assert g == want, f"{n} bytes at 2**{edge.bit_length() - 1} {off - edge:+d}"


@pytest.mark.parametrize("index", range(3))
def test_unpack_pack_far_offsets(far_tensor, index):
    import torch

    from modal_amd.ops.packing import pack_gpu, unpack_gpu

    far_tensor = far_tensor[0]
    table = corpus.far_destinations()[index]
    total = sum(n for _o, n in table)
    packed_host = np.random.default_rng(500 + index).integers(0, 256, total, dtype=np.uint8)
    packed = _to_device(packed_host)
    near = corpus.FAR_NEAR
    for edge in corpus.FAR_EDGES:
        far_tensor[edge - near : edge + near].fill_(CANARY)
    offsets, lengths = _i64(o for o, _n in table), _i64(n for _o, n in table)
    unpack_gpu(packed, far_tensor, offsets, lengths)
    for edge in corpus.FAR_EDGES:
        got = far_tensor[edge - near : edge + near].cpu().numpy()
        wrong = np.flatnonzero(got != corpus.far_image(table, packed_host, edge))
        assert wrong.size == 0, (
            f"around 2**{edge.bit_length() - 1}: {wrong.size} bytes differ, "
            f"the first at {(wrong[:8] - near).tolist()} from it"
        )
    gathered, _offsets = pack_gpu(far_tensor, offsets, lengths)
    assert bool(torch.equal(gathered.cpu(), torch.from_numpy(packed_host)))

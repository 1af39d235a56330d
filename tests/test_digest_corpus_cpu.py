"""Self-checks of tests/digest_corpus.py, all on the host. A pass of
tests/test_digest_gpu.py means what it says only while these hold: the
expectations come from hashlib, the host tree hash and the compressor's
model, and the corpus reaches the edges it claims to."""

from __future__ import annotations

import hashlib

import numpy as np
import pytest

import digest_corpus as corpus
from digest_corpus import THRESHOLD, WINDOW, expected_container, expected_digest, pipeline_blocks
from modal_amd.ops import compress
from modal_amd.ops.hashing import LEAF_SIZE, content_digest, tree_sha256_cpu


def test_edge_lengths():
    want = (0, 1, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 121, 127, 128, 129, 8191, 8192, 8193)
    assert LEAF_SIZE == 8192 and corpus.sha_edge_lengths() == want


def test_layout_yields_every_residue_for_every_edge_length():
    lengths, residues = corpus.edge_cases()
    lay = corpus.layout(lengths, residues, seed=1)
    got = {(n, o % 16) for n, o in zip(lay.lengths, lay.offsets)}
    assert got == {(n, r) for n in corpus.sha_edge_lengths() for r in range(16)}
    assert len(lay.offsets) == 19 * 16
    corpus.check_layout(lay, residues)
    # messages differ, so a digest stored in another's row is seen
    nonempty = [lay.message(i) for i in range(len(lay.offsets)) if lay.lengths[i]]
    assert len(set(nonempty)) == len(nonempty)


def test_layout_check_refuses_a_shared_packet():
    lay = corpus.Layout(np.zeros(64, dtype=np.uint8), [3, 9], [5, 4])
    with pytest.raises(AssertionError, match="share a packet"):
        corpus.check_layout(lay, [3, 9])
    with pytest.raises(AssertionError, match="no unused byte"):
        corpus.check_layout(corpus.Layout(lay.data, [3, 8], [5, 4]), [3, 8])


def test_pair_lists_put_every_edge_length_in_both_slots():
    lists = corpus.pair_position_lists()
    a, b = corpus.slots_of(lists)
    edges = set(corpus.sha_edge_lengths())
    assert edges <= a and edges <= b
    assert lists["empty_then_long"][:2] == [0, LEAF_SIZE + 1]
    assert lists["long_then_empty"][:2] == [LEAF_SIZE + 1, 0]


def test_grid_and_arbitrary_tables():
    lay = corpus.grid_messages(1025)
    assert lay.lengths == [i % 131 for i in range(1025)]
    assert len({lay.message(i) for i in range(1025) if lay.lengths[i] > 3}) == sum(
        n > 3 for n in lay.lengths
    )
    table = corpus.arbitrary_table()
    spans = list(zip(table.offsets, table.lengths))
    assert spans[1] == spans[6] and spans[1][1] > 0
    assert any(o1 < o0 for (o0, _), (o1, _) in zip(spans, spans[1:]))
    assert any(o0 < o1 < o0 + n0 for o0, n0 in spans for o1, _ in spans)  # an overlap
    digests = corpus.sha_digests(table)
    # distinct spans give distinct digests, but for the two empty ones
    assert digests[1] == digests[6] and len(set(digests)) == len(set(spans)) - 1


def test_far_tables():
    spans = corpus.far_messages()
    assert {n for _o, n in spans} == set(corpus.FAR_SHA_LENGTHS) and len(spans) == 20
    tables = corpus.far_destinations()
    assert len(tables) == 3
    packed = np.arange(sum(corpus.FAR_SEGMENT_LENGTHS), dtype=np.uint8)
    for table in tables:
        for edge in corpus.FAR_EDGES:
            img = corpus.far_image(table, packed, edge)
            inside = sum(n for o, n in table if abs(o - edge) < corpus.FAR_NEAR)
            assert int((img != corpus.CANARY).sum()) <= inside
    assert corpus.FAR_BYTES == 2**32 + 2**20


def test_multi_leaf_inputs_have_distinct_full_leaves():
    for size in corpus.tree_sizes():
        corpus.assert_distinct_full_leaves(corpus.tree_input(size))
    for block in pipeline_blocks():
        corpus.assert_distinct_full_leaves(block)
    L = LEAF_SIZE
    assert corpus.tree_sizes() == (
        1, L - 1, L, L + 1, 255 * L, 256 * L, 256 * L + 1, 257 * L + L - 1, 513 * L + 7
    )
    with pytest.raises(AssertionError, match="two full leaves are equal"):
        corpus.assert_distinct_full_leaves(bytes(range(256)) * 64)


def test_swapping_two_leaves_changes_the_tree_digest():
    """Why the leaves have to differ: the root commits to their order, which
    a test on periodic data cannot see."""
    data = corpus.tree_input(LEAF_SIZE * 256 + 1)
    swapped = corpus.swap_leaves(data, 1, 200)
    assert swapped != data and sorted(corpus.full_leaves(swapped)) == sorted(corpus.full_leaves(data))
    assert tree_sha256_cpu(swapped) != tree_sha256_cpu(data)
    periodic = bytes(range(256)) * (3 * LEAF_SIZE // 256)
    assert tree_sha256_cpu(corpus.swap_leaves(periodic, 0, 2)) == tree_sha256_cpu(periodic)


def test_pipeline_blocks_are_as_specified():
    blocks = pipeline_blocks()
    assert tuple(len(b) for b in blocks) == (
        0, 1, 4095, 4096, 4097, 8192, 16383, 16384, 16385, 40000, 65536, 65537, 100000, 0, 24576
    )
    assert blocks is pipeline_blocks()
    # no variant is used twice: the full segments of the compressible blocks differ
    segments = [
        b[o : o + 4096] for k, b in enumerate(blocks) if k % 3 for o in range(0, len(b) - 4095, 4096)
    ]
    assert len(segments) > 40 and len(set(segments)) == len(segments)


@pytest.fixture(params=["core", "python"])
def backend(request, monkeypatch):
    """The host codec over the C++ core, then over utils/lz4ref.py."""
    if request.param == "python":
        monkeypatch.setattr(compress, "_native_core", lambda: None)
    else:
        assert compress._native_core() is not None, "the native core is not built"
    return request.param


def test_expected_containers_decode_and_validate(backend):
    kept = 0
    for k, block in enumerate(pipeline_blocks()):
        blob = expected_container(block)
        if blob is None:
            continue
        kept += 1
        raw_len, comp_lens, _off = compress.validate_container(blob)
        assert raw_len == len(block) and len(comp_lens) == -(-len(block) // compress.SEG_SIZE)
        assert compress.decompress_buffer_cpu(blob) == block, f"block {k}"
    assert kept >= 4 and len(pipeline_blocks()) - kept >= 4
    assert expected_container(b"") is None


def test_expected_containers_equal_the_host_codecs(monkeypatch):
    """Byte for byte against ``compress_buffer_cpu`` over utils/lz4ref.py,
    whose parser is the kernel's (7-bit hash, skip through miss runs). The C++
    core behind the same function is another LZ4 parser (12-bit hash, no
    skip): its blocks are as valid and shorter, 1853 bytes against 2071 for
    the 4097-byte block, so there the containers are only required to be kept
    or dropped alike and to decode to the block."""
    core = compress._native_core()
    assert core is not None, "the native core is not built"
    for k, block in enumerate(pipeline_blocks()):
        native = compress.compress_buffer_cpu(block)
        assert (native is None) == (expected_container(block) is None), f"block {k}"
        if native is not None:
            compress.validate_container(native)
            assert compress.decompress_buffer_cpu(native) == block, f"block {k}"
    monkeypatch.setattr(compress, "_native_core", lambda: None)
    for k, block in enumerate(pipeline_blocks()):
        assert expected_container(block) == compress.compress_buffer_cpu(block), f"block {k}"


def test_expected_digests_and_what_the_blocks_exercise():
    blocks = pipeline_blocks()
    for block in blocks:
        assert expected_digest(block, THRESHOLD) == content_digest(block, THRESHOLD, gpu=False)
    plain = [b for b in blocks if len(b) < THRESHOLD]
    tree = [b for b in blocks if len(b) >= THRESHOLD]
    assert len(plain) >= 4 and len(tree) >= 4
    assert all(expected_digest(b, THRESHOLD) == hashlib.sha256(b).hexdigest() for b in plain)
    assert all(expected_digest(b, THRESHOLD) == tree_sha256_cpu(b).hex() for b in tree)
    assert any(len(b) % LEAF_SIZE for b in tree)
    assert any(len(b) > WINDOW for b in blocks)
    assert THRESHOLD == 2 * LEAF_SIZE and WINDOW == 64 * 1024


def test_window_partition_of_the_pipeline_blocks():
    sizes = [len(b) for b in pipeline_blocks()]
    windows = corpus.window_partition(sizes, WINDOW)
    assert [i for w in windows for i in w] == list(range(len(sizes)))
    assert len(windows) >= 6  # both slots reused more than once
    assert any(len(w) == 1 and sizes[w[0]] > WINDOW for w in windows)
    assert sum(sizes[w[-1]] % LEAF_SIZE != 0 for w in windows) >= 3  # close on odd sizes
    rest = sorted(sizes)[:-1][::-1]
    assert len(corpus.window_partition(rest, WINDOW)) >= 3


def test_unpack_tables_cover_every_residue_pair():
    tables = corpus.unpack_tables()
    corpus.check_unpack_coverage(tables)
    assert any(0 in t.lengths for t in tables)
    for t in tables:
        img = t.image()
        assert len(img) == t.dst_size
        covered = np.zeros(t.dst_size, dtype=bool)
        for d, n in zip(t.dst_offsets, t.lengths):
            assert not covered[d : d + n].any()
            covered[d : d + n] = True
        assert (img[~covered] == corpus.CANARY).all()
    # the tile-edge table spreads each segment over two blocks
    last = tables[-1]
    assert corpus.blocks_per_segment(len(last.lengths), max(last.lengths)) == 2


def test_many_segment_tables_take_the_branches_they_are_for():
    many = corpus.many_segments_table()
    assert len(many.lengths) == 1500 and sorted(many.lengths)[-2:] == [200_000, 200_000]
    assert corpus.blocks_per_segment(1500, 200_000) == 1 and -(-200_000 // corpus.TILE) == 4
    strided = corpus.strided_table()
    tiles = -(-max(strided.lengths) // corpus.TILE)
    bps = corpus.blocks_per_segment(len(strided.lengths), max(strided.lengths))
    assert len(strided.lengths) == 1023 and (bps, tiles) == (3, 5)
    for t in (many, strided):
        corpus.check_gaps(t)
        assert len({d % 16 for d in t.dst_offsets}) == 16

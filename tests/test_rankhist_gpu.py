"""ma_rank_hist (csrc/rankhist.hip) called directly: the histogram at element
size 1, 2 and 4 against the numpy twin's table and the rank tables against
``rankcodec.block_order``, every comparison exact."""

import functools

import numpy as np
import pytest

import byte_corpus as bc
from test_probe3_gpu import LENGTHS, ONE_VALUE

pytestmark = pytest.mark.gpu

GUARD = 0xA5
ROW = {1: 0, 2: 1, 4: 2}  # the table of probe_counts_cpu that es ranks by


def _rank_hist(parts: list, offsets: list, es: int) -> tuple:
    """(rc, counts, order, rank_of) of ONE ma_rank_hist launch over the parts,
    each at its offset in a buffer of guard bytes; the three tables come in as
    0, 1 and 2 so that a launch which writes nothing shows."""
    import torch

    from modal_amd.ops import load_lib

    host = np.full(-(-(offsets[-1] + len(parts[-1])) // 16) * 16 + 32, GUARD, dtype=np.uint8)
    for off, data in zip(offsets, parts):
        host[off : off + len(data)] = np.frombuffer(data, dtype=np.uint8)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    off_d = torch.tensor(offsets, dtype=torch.int64).cuda()
    len_d = torch.tensor([len(p) for p in parts], dtype=torch.int64).cuda()
    counts = torch.zeros(len(parts), 256, dtype=torch.int32, device="cuda")
    order = torch.ones(len(parts), 256, dtype=torch.uint8, device="cuda")
    rank_of = torch.full((len(parts), 256), 2, dtype=torch.uint8, device="cuda")
    rc = load_lib(required=True).ma_rank_hist(
        buf.data_ptr(), off_d.data_ptr(), len_d.data_ptr(), es, counts.data_ptr(),
        order.data_ptr(), rank_of.data_ptr(), len(parts), torch.cuda.current_stream().cuda_stream,
    )
    torch.cuda.synchronize()
    return rc, counts.cpu().numpy(), order.cpu().numpy(), rank_of.cpu().numpy()


def _differing(parts: list, offsets: list, es: int) -> list:
    """The indices whose counts, order or rank_of are not the numpy model's."""
    from modal_amd.ops import probe, rankcodec

    rc, counts, order, rank_of = _rank_hist(parts, offsets, es)
    assert rc == 0
    bad = []
    for k, data in enumerate(parts):
        want_order = rankcodec.block_order(np.frombuffer(data, dtype=np.uint8), es)
        want_rank = np.empty(256, dtype=np.uint8)
        want_rank[want_order] = np.arange(256, dtype=np.uint8)
        if not (
            np.array_equal(counts[k], probe.probe_counts_cpu(data)[ROW[es]])
            and np.array_equal(order[k], want_order)
            and np.array_equal(rank_of[k], want_rank)
        ):
            bad.append(k)
    return bad


@functools.lru_cache(maxsize=None)
def _every_alignment() -> tuple:
    """Every length at source residues 0..15 mod 16, 16 to 31 guard bytes
    between spans. Built once; nobody changes it."""
    e4m3 = bc.fp8(max(LENGTHS) + 16, "float8_e4m3fn", 94)
    assert GUARD not in b"\x38" and len(set(e4m3)) > 64
    parts, offsets, end = [], [], 0
    for n in LENGTHS:
        for r in range(16):
            offsets.append(-(-end // 16) * 16 + 16 + r)
            parts.append(b"\x38" * n if n in ONE_VALUE else e4m3[r : r + n])
            end = offsets[-1] + n
    return parts, offsets


@pytest.mark.parametrize("es", (1, 2, 4))
def test_tables_at_every_alignment(es):
    """A byte from outside a span, one of its own left out or one of another
    offset class changes a count. Below es the model has no whole element:
    every count is zero and the order is 0..255."""
    parts, offsets = _every_alignment()
    bad = _differing(parts, offsets, es)
    assert not bad, [(len(parts[k]), offsets[k] % 16) for k in bad]  # (length, residue)


def test_more_spans_than_one_grid():
    """65536 spans of 8 bytes, one past MAX_GRID_Y, at residues 3 and 11."""
    data = bc.fp8(8 * 65536, "float8_e5m2", 95)
    bad = _differing([data[8 * k : 8 * k + 8] for k in range(65536)], list(range(3, 8 * 65536, 8)), 2)
    assert not bad, bad[-3:]


@pytest.mark.parametrize("es", (0, 3))
def test_other_element_sizes_launch_nothing(es):
    rc, counts, order, rank_of = _rank_hist([bc.fp8(4097, "float8_e4m3fn", 96)], [16], es)
    assert rc != 0
    assert not counts.any() and (order == 1).all() and (rank_of == 2).all()

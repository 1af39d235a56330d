"""The three-way element-size probe: which rank-plane format, at which element
size, pays for bytes of no known element type.

MAFB10 (ops/bytecodec.py) codes every byte of a block, MAFP10 (ops/fpcodec.py)
the top byte of every 2- or 4-byte element. A caller that has no element type
(a tracked raw allocation, a uint8 tensor of packed fp8) asks the bytes: the
probe gives a block's histogram at element sizes 1, 2 and 4 in one pass
(``ma_rank_probe`` in csrc/rankhist.hip, ``probe_counts_cpu`` its numpy
twin) and ``choose_elem_size`` picks the size whose container comes out
smallest, or none. ``devcodec`` does this under ``fpcodec.AUTO`` and hands the
winning histogram on to the encoder, which then runs no histogram launch.

The two-way probe of ops/fpcodec.py (sizes 2 and 4) is still there for its
callers; on every input where its answer is pinned this rule gives the same.
"""

from __future__ import annotations

from typing import Any, Sequence

import numpy as np

from . import container
from .container import worth_keeping
from .fpcodec import _estimate

#: the rows of a probe's table, and the order ties are settled in
ELEM_SIZES = (1, 2, 4)
_TIE_ORDER = (2, 4, 1)


def probe_counts_cpu(data: Any) -> tuple[Any, Any, Any]:
    """(counts1, counts2, counts4): the histograms ``rankcodec.block_order``
    sorts at ``es`` 1, 2 and 4, 256 int64 counts each. The numpy twin of
    ``ma_rank_probe``."""
    data = np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8)
    n = len(data)
    return (
        np.bincount(data, minlength=256),
        np.bincount(data[1 : n - n % 2 : 2], minlength=256),
        np.bincount(data[3 : n - n % 4 : 4], minlength=256),
    )


def _choose(
    counts1: Any, counts2: Any, counts4: Any, raw_len: Any, estimate: Any = _estimate
) -> tuple[Any, Any]:
    tables = {1: counts1, 2: counts2, 4: counts4}
    ests = np.stack([estimate(tables[es], raw_len, es) for es in _TIE_ORDER])
    pick = ests.argmin(axis=0)  # the first minimum: 2, then 4, then 1
    est = ests.min(axis=0)
    es = np.asarray(_TIE_ORDER)[pick]
    return np.where(worth_keeping(est, np.asarray(raw_len, dtype=np.int64)), es, 0), est


def choose_elem_size(
    counts1: Any, counts2: Any, counts4: Any, raw_len: int, estimate: Any = _estimate
) -> tuple[int, int]:
    """(es, estimate): the element size, 1, 2 or 4, at which a rank-plane
    container of a block of ``raw_len`` bytes with these three histograms comes
    out smallest, and the payload estimated for it; ``es`` is 0 when even that
    misses ``container.worth_keeping``. The estimate is
    ``fpcodec.choose_elem_size``'s, taken at es 1 too: there ``n = raw_len``,
    no low bytes and no bytes outside a whole element. Ties go to 2, then 4,
    then 1, so element size 1 wins only where it is strictly smaller. Exact
    integer arithmetic, so the same tables give the same answer anywhere.

    The estimate bounds MAFB10's payload by the argument given there for
    MAFP10's: a full segment's ``m = 4096`` is a multiple of 8 as 2048 and
    1024 are, and MAFB10's encoder picks its widths by the same rule. At es 1
    every length is a whole number of elements, so the short last segment is
    never stored raw for being odd.

    ``estimate(counts, raw_len, es)`` is the fixed-width rule above unless the
    caller codes ranks another way and gives its own
    (``ricecodec.estimate``); the ties and the 5 % rule are the same."""
    es, est = _choose(counts1, counts2, counts4, raw_len, estimate)
    return int(es), int(est)


def probe_spans_gpu(
    lib: Any, base: int, spans: Sequence[tuple[int, int]], estimate: Any = _estimate
) -> tuple[list, Any]:
    """``choose_elem_size`` for the device bytes ``(base + offset, raw_len)``
    of every span: (the element size per span, 0 where no rank-plane container
    would pay; the probe's tables, a ``len(spans) x 3 x 256`` int32 device
    tensor whose ``[:, 0]``, ``[:, 1]`` and ``[:, 2]`` are the histograms at es
    1, 2 and 4, each what ``Format.compress_spans_gpu`` takes as ``counts``).
    One probe launch and one D2H of the tables (3 KiB per span) on the current
    stream; the rule itself runs on the host, on the same tables as the numpy
    path."""
    import torch

    counts = torch.zeros(len(spans), 3, 256, dtype=torch.int32, device="cuda")
    if not spans:
        return [], counts
    src_off_d = container.to_dev(np.array([off for off, _ln in spans], dtype=np.int64))
    raw_d = container.to_dev(np.array([ln for _off, ln in spans], dtype=np.int64))
    container.check(
        lib.ma_rank_probe(
            base, src_off_d.data_ptr(), raw_d.data_ptr(), counts.data_ptr(), len(spans),
            torch.cuda.current_stream().cuda_stream,
        ),
        "rank probe kernel",
    )
    host = counts.cpu().numpy().view(np.uint32)  # syncs: the tables may be freed
    es, _est = _choose(
        host[:, 0], host[:, 1], host[:, 2], [ln for _off, ln in spans], estimate
    )
    return es.tolist(), counts

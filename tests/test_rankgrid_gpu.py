"""The rank codecs' launches past 65,535 grid rows (``launch_chunked`` of
csrc/malz_common.h): one ``compress_spans_gpu`` call of 65,535 + 70 spans goes
through the chunk loop of the histogram, the rank encode, the plan and the
rank assemble. Span i holds content i % 7 and 65,535 % 7 is 1, so a kernel
that restarts a table index at the chunk boundary pairs a span with another
span's bytes, rank table or order table. Compared exactly with the numpy
model, computed once per content."""

from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPAN = 512
N_SPANS = 65535 + 70
POOL = 7


def _pool() -> list:
    """Seven compressible contents with different dominant bytes and order tables."""
    rng = np.random.default_rng(11)
    out = []
    for p in range(POOL):
        data = np.full(SPAN, 16 * p + 3, dtype=np.uint8)
        where = rng.permutation(SPAN)[: 40 + 4 * p]
        data[where] = 16 * p + 4 + rng.integers(0, 3 + p, len(where))
        out.append(data)
    return out


@pytest.mark.parametrize("codec_name", ["ricecodec", "bytecodec"])
def test_spans_past_one_grid_of_rows_keep_their_own_tables(codec_name):
    import importlib

    import torch

    from modal_amd.ops import load_lib

    codec = importlib.import_module(f"modal_amd.ops.{codec_name}")
    lib = load_lib(required=True)
    if torch.cuda.mem_get_info()[0] < 2 << 30:
        pytest.skip("less than 2 GiB of device memory free")
    pool = _pool()
    want = [codec.FORMAT.compress_buffer_cpu(data.tobytes(), 1) for data in pool]
    assert all(z is not None for z in want)
    assert len({bytes(codec.validate_container(z).order) for z in want}) == POOL

    src = torch.from_numpy(np.stack(pool)[np.arange(N_SPANS) % POOL].reshape(-1)).cuda()
    spans = [(i * SPAN, SPAN) for i in range(N_SPANS)]
    ws = codec.Workspace.for_lengths([SPAN] * N_SPANS, codec.HEADER_FIXED)
    got = codec.FORMAT.compress_spans_gpu(lib, src.data_ptr(), spans, 1, ws)
    assert len(got) == N_SPANS
    wrong = [i for i, z in enumerate(got) if z is None or bytes(z) != want[i % POOL]]
    assert not wrong, f"{len(wrong)} spans differ from the model, the first at {wrong[:5]}"

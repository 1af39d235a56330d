"""The slot alignment an encoder never meets through a Workspace: the
low-byte gather of csrc/rank_common.h (fpz and ricez encoders) stores bytes,
not dwords, into a slot that is not 4-aligned, and the bytez encoder sends its
codes through the staging buffer then. Each encode entry is called directly,
once on an aligned stride buffer and once on the same buffer one byte on, and
must write the same segments."""

import functools

import numpy as np
import pytest

import byte_corpus as bc
import fp_corpus as fc

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 64  # guard bytes on either side of the stride buffer
SEG = 4096

# entry, element size, length of the short third segment
CASES = [
    ("ma_fpz_encode", 2, 4094),
    ("ma_fpz_encode", 4, 4092),
    ("ma_ricez_encode", 2, 4094),
    ("ma_ricez_encode", 4, 4092),
    ("ma_bytez_encode", 1, 4093),
]


@functools.lru_cache(maxsize=None)
def _span(es: int, last: int) -> bytes:
    """Two full segments and one of ``last`` bytes of N(0,1) values as fp8,
    bf16 or fp32. Built once; nobody changes it."""
    n = 2 * SEG + last
    if es == 1:
        return bc.fp8(n, "float8_e4m3fn", 7)
    return fc.bf16_gauss(n, seed=7) if es == 2 else fc.fp32_gauss(n, seed=7)


def _encode(entry: str, es: int, data: bytes, shift: int) -> tuple:
    """(comp_lens, the three slots, guards intact) of one launch whose stride
    buffer begins ``shift`` bytes past a 16-byte boundary."""
    import torch

    from modal_amd.ops import load_lib
    from modal_amd.ops.container import OUT_STRIDE

    lib = load_lib(required=True)
    stream = torch.cuda.current_stream().cuda_stream
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    off_d = torch.zeros(1, dtype=torch.int64, device="cuda")
    len_d = torch.tensor([len(data)], dtype=torch.int64).cuda()
    first_d = torch.zeros(1, dtype=torch.int32, device="cuda")
    counts = torch.zeros(256, dtype=torch.int32, device="cuda")
    order = torch.zeros(256, dtype=torch.uint8, device="cuda")
    rank_of = torch.zeros(256, dtype=torch.uint8, device="cuda")
    assert 0 == lib.ma_rank_hist(
        src.data_ptr(), off_d.data_ptr(), len_d.data_ptr(), es, counts.data_ptr(),
        order.data_ptr(), rank_of.data_ptr(), 1, stream,
    )
    whole = torch.full((PAD + shift + 3 * OUT_STRIDE + PAD,), GUARD, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    comp_lens = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    es_arg = () if entry == "ma_bytez_encode" else (es,)
    rc = getattr(lib, entry)(
        src.data_ptr(), off_d.data_ptr(), len_d.data_ptr(), first_d.data_ptr(),
        rank_of.data_ptr(), *es_arg, whole.data_ptr() + PAD + shift, OUT_STRIDE,
        comp_lens.data_ptr(), 1, 3, stream,
    )
    torch.cuda.synchronize()
    assert rc == 0
    out = whole.cpu().numpy()
    body = out[PAD + shift : PAD + shift + 3 * OUT_STRIDE]
    guards = bool((out[: PAD + shift] == GUARD).all() and (out[PAD + shift + 3 * OUT_STRIDE :] == GUARD).all())
    return comp_lens.cpu().numpy(), body.reshape(3, OUT_STRIDE), guards


@pytest.mark.parametrize("entry,es,last", CASES, ids=[f"{c[0][3:-7]}-es{c[1]}" for c in CASES])
def test_unaligned_slots_hold_the_same_segments(entry, es, last):
    data = _span(es, last)
    lens_a, slots_a, guards_a = _encode(entry, es, data, 0)
    lens_u, slots_u, guards_u = _encode(entry, es, data, 1)
    assert guards_a and guards_u, "an encoder wrote outside its stride buffer"
    for lens in (lens_a, lens_u):
        assert (lens >= 0).all() and (lens < SEG).all(), lens  # every one written
        assert lens.any(), "every segment declined: nothing was compared"
    assert lens_a.tolist() == lens_u.tolist()
    for s, n in enumerate(lens_a.tolist()):
        assert slots_a[s, :n].tobytes() == slots_u[s, :n].tobytes(), f"segment {s}"

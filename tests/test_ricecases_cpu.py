"""The MARC10 numpy model (ops/ricecodec.py) against the bit-serial reference
of tests/rice_cases.py on inputs that reach every path of the format: what
the named cases reach, counted from the model's own containers; model, reader
and writer on every case; and the containers only the writer makes, a ``k``
no encoder picks and a code for a rank above 255. Every comparison is exact."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import rice_cases as rk
from modal_amd.ops import ricecodec

NAMES = sorted(rk.CASES)


@functools.lru_cache(maxsize=None)
def _model(name: str):
    raw, es = rk.CASES[name]
    return ricecodec.compress_buffer_cpu(raw, es)


@functools.lru_cache(maxsize=None)
def _reached(name: str) -> list:
    """Per segment of the model's container: None where it is raw, else
    (k, its codes, its end table)."""
    _raw_len, es, _order, segments = rk.read_container(_model(name))
    out: list = []
    for coded, body, L in segments:
        if not coded:
            out.append(None)
            continue
        lo = (L // es) * (es - 1)
        codes = rk.read_segment(body, L, es)
        assert not isinstance(codes, str), (name, codes)
        out.append((body[lo], codes, np.frombuffer(body, dtype="<u2", count=16, offset=lo + 1).tolist()))
    return out


def _escapes(name: str) -> list:
    return [sum(isinstance(c, rk.Esc) for c in seg[1]) if seg else 0 for seg in _reached(name)]


# ---------------------------------------------------------------------------
# what the cases reach
# ---------------------------------------------------------------------------


def test_every_case_has_a_container():
    assert all(_model(name) is not None for name in NAMES)


def test_cases_reach_every_k_the_model_can_pick():
    reached = {(rk.CASES[name][1], seg[0]) for name in NAMES for seg in _reached(name) if seg}
    print("reached (es, k):", sorted(reached))
    assert reached == {(es, k) for es in rk.ELEM_SIZES for k in range(7)}


def test_cases_have_dense_escapes_and_runs_of_them():
    for es in rk.ELEM_SIZES:
        counts = {name: _escapes(name) for name in NAMES if name.endswith(f"es{es}") and any(_escapes(name))}
        print(f"escapes per segment, es {es}:", counts)
        assert max(_escapes(f"escapes_es{es}")) >= rk.MIN_ESCAPES[es]
        # forty consecutive elements of sub-stream 0, all escapes
        k, codes, _end = _reached(f"escape_run_es{es}")[0]
        assert all(isinstance(c, rk.Esc) for c in codes[5:45]) and 45 < -(-len(codes) // 16)


@pytest.mark.parametrize("es", rk.ELEM_SIZES)
def test_smallest_segments_that_code(es):
    def tail_codes(m: int) -> bool:
        raw = bytes([0x3C]) * (rk.SEG + m * es)
        return ricecodec.validate_container(ricecodec.compress_buffer_cpu(raw, es)).seg_lens[1] != 0

    smallest = next(m for m in range(1, 200) if tail_codes(m))
    print(f"smallest coding m at es {es}: {smallest}")
    assert smallest == rk.MIN_M[es] and rk.TAILS[es][:2] == (smallest, smallest + 1)
    empty = 0
    for m in rk.TAILS[es]:
        full, tail = _reached(f"tail_{m}_es{es}")
        assert full and tail and len(tail[1]) == m, m  # coded, not stored raw
        empty += sum(a == b for a, b in zip(tail[2], tail[2][1:]))
    # 49 elements: twelve sub-streams of four, one of one whose other three
    # quarter-lanes have no run, three of none
    assert _reached(f"tail_49_es{es}")[1][2][12:] == [13, 13, 13, 13] and empty >= 3


@pytest.mark.parametrize("es", rk.ELEM_SIZES)
def test_mixed_block_has_three_k_and_a_raw_segment_between(es):
    segs = _reached(f"mixed_es{es}")
    ks = [seg[0] if seg else None for seg in segs]
    print(f"mixed block, es {es}: k per segment {ks}")
    assert len({k for k in ks if k is not None}) >= 3
    assert any(k is None and ks[i - 1] is not None and ks[i + 1] is not None
               for i, k in enumerate(ks) if 0 < i < len(ks) - 1)


# ---------------------------------------------------------------------------
# model, reader and writer on every case
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("name", NAMES)
def test_model_reader_and_writer_agree(name):
    raw, es = rk.CASES[name]
    z = _model(name)
    assert ricecodec.validate_container(z, len(raw)).es == es
    assert ricecodec.decompress_buffer_cpu(z) == raw
    assert rk.decode_container(z) == raw  # the reader, every coded segment
    # the writer, from the format's order rule and the k the model chose
    ks = [seg[0] if seg else None for seg in _reached(name)]
    assert list(rk.read_container(z)[2]) == rk.order_of(raw, es)
    assert rk.forced(raw, es, ks) == z


# ---------------------------------------------------------------------------
# containers no encoder writes
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("name,ks", sorted(rk.FORCED.items()))
def test_model_decodes_a_k_the_encoder_would_not_pick(name, ks):
    raw, es = rk.CASES[name]
    z = rk.forced_case(name)
    assert z != _model(name) and [seg[0] if seg else None for seg in _reached(name)] != ks
    ricecodec.validate_container(z, len(raw))
    assert ricecodec.decompress_buffer_cpu(z) == raw
    assert rk.decode_container(z) == raw


@pytest.mark.parametrize("es", rk.ELEM_SIZES)
def test_no_segment_at_k_7_passes_the_validator(es):
    """Every code at k = 7 is at least a byte, so the smallest such segment
    (every rank below 128) has seg_len = L + 33 and no reader walks it."""
    raw = bytes([0x3C]) * rk.SEG
    z = rk.forced(raw, es, [7])
    assert rk.read_container(z)[3][0][1][rk.SEG - rk.SEG // es] == 7
    assert len(z) == ricecodec.HEADER_FIXED + 4 + rk.SEG + 33
    assert rk.decode_container(z) == raw  # the layout itself holds at k = 7
    with pytest.raises(ValueError, match="seg_len out of range"):
        ricecodec.validate_container(z)


@pytest.mark.parametrize("k", [5, 7])
def test_readers_reject_a_rank_above_255(k):
    good, bad, raw = rk.bad_rank(k)
    assert ricecodec.decompress_buffer_cpu(good) == raw and rk.decode_container(good) == raw
    ricecodec.validate_container(bad, len(raw))  # the header fields are sound
    assert rk.decode_container(bad) == (1, "rank")
    with pytest.raises(ValueError, match="corrupt at segment 1"):
        ricecodec.decompress_buffer_cpu(bad)
    # segments 0 and 2 are the good container's: nothing else is touched
    assert [seg[1] for seg in rk.read_container(bad)[3]][::2] == [seg[1] for seg in rk.read_container(good)[3]][::2]

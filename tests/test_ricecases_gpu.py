"""The MARC10 kernels (csrc/ricez.hip) on the inputs of tests/rice_cases.py:
every Rice parameter, dense escapes and runs of them, the smallest segments
that code, a block of mixed segments, and the containers only the bit-serial
writer makes. The encoder is held to the numpy model byte for byte, the
decoder to the raw bytes and to the status word. Every comparison is exact."""

from __future__ import annotations

import functools

import pytest

import rice_cases as rk
import rice_corpus as rc
from test_ricecodec_gpu import CANARY, _decode_run, _feature, _upload

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _model(name: str):
    from modal_amd.ops import ricecodec

    raw, es = rk.CASES[name]
    return ricecodec.compress_buffer_cpu(raw, es)


@pytest.mark.parametrize("residue", [0, 5])
@pytest.mark.parametrize("es", rk.ELEM_SIZES)
def test_encoder_matches_the_model_on_every_case(es, residue):
    ricecodec, lib = _feature()
    names = [name for name in sorted(rk.CASES) if rk.CASES[name][1] == es]
    buf, spans = _upload([rk.CASES[name][0] for name in names], residue)
    ws = ricecodec.Workspace.for_lengths([ln for _off, ln in spans], ricecodec.HEADER_FIXED)
    got = ricecodec.compress_spans_gpu(lib, buf.data_ptr(), spans, es, ws)
    for name, z in zip(names, got):
        assert (z is None) == (_model(name) is None), name
        if z is not None:
            assert bytes(z) == _model(name), f"{name}: container differs from the model"


@pytest.mark.parametrize("residue", [0, 5])
def test_decoder_writes_every_case_and_forced_k_in_one_launch(residue):
    ricecodec, _lib = _feature()
    names = sorted(rk.CASES)
    blobs = [_model(name) for name in names] + [rk.forced_case(name) for name in sorted(rk.FORCED)]
    raw = b"".join(rk.CASES[name][0] for name in names + sorted(rk.FORCED))
    status, out, lo = _decode_run(blobs, [ricecodec.validate_container(z) for z in blobs], residue)
    assert status == 0
    assert out[lo : lo + len(raw)].tobytes() == raw
    assert (out[:lo] == CANARY).all() and (out[lo + len(raw) :] == CANARY).all()


@pytest.mark.parametrize("k", [5, 7])
def test_decoder_rejects_a_rank_above_255_and_leaves_the_segment_alone(k):
    ricecodec, _lib = _feature()
    good, bad, raw = rk.bad_rank(k)
    later = bytearray(good)
    later[rc.hi_offsets(good)[0]] = 9  # a later corrupt segment must not win
    headers = [ricecodec.validate_container(z) for z in (good, bad, good)]
    status, out, lo = _decode_run([good, bad, bytes(later)], headers, 0)
    assert status == 1 + 3 + 1
    first = lo + len(raw) + rk.SEG
    assert (out[first : first + rk.SEG] == CANARY).all()
    assert out[lo:first].tobytes() == raw + raw[: rk.SEG]
    assert (out[:lo] == CANARY).all() and (out[lo + 3 * len(raw) :] == CANARY).all()

"""Property tests of the native chunk_done parser against msgpack."""

from __future__ import annotations

import msgpack
import pytest

from modal_amd import _core as core

# only these property tests need hypothesis
hypothesis = pytest.importorskip("hypothesis")
from hypothesis import given, settings, strategies as st  # noqa: E402

CLEAN_KEYS = ("t", "token", "call_id", "chunk_id", "function_id", "count", "data", "cis")

_scalars = st.one_of(
    st.none(), st.booleans(), st.integers(-(2**63), 2**64 - 1), st.floats(allow_nan=False),
    st.text(max_size=40), st.binary(max_size=300),
)
_values = st.recursive(
    _scalars,
    lambda inner: st.one_of(st.lists(inner, max_size=4), st.dictionaries(st.text(max_size=6), inner, max_size=4)),
    max_leaves=8,
)
_ids = st.one_of(st.text(alphabet="abcdefg:-0123456789", max_size=40), st.text(max_size=8))

_done_shaped = st.fixed_dictionaries(
    {
        "t": st.sampled_from(["chunk_done", "chunk_done", "chunk_done", "outputs", ""]),
        "token": _ids, "call_id": _ids, "chunk_id": _ids, "function_id": _ids,
        "count": st.one_of(st.integers(0, 2**40), st.integers(-5, 5), st.floats(allow_nan=False)),
        "data": st.one_of(st.binary(max_size=70000), st.none(), st.text(max_size=5)),
        "cis": st.one_of(st.none(), st.lists(st.integers(0, 10**6), max_size=20), st.lists(_scalars, max_size=3)),
    },
    optional={"failed": st.booleans(), "exceptions": _values, "items": _values, "zz": _values},
).flatmap(
    lambda d: st.permutations(list(d.items())).map(dict)
).flatmap(
    lambda d: st.sets(st.sampled_from(sorted(d)), max_size=2).map(
        lambda drop: {k: v for k, v in d.items() if k not in drop or len(drop) == 2 and k == "zz"}
    )
)


def check_parse(body: bytes) -> None:
    parsed = core.parse_chunk_done(body)
    if parsed is None:
        return  # raw: msgpack.unpackb's business
    msg = msgpack.unpackb(body, raw=False, strict_map_key=False)
    assert set(msg) == set(CLEAN_KEYS) and msg["t"] == "chunk_done"
    assert parsed == tuple(msg[k] for k in CLEAN_KEYS[1:])
    assert [type(v) for v in parsed] == [type(msg[k]) for k in CLEAN_KEYS[1:]]


@settings(max_examples=300, deadline=None)
@given(_done_shaped)
def test_parser_matches_msgpack_on_chunk_done_shapes(msg):
    check_parse(msgpack.packb(msg, use_bin_type=True))


@settings(max_examples=200, deadline=None)
@given(st.dictionaries(st.one_of(st.text(max_size=8), st.integers(0, 9)), _values, max_size=10))
def test_parser_matches_msgpack_on_arbitrary_maps(msg):
    check_parse(msgpack.packb(msg, use_bin_type=True))


@settings(max_examples=200, deadline=None)
@given(_done_shaped, st.data())
def test_parser_truncated_input_is_raw(msg, data):
    body = msgpack.packb(msg, use_bin_type=True)
    cut = data.draw(st.integers(0, len(body) - 1))
    # the slice is an exact-size buffer: a read past its end is out of bounds
    assert core.parse_chunk_done(bytes(body[:cut])) is None
    assert core.parse_chunk_done(body + b"\x00") is None  # trailing bytes



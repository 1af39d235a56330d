"""The three-way element-size probe without a GPU (ops/probe.py): the rule on
data of known kind, its estimate against MAFB10's payload, AUTO on the host."""

import functools

import numpy as np
import pytest

import byte_corpus as bc
import fp_corpus as fc

MiB = fc.MiB


@functools.lru_cache(maxsize=None)
def inputs() -> dict:
    """name -> (1 MiB of bytes, the element size the rule must choose)."""
    gauss = fc.corpus()["bf16_n01_1m"][0]
    counters = np.random.default_rng(2024).integers(0, 50000, MiB // 4, dtype=np.int32)
    return {
        "e4m3": (bc.fp8(MiB, "float8_e4m3fn", 1), 1),
        "e5m2": (bc.fp8(MiB, "float8_e5m2", 2), 1),
        "int32_counters": (counters.tobytes(), 1),
        "bf16_behind_an_odd_byte": ((b"\x07" + gauss)[:MiB], 1),
        "bf16": (gauss, 2),
        "fp16": (fc.fp16_gauss(MiB, seed=4), 2),
        "fp32": (fc.fp32_gauss(MiB, seed=3), 4),
        "random": (fc.random_bytes(MiB, seed=5), 0),
    }


def five_parts() -> bytes:
    """LZ4's block, a bf16 one, one nothing takes, an e4m3 one (1 MiB each)
    and 64 KiB of e5m2, too short for LZ4 and for MAFP10."""
    unit = np.random.default_rng(11).integers(0, 256, 1024, dtype=np.uint8).tobytes()
    parts = [unit * 1024, inputs()["bf16"][0], fc.random_bytes(MiB, seed=77), inputs()["e4m3"][0]]
    return b"".join(parts) + bc.fp8(64 * 1024, "float8_e5m2", 9)


@pytest.mark.parametrize("name", sorted(inputs()))
def test_rule_chooses_the_element_size(name):
    from modal_amd.ops import fpcodec, probe

    data, want = inputs()[name]
    tables = probe.probe_counts_cpu(data)
    es, est = probe.choose_elem_size(*tables, MiB)
    each = sorted(int(fpcodec._estimate(c, MiB, e)) for c, e in zip(tables, probe.ELEM_SIZES))
    print(f"{name}: es {es}, estimates {[round(e / MiB, 4) for e in each]} of raw")
    assert len(data) == MiB and est == each[0]
    assert abs(est / MiB - 0.95) >= 0.01, "a borderline input proves nothing"
    assert each[1] - est >= 0.01 * MiB, "the runner-up is too close to tell"
    assert es == want


@pytest.mark.parametrize("cut", [0, 1, 3, 4097])
def test_estimate_bounds_the_byte_codecs_payload(cut):
    from modal_amd.ops import bytecodec, fpcodec, probe

    data = inputs()["e4m3"][0][: MiB - cut]
    z = bytecodec.compress_buffer_cpu(data)
    payload = len(z) - bytecodec.validate_container(z).payload_off
    est = int(fpcodec._estimate(probe.probe_counts_cpu(data)[0], len(data), 1))
    print(f"len {len(data)}: payload {payload}, estimate {est}")
    assert payload <= est + (0 if len(data) % 4 == 0 else fpcodec.SEG_SIZE)


def test_encode_host_auto_finds_byte_blocks_too():
    from modal_amd.ops import bytecodec, compress, devcodec, fpcodec

    data = five_parts()
    part = [data[k * MiB : (k + 1) * MiB] for k in range(5)]
    auto = devcodec.encode_host(data, block_size=MiB, elem_size=fpcodec.AUTO)
    assert [(bytes(b.payload), b.compressed) for b in auto] == [
        (compress.compress_buffer(part[0]), True), (fpcodec.compress_buffer_cpu(part[1], 2), True),
        (part[2], False), (bytecodec.compress_buffer_cpu(part[3]), True),
        (bytecodec.compress_buffer_cpu(part[4]), True),
    ]
    plain = devcodec.encode_host(data, block_size=MiB, elem_size=0)
    assert [b.digest for b in auto] == [b.digest for b in plain]
    assert devcodec.decode_host([tuple(b) for b in auto]) == data

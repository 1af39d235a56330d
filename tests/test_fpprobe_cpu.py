"""The element-size probe of the float-plane codec without a GPU
(ops/fpcodec.py): the rule on data of known kind, its estimate as a bound on
the numpy codec's payload, the numpy twin of the probe kernel against
``block_order``'s histograms, and ``fpcodec.AUTO`` through ``encode_host`` and
``capture_manifest(float_codec="auto")``."""

from __future__ import annotations

import functools
import pickle

import numpy as np
import pytest

import fp_corpus as fc

MiB = fc.MiB
SEG = fc.SEG


@functools.lru_cache(maxsize=None)
def inputs() -> dict:
    """name -> (1 MiB of bytes, the element size the rule must choose)."""
    rng = np.random.default_rng(2024)
    gauss = fc.corpus()["bf16_n01_1m"][0]
    return {
        "bf16_n01": (gauss, 2),
        "bf16_n002": (fc.corpus()["bf16_n002_1m"][0], 2),
        "fp16_n01": (fc.fp16_gauss(MiB, seed=4), 2),
        "fp32_n01": (fc.fp32_gauss(MiB, seed=3), 4),
        "fp32_u01": (rng.random(MiB // 4, dtype=np.float32).tobytes(), 4),
        "int32_counters": (rng.integers(0, 50000, MiB // 4, dtype=np.int32).tobytes(), 4),
        "random": (fc.random_bytes(MiB, seed=5), 0),
        "bf16_behind_an_odd_byte": ((b"\x07" + gauss)[:MiB], 0),
    }


def _pattern(n: int, seed: int = 11) -> bytes:
    unit = np.random.default_rng(seed).integers(0, 256, 1024, dtype=np.uint8)
    return np.tile(unit, -(-n // 1024))[:n].tobytes()


def four_parts() -> bytes:
    """LZ4's block, a bf16 one, one nothing takes, an fp32 one: 1 MiB each."""
    return (
        _pattern(MiB) + inputs()["bf16_n01"][0] + fc.random_bytes(MiB, seed=77)
        + inputs()["fp32_n01"][0]
    )


@pytest.mark.parametrize("name", sorted(inputs()))
def test_rule_chooses_the_element_size(name):
    from modal_amd.ops import fpcodec

    data, want = inputs()[name]
    assert len(data) == MiB
    es, est = fpcodec.choose_elem_size(*fpcodec.probe_counts_cpu(data), len(data))
    print(f"{name}: estimate {est / len(data):.4f} of raw, es {es}")
    assert abs(est / len(data) - 0.95) >= 0.01, "a borderline input proves nothing"
    assert es == want


def test_rule_is_the_formula_on_a_table_worked_by_hand():
    """4096 bytes of es 2: 2048 elements, top bytes 1500 x A, 500 x B, 48
    others one each. b=1: 256 + 548 = 804; b=2: 512 + (2048 - 2001) = 559 (the
    third largest count is 1); b=3: 768 + 43; so hi = 559 and the estimate is
    2048 low bytes + 559 + 1 width byte."""
    from modal_amd.ops import fpcodec

    c2 = np.zeros(256, dtype=np.int64)
    c2[0x3F], c2[0xBF], c2[1:49] = 1500, 500, 1
    c4 = np.zeros(256, dtype=np.int64)
    c4[:] = 4  # 1024 elements spread evenly: nothing to gain at es 4
    assert fpcodec.choose_elem_size(c2, c4, 4096) == (2, 2048 + 559 + 1)
    # both spread evenly: b=1 is the cheapest width at either size, 128 + 1020
    # at es 4 against 256 + 2040 at es 2, and 3072 + 1148 + 1 is not worth keeping
    assert fpcodec.choose_elem_size(c4 * 2, c4, 4096) == (0, 3072 + 1148 + 1)


def test_rule_on_many_tables_at_once_is_the_rule_on_each():
    """What ``probe_spans_gpu`` runs on all its spans' tables in one go."""
    from modal_amd.ops import fpcodec

    datas = [d[: MiB - cut] for (d, _w), cut in zip(inputs().values(), (0, 1, 2, 3, 5, 2050, 4097, 0))]
    tables = [fpcodec.probe_counts_cpu(d) for d in datas]
    es, est = fpcodec._choose(
        np.stack([t[0] for t in tables]), np.stack([t[1] for t in tables]), [len(d) for d in datas]
    )
    each = [fpcodec.choose_elem_size(c2, c4, len(d)) for (c2, c4), d in zip(tables, datas)]
    assert list(zip(es.tolist(), est.tolist())) == each
    assert sorted(set(es.tolist())) == [0, 2, 4]


@pytest.mark.parametrize("cut", [0, 1, 2, 3, 5, 2050, 4097])
def test_estimate_bounds_the_payload(cut):
    from modal_amd.ops import fpcodec

    kept = 0
    for name, (full, _want) in sorted(inputs().items()):
        data = full[: MiB - cut]
        counts = dict(zip(fpcodec.ELEM_SIZES, fpcodec.probe_counts_cpu(data)))
        for es in fpcodec.ELEM_SIZES:
            z = fpcodec.compress_buffer_cpu(data, es)
            if z is None:
                continue
            kept += 1
            payload = len(z) - fc.parse(z)[4]
            est = fpcodec._estimate(counts[es], len(data), es)
            print(f"{name} es {es} len {len(data)}: payload {payload}, estimate {est}")
            assert payload <= est + fpcodec.SEG_SIZE
            if len(data) % 4 == 0:
                assert payload <= est
    assert kept >= 6


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 9, 4095, 4096, 4097])
def test_numpy_twin_gives_block_orders_histograms(n):
    from modal_amd.ops import fpcodec

    data = np.frombuffer(fc.bf16_gauss(4098, seed=8)[:n], dtype=np.uint8)
    c2, c4 = fpcodec.probe_counts_cpu(data)
    for es, got in ((2, c2), (4, c4)):
        whole = (n // es) * es
        want = np.bincount(data[es - 1 : whole : es], minlength=256)
        assert got.shape == (256,) and np.array_equal(got, want)
        assert int(got.sum()) == n // es
        # and so the order the codec derives from them is block_order's
        order = np.lexsort((np.arange(256), -got)).astype(np.uint8)
        assert np.array_equal(order, fpcodec.block_order(data, es))


def test_encode_host_auto_finds_each_blocks_element_size():
    from modal_amd.ops import compress, devcodec, fpcodec

    assert fpcodec.AUTO == -1
    data = four_parts()
    plain = devcodec.encode_host(data, block_size=MiB, elem_size=0)
    auto = devcodec.encode_host(data, block_size=MiB, elem_size=fpcodec.AUTO)
    assert [b.compressed for b in auto] == [True, True, False, True]
    assert compress.is_compressed(auto[0].payload) and not fpcodec.is_fp_container(auto[0].payload)
    assert bytes(auto[1].payload) == fpcodec.compress_buffer_cpu(data[MiB : 2 * MiB], 2)
    assert bytes(auto[2].payload) == data[2 * MiB : 3 * MiB]
    assert bytes(auto[3].payload) == fpcodec.compress_buffer_cpu(data[3 * MiB :], 4)
    assert [b.digest for b in auto] == [b.digest for b in plain]
    assert [b.raw_len for b in auto] == [MiB] * 4
    assert devcodec.decode_host([tuple(b) for b in auto]) == data
    with pytest.raises(ValueError):
        devcodec.encode_host(data, block_size=MiB, elem_size=-2)


def test_capture_manifest_auto_codes_float_bytes_under_an_integer_dtype(tmp_path):
    import torch

    from modal_amd.ops import fpcodec
    from modal_amd.runtime import gpu_snapshot as gs
    from modal_amd.scheduler.blobs import BlobStore

    raw = fc.bf16_gauss(2 * MiB, seed=21)
    t = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    manifests, stores = {}, {}
    try:
        for opt in (False, True, "auto"):
            gs._registered_tensors.clear()
            gs._restored_tensors.clear()
            gs.register_tensor("packed", t)
            stores[opt] = BlobStore(str(tmp_path / f"blobs-{opt}"))
            manifests[opt] = pickle.loads(gs.capture_manifest(stores[opt], float_codec=opt))
        entry = manifests["auto"]["tensors"]["packed"]
        assert manifests["auto"]["tensors"] == manifests[False]["tensors"] == manifests[True]["tensors"]
        assert entry["block_lens"] == [2 * MiB] and entry["dtype"] == "uint8"
        stored, compressed = stores["auto"].get_stored(entry["blocks"][0])
        assert compressed and fpcodec.validate_container(stored, 2 * MiB).es == 2
        assert len(stored) < 0.73 * 2 * MiB
        for opt in (False, True):  # a uint8 tensor has no float dtype to hint
            assert stores[opt].get_stored(entry["blocks"][0]) == (raw, False)

        gs._registered_tensors.clear()
        gs._restored_tensors.clear()
        gs.restore_payload(pickle.dumps(manifests["auto"], 4), stores["auto"])  # no flag
        out = gs.restored_tensor("packed")
        assert out.dtype == torch.uint8 and out.numpy().tobytes() == raw

        gs.register_tensor("packed", t)
        with pytest.raises(ValueError, match="float_codec"):
            gs.capture_manifest(stores["auto"], float_codec="yes")
    finally:
        gs._registered_tensors.clear()
        gs._restored_tensors.clear()


def test_scheduler_and_worker_turn_down_other_values():
    import asyncio

    from modal_amd.exception import InvalidError
    from modal_amd.runtime.worker import WorkerRPCTarget
    from modal_amd.scheduler.core import Scheduler

    with pytest.raises(InvalidError, match="float_codec"):
        asyncio.run(Scheduler.worker_snapshot(None, 0, block_addressed=True, float_codec="yes"))
    with pytest.raises(InvalidError, match="block_addressed"):
        asyncio.run(Scheduler.worker_snapshot(None, 0, float_codec="auto"))
    with pytest.raises(InvalidError, match="float_codec"):
        asyncio.run(WorkerRPCTarget.snapshot_manifest(None, float_codec="yes"))

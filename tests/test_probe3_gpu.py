"""The three-way probe on the GPU (ma_rank_probe, csrc/rankhist.hip) and
its callers, every comparison exact."""

import pickle

import numpy as np
import pytest

import byte_corpus as bc
from test_probe3_cpu import MiB, five_parts

pytestmark = pytest.mark.gpu

# 262147: 8 grid-stride steps of the 256-span launch (8 groups x 256 lanes x
# 16 bytes) and 3 bytes, and one step and 3 bytes of the widest grid
LENGTHS = (1, 2, 3, 4, 5, 7, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 262147)
ONE_VALUE = (4097, 262147)  # one byte value: every lane meets on one bin


def _differing(parts: list, offsets: list) -> list:
    """The parts, each at its offset in one buffer of 0xA5, through ONE probe
    launch: the indices whose three tables are not the numpy twin's."""
    import torch

    from modal_amd.ops import load_lib, probe

    host = np.full(-(-(offsets[-1] + len(parts[-1])) // 16) * 16 + 32, 0xA5, dtype=np.uint8)
    for off, data in zip(offsets, parts):
        host[off : off + len(data)] = np.frombuffer(data, dtype=np.uint8)
    buf = torch.from_numpy(host).cuda()
    spans = list(zip(offsets, map(len, parts)))
    got = probe.probe_spans_gpu(load_lib(required=True), buf.data_ptr(), spans)[1].cpu().numpy()
    want = np.zeros((len(parts), 3, 256), dtype=np.int32)
    for k, data in enumerate(parts):
        want[k] = probe.probe_counts_cpu(data)
    assert buf.data_ptr() % 16 == 0 and got.shape == want.shape
    return np.flatnonzero((got != want).any(axis=(1, 2))).tolist()


def test_probe_tables_at_every_alignment():
    """Every length at source residues 0..15 mod 16, 16 to 31 guard bytes
    between spans: a byte from outside a span, one of its own left out or one
    in the wrong table changes a count."""
    e4m3 = bc.fp8(max(LENGTHS) + 16, "float8_e4m3fn", 91)
    parts, offsets, end = [], [], 0
    for n in LENGTHS:
        for r in range(16):
            offsets.append(-(-end // 16) * 16 + 16 + r)
            parts.append(b"\x38" * n if n in ONE_VALUE else e4m3[r : r + n])
            end = offsets[-1] + n
    bad = _differing(parts, offsets)
    assert not bad, [(len(parts[k]), offsets[k] % 16) for k in bad]  # (length, residue)


def test_probe_more_spans_than_one_grid():
    """65536 spans of 8 bytes, one past MAX_GRID_Y, at residues 3 and 11."""
    data = bc.fp8(8 * 65536, "float8_e5m2", 92)
    bad = _differing([data[8 * k : 8 * k + 8] for k in range(65536)], list(range(3, 8 * 65536, 8)))
    assert not bad, bad[-3:]


def test_device_codec_auto_is_the_hosts():
    import torch

    from modal_amd.ops import devcodec, fpcodec

    raw = five_parts()
    src = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    host = devcodec.encode_host(raw, block_size=MiB, elem_size=fpcodec.AUTO)
    got = devcodec.encode_device(src.data_ptr(), len(raw), block_size=MiB, elem_size=fpcodec.AUTO)
    assert [(*b[:2], bytes(b.payload), b.compressed) for b in got] == [
        (*b[:2], bytes(b.payload), b.compressed) for b in host
    ]
    dst = torch.zeros(len(raw), dtype=torch.uint8, device="cuda")
    devcodec.decode_to_device([tuple(b) for b in got], dst.data_ptr(), len(raw), verify=True)
    assert dst.cpu().numpy().tobytes() == raw


def test_auto_snapshot_of_untyped_fp8_memory(tmp_path):
    """e4m3 bytes in a tracked raw allocation, which has no element type."""
    from modal_amd.ops import bytecodec, rawmem
    from modal_amd.runtime import gpu_snapshot as gs
    from modal_amd.scheduler.blobs import BlobStore

    key, want = "raw-fp8-kv", bc.fp8(2 * MiB, "float8_e4m3fn", 93)
    buf = rawmem.RawDeviceBuffer(key, len(want))
    try:
        buf.write(want)
        stores = {opt: BlobStore(str(tmp_path / f"blobs-{opt}")) for opt in (False, "auto")}
        blobs = {opt: gs.capture_manifest(store, float_codec=opt) for opt, store in stores.items()}
        auto, plain = pickle.loads(blobs["auto"]), pickle.loads(blobs[False])
        assert all(auto[part] == plain[part] for part in ("version", "tensors", "raw", "fidelity"))
        entry = auto["raw"][key]
        stored, compressed = stores["auto"].get_stored(entry["blocks"][0])
        assert entry["block_lens"] == [2 * MiB] and compressed and stored[:6] == b"MAFB10"
        assert bytecodec.validate_container(stored, 2 * MiB).es == 1
        buf.free()
        gs.restore_payload(blobs["auto"], stores["auto"])
        assert rawmem.snapshot_all()[key] == want
    finally:
        rawmem.load_lib(required=True).ma_tracked_free(key.encode())

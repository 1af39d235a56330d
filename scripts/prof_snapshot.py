"""Time cross-process GPU snapshot payloads: v1 (one pickled blob) against
v2 (block-addressed manifest, encoded on the device) on one GPU, one process.

For a CUDA tensor of --size-mib per kind -- "pattern" (one 1 KiB unit
repeated: compressible, and every 8 MiB block identical, so the capture
dedups against itself), "distinct" (a different 1 KiB unit per block:
compressible, no dedup), "random" (incompressible) and, when named, "bf16"
(N(0,1) weights as bfloat16: LZ4 stores them raw, --float-codec offers them
to the float-plane codec) and "rawbf16" (the same bytes held in a tracked raw
allocation, ops/rawmem.py, registered as no tensor: only --float-codec auto
reaches them) -- capture + restore through both paths, N timed
runs after one warm-up, median and min-max of host wall time around work
that ends in torch.cuda.synchronize(). v2 also reports the bytes the CAS
stored, the time of a second capture (every block already present), and the
longest single tail-hash dispatch (one lane per short block), measured on a
tensor of --tail-bytes.

    python scripts/prof_snapshot.py --size-mib 1024 --runs 5
    python scripts/prof_snapshot.py --kinds bf16 --float-codec
    python scripts/prof_snapshot.py --kinds rawbf16,random --float-codec auto
"""

from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import tempfile
import time

import torch

from modal_amd.ops import devcodec, rawmem
from modal_amd.runtime import gpu_snapshot as gs
from modal_amd.scheduler.blobs import BLOCK_SIZE, BlobStore

assert torch.cuda.is_available(), "prof_snapshot needs a GPU"

MiB = 1024 * 1024


def make_tensor(kind: str, nbytes: int) -> torch.Tensor:
    gen = torch.Generator(device="cuda").manual_seed(1234)
    if kind == "bf16":
        return torch.randn(nbytes // 2, device="cuda", generator=gen).to(torch.bfloat16)
    if kind == "random":
        return torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=gen)
    if kind == "distinct":
        # a different 1 KiB unit per 8 MiB block: compressible, but no two
        # blocks equal, so nothing dedups inside one capture
        n_blocks = -(-nbytes // BLOCK_SIZE)
        units = torch.randint(0, 256, (n_blocks, 1, 1024), dtype=torch.uint8, device="cuda", generator=gen)
        return units.expand(n_blocks, BLOCK_SIZE // 1024, 1024).reshape(-1)[:nbytes].contiguous()
    unit = torch.randint(0, 256, (1024,), dtype=torch.uint8, device="cuda", generator=gen)
    return unit.repeat(-(-nbytes // 1024))[:nbytes].contiguous()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stored_bytes(root: str) -> int:
    return sum(
        os.path.getsize(os.path.join(d, f)) for d, _s, files in os.walk(root) for f in files
    )


def summary(samples: list) -> dict:
    return {
        "median_s": round(statistics.median(samples), 4),
        "min_s": round(min(samples), 4),
        "max_s": round(max(samples), 4),
    }


RAW_KEY = "prof-snapshot-raw"
_hip = None


def _copy_d2d(dst: int, src: int, nbytes: int) -> None:
    global _hip
    if _hip is None:
        import ctypes

        _hip = ctypes.CDLL("libamdhip64.so")  # the runtime torch has loaded
        _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    torch.cuda.synchronize()
    rc = _hip.hipMemcpy(dst, src, nbytes, 3)  # hipMemcpyDeviceToDevice
    assert rc == 0, f"hipMemcpy -> hipError {rc}"


def reset(t: torch.Tensor, raw: bool = False) -> None:
    """The state a capture sees: t as the registered tensor "w", or, with
    ``raw``, its bytes in a tracked raw allocation and no tensor at all."""
    gs._registered_tensors.clear()
    gs._restored_tensors.clear()
    if raw:
        nbytes = t.numel() * t.element_size()
        _copy_d2d(rawmem.acquire(RAW_KEY, nbytes), t.data_ptr(), nbytes)
    else:
        gs.register_tensor("w", t)


def drop(raw: bool = False) -> None:
    """Forget the state, as a fresh process would have, before a restore."""
    gs._registered_tensors.clear()
    if raw:
        rawmem.load_lib(required=True).ma_tracked_free(RAW_KEY.encode())


def check(t: torch.Tensor, raw: bool = False) -> None:
    if raw:
        ptr, size = rawmem.lookup(RAW_KEY)
        assert ptr and size == t.numel() * t.element_size(), "restore lost the allocation"
        got = torch.empty_like(t)
        _copy_d2d(got.data_ptr(), ptr, size)
    else:
        got = gs.restored_tensor("w")
    assert got.is_cuda and torch.equal(got, t), "restore changed the bytes"


def run_kind(kind: str, nbytes: int, runs: int, float_codec: object = False) -> dict:
    raw = kind == "rawbf16"
    t = make_tensor("bf16" if raw else kind, nbytes)
    times: dict[str, list] = {k: [] for k in ("v1_capture", "v1_restore", "v2_capture", "v2_restore", "v2_second_capture")}
    stored = 0
    for it in range(runs + 1):  # run 0 is the warm-up
        reset(t, raw)
        c1, payload = timed(gs.capture_payload)
        drop(raw)
        r1, _ = timed(lambda: gs.restore_payload(payload))
        check(t, raw)
        v1_bytes = len(payload)
        del payload

        root = tempfile.mkdtemp(prefix="prof-snapshot-")
        try:
            store = BlobStore(root)
            reset(t, raw)
            c2, manifest = timed(lambda: gs.capture_manifest(store, float_codec=float_codec))
            stored = stored_bytes(root)
            c2b, _ = timed(lambda: gs.capture_manifest(store, float_codec=float_codec))
            assert stored_bytes(root) == stored
            drop(raw)
            r2, _ = timed(lambda: gs.restore_payload(manifest, store))
            check(t, raw)
        finally:
            shutil.rmtree(root, ignore_errors=True)
        if it:
            for key, val in zip(times, (c1, r1, c2, r2, c2b)):
                times[key].append(val)
    drop(raw)
    out = {"kind": kind, "float_codec": float_codec, "nbytes": nbytes, "v1_payload_bytes": v1_bytes, "v2_stored_bytes": stored}
    out.update({key: summary(vals) for key, vals in times.items()})
    return out


def tail_hash(nbytes: int) -> dict:
    t = make_tensor("random", nbytes)
    devcodec.encode_tensor(t)  # warm-up
    devcodec.last_stats.update(tail_hash_s=0.0, tail_hash_max_len=0)
    devcodec.encode_tensor(t)
    return {"tail_bytes": nbytes, "tail_hash_dispatch_s": round(devcodec.last_stats["tail_hash_s"], 4)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mib", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tail-bytes", type=int, default=8 * MiB - 1)
    ap.add_argument("--kinds", default="pattern,distinct,random")
    ap.add_argument("--float-codec", nargs="?", const=True, default=False, choices=["auto"],
                    help="capture_manifest(float_codec=True): MAFP10 for float tensors; "
                         "'--float-codec auto': also for untyped tensors and raw allocations, "
                         "at the element size probed in their bytes")
    args = ap.parse_args()
    for kind in args.kinds.split(","):
        print(json.dumps(run_kind(kind, args.size_mib * MiB, args.runs, args.float_codec)), flush=True)
    print(json.dumps(tail_hash(args.tail_bytes)), flush=True)


if __name__ == "__main__":
    main()

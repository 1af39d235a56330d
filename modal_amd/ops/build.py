"""Build the HIP ops library in-tree with hipcc (gfx950 only, no multi-arch).

The built .so is git-ignored but ships to GPU boxes with the repo snapshot.
"""

from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile

_THIS_DIR = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_THIS_DIR, "csrc")
SOURCES = ["sha256.hip", "pack.hip", "lz4.hip", "rawmem.hip", "malz.hip", "fpz.hip", "bytez.hip",
           "ricez.hip", "lz4w.hip", "sha256w.hip", "rankhist.hip", "lz4s.hip"]
HEADERS = ["malz_common.h", "rank_common.h", "lz4_lane.h", "lz4_wave.h"]  # included by SOURCES: a change rebuilds
# Kernel files added from now on are compiled on their own with packed fp32
# instructions turned off, some forms of which miscompute on gfx950, and
# linked in as objects; the files above them in SOURCES build as they always
# did. bytez.hip, ricez.hip, lz4w.hip, sha256w.hip, rankhist.hip and lz4s.hip have no float math: they come out with the
# same registers and no spills either way (kernel-resource-usage), the flag
# only keeps a later float addition to them off those instructions. The host
# pass does not know the feature and says so once per kernel; that warning is
# harmless.
NO_PACKED_FP32 = ["bytez.hip", "ricez.hip", "lz4w.hip", "sha256w.hip", "rankhist.hip", "lz4s.hip"]
_NO_PACKED_FP32_FLAGS = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]


def _hipcc() -> str:
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found; ROCm toolchain required to build modal_amd ops")
    return hipcc


def needs_build() -> bool:
    from . import lib_path

    out = lib_path()
    if not os.path.exists(out):
        return True
    out_mtime = os.path.getmtime(out)
    for src in SOURCES + HEADERS:
        if os.path.getmtime(os.path.join(_CSRC, src)) > out_mtime:
            return True
    return False


def build(verbose: bool = True, force: bool = False) -> str:
    from . import lib_path

    out = lib_path()
    if not force and not needs_build():
        return out
    common = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]

    def run(cmd: list) -> None:
        if verbose:
            print("[modal_amd.ops]", " ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True, capture_output=not verbose)

    with tempfile.TemporaryDirectory(prefix="modal_amd_ops_") as tmp:
        objects = []
        for src in NO_PACKED_FP32:
            objects.append(os.path.join(tmp, os.path.splitext(src)[0] + ".o"))
            run([*common, *_NO_PACKED_FP32_FLAGS, "-c", os.path.join(_CSRC, src), "-o", objects[-1]])
        together = [os.path.join(_CSRC, src) for src in SOURCES if src not in NO_PACKED_FP32]
        # objects first: hipcc marks every .hip source, and what follows it, as HIP
        run([*common, "-shared", *objects, *together, "-o", out])
    return out


if __name__ == "__main__":
    build()

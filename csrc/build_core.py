"""Build modal_amd/_core.so (pybind11, C++20) in-tree."""

from __future__ import annotations

import os
import subprocess
import sys
import sysconfig

_THIS = os.path.dirname(os.path.abspath(__file__))
_REPO = os.path.dirname(_THIS)
_OUT = os.path.join(_REPO, "modal_amd", f"_core{sysconfig.get_config_var('EXT_SUFFIX')}")


def _sources() -> list[str]:
    """core.cpp and every header under csrc/ (it includes them): a change
    to any of these makes the module stale."""
    return [os.path.join(_THIS, "core.cpp")] + sorted(
        os.path.join(_THIS, name)
        for name in os.listdir(_THIS)
        if name.endswith((".h", ".hpp"))
    )


def needs_build() -> bool:
    if not os.path.exists(_OUT):
        return True
    built = os.path.getmtime(_OUT)
    return any(os.path.getmtime(src) > built for src in _sources())


def build(verbose: bool = True, force: bool = False) -> str:
    if not force and not needs_build():
        return _OUT
    import pybind11

    cmd = [
        "g++",
        "-O3",
        "-std=c++20",
        "-shared",
        "-fPIC",
        "-pthread",
        f"-I{pybind11.get_include()}",
        f"-I{sysconfig.get_paths()['include']}",
        os.path.join(_THIS, "core.cpp"),
        "-o",
        _OUT,
    ]
    if verbose:
        print("[modal_amd._core]", " ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, capture_output=not verbose)
    return _OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)

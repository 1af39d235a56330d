"""Compare our public class surfaces against the reference's, by AST.

For each mapped (reference file, class) -> (our module, class), list public
methods/properties the reference exposes that we don't. Names in ALLOW are
accepted gaps (documented in docs/PARITY.md). Run: python scripts/api_audit.py
Exit code 1 if any unexplained gap exists (used by tests).

The reference's public member names are recorded in
tests/golden/ref_api_members.json, so the audit needs no reference checkout.
`python scripts/api_audit.py --ref <reference>/py/modal` re-parses a reference
tree instead, and with `--record` rewrites the recorded list from it.
"""

from __future__ import annotations

import argparse
import ast
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

GOLDEN = os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ref_api_members.json"
)

# (ref_file, ref_class) -> (our_module, our_class)
MAP = [
    ("app.py", "_App", "modal_amd.app", "App"),
    ("_functions.py", "_Function", "modal_amd.functions", "_Function"),
    ("_functions.py", "_FunctionCall", "modal_amd.functions", "_FunctionCall"),
    ("queue.py", "_Queue", "modal_amd.queue", "_Queue"),
    ("dict.py", "_Dict", "modal_amd.dict", "_Dict"),
    ("secret.py", "_Secret", "modal_amd.secret", "_Secret"),
    ("volume.py", "_Volume", "modal_amd.volume", "_Volume"),
    ("sandbox.py", "_Sandbox", "modal_amd.sandbox", "_Sandbox"),
    ("_image.py", "_Image", "modal_amd.image", "_Image"),
    ("cls.py", "_Cls", "modal_amd.cls", "Cls"),
    ("network_file_system.py", "_NetworkFileSystem",
     "modal_amd.network_file_system", "_NetworkFileSystem"),
]

# Accepted, documented gaps (docs/PARITY.md explains each).
ALLOW = {
    "App": {
        "get_dashboard_url",  # no hosted dashboard in a local-first control plane
        "_uncreate",  # internal in reference too (underscore caught by filter normally)
    },
    "_Function": {
        "from_name",  # exposed as Function.from_name on the wrapper (classmethod there)
    },
    "_Image": {
        "from_gcp_artifact_registry",  # alias present; audit sees decorator wrappers
    },
}


def ref_members(ref: str, path: str, klass: str) -> set[str]:
    tree = ast.parse(open(f"{ref}/{path}").read())
    for node in ast.walk(tree):
        if isinstance(node, ast.ClassDef) and node.name == klass:
            out = set()
            for item in node.body:
                if isinstance(item, (ast.FunctionDef, ast.AsyncFunctionDef)):
                    if not item.name.startswith("_"):
                        out.add(item.name)
            return out
    return set()


def our_members(module: str, klass: str) -> set[str]:
    mod = importlib.import_module(module)
    cls = getattr(mod, klass)
    return {n for n in dir(cls) if not n.startswith("_")}


def main() -> int:
    parser = argparse.ArgumentParser()
    parser.add_argument("--ref", default=None, help="parse this reference py/modal tree")
    parser.add_argument("--record", action="store_true", help="rewrite the recorded names from --ref")
    args = parser.parse_args()
    if args.record and not args.ref:
        parser.error("--record needs --ref")
    if args.ref:
        recorded = {
            f"{ref_file}::{ref_cls}": sorted(ref_members(args.ref, ref_file, ref_cls))
            for ref_file, ref_cls, _, _ in MAP
        }
        if args.record:
            with open(GOLDEN, "w") as f:
                json.dump(recorded, f, indent=1, sort_keys=True)
                f.write("\n")
    else:
        with open(GOLDEN) as f:
            recorded = json.load(f)
    bad = 0
    for ref_file, ref_cls, our_mod, our_cls in MAP:
        want = set(recorded[f"{ref_file}::{ref_cls}"])
        have = our_members(our_mod, our_cls)
        missing = sorted(want - have - ALLOW.get(our_cls, set()) - ALLOW.get(ref_cls, set()))
        if missing:
            print(f"{our_cls}: missing {missing}")
            bad = 1
        else:
            print(f"{our_cls}: ok ({len(want)} reference members covered)")
    return bad


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Statement fingerprints of the reference's core/*.py for
tests/test_host_api.py::test_host_modules_are_not_transliterations.

    python oracle/gen_golden_overlap.py <reference>/src/wt_simulator/core

Every file goes through tools/overlap_check.normalised_lines (ast, docstrings and comments dropped, one
statement per line); each distinct statement is stored only as the first 16 hex digits of its SHA-256.
No statement text is written, so the fixture carries no reference source, yet the test can count how many
of a host module's statements occur verbatim in the reference without the reference present.

Output: tests/golden/g12_reference_core_statements.json
"""
from __future__ import annotations

import glob
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import overlap_check as oc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g12_reference_core_statements.json")


def digest(statement: str) -> str:
    return hashlib.sha256(statement.encode("utf-8")).hexdigest()[:16]


def main(core_dir: str) -> None:
    files = sorted(glob.glob(os.path.join(core_dir, "*.py")))
    if not files:
        raise SystemExit(f"no *.py under {core_dir}")
    known = set()
    for f in files:
        known.update(digest(l) for l in oc.normalised_lines(f))
    doc = {"what": "sha256(normalised statement)[:16] of every statement of the reference's core/*.py "
                   "(tools/overlap_check.normalised_lines); statement text is not stored",
           "files": [os.path.basename(f) for f in files],
           "digests": sorted(known)}
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=0)
        fh.write("\n")
    print(f"{OUT}: {len(known)} statements from {len(files)} files")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])

#!/usr/bin/env python3
"""Generates tests/golden/known_work.json: the shape tests/test_gpu_known_work.py needs and tests/golden/differential.json does
not hold — |K| = 8, below the size from which round 3 keeps f on K and lays it out by cosets (differential.json has |K| = 4 and
16, 32, ..., none of 8).  The Python model (oracle/pyref) indexes and proves the system of tests/differential_model.py::emit
for the parameters below and records the bytes the product must reproduce, in the record format of differential.json.
Run from the repo root:  python tests/golden/gen_golden_known_work.py  (under a minute)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

from pyref.poly import Domain  # noqa: E402
from gen_golden_differential import run_case  # noqa: E402

# seven rows of one term in A, one in B and one in C: 7 non-zero entries per matrix
CASES = [("k_8", dict(seed=181, inputs=1, free=2, rows=7, a=[1, 1], b=[1, 1]))]


def main():
    recs = []
    for item in CASES:
        rec, props, secs = run_case(item)
        H, K = Domain(rec["num_constraints"]).size, Domain(rec["num_non_zero"]).size
        print(" %-10s %5.1fs  |H| %3d |K| %3d  %s" % (rec["name"], secs, H, K, " ".join(props)))
        assert K == 8, K
        recs.append(rec)
    path = os.path.join(HERE, "known_work.json")
    with open(path, "w") as f:
        json.dump({"cases": recs}, f, indent=0, separators=(",", ":"))
    print("wrote known_work.json", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates tests/golden/differential.json: for every case of tests/differential_model.py::CASES the Python model
(oracle/pyref) indexes and proves the random odd-shaped system and records the proof and verifying-key bytes the product
must reproduce.  Run from the repo root:  python tests/golden/gen_golden_differential.py  (a few minutes on 8 cores).

The generator also holds the table to the coverage list below: every property must be carried by at least one case, judged
on the model's own index (pk["index"].a/.b/.c after padding and balancing, the vk's three sizes) — except the three
balance properties, which compare nnz(A) with nnz(B) BEFORE balancing, and the three term properties (duplicate, cancelling
pair, zero coefficient), which exist only in the builder's terms.  It prints which case carries which property.
"""
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

from pyref import marlin as M  # noqa: E402
from pyref.bls12_377 import R  # noqa: E402
from pyref.poly import Domain  # noqa: E402
import differential_model as D  # noqa: E402


def srs_sizes(cs):
    """(num_constraints, num_variables, max nnz) of the unpadded system."""
    mats = cs.to_matrices()
    return (cs.num_constraints, len(cs.instance) + len(cs.witness), max(sum(len(r) for r in m) for m in mats))


def find_flip(cs):
    """The first witness whose value + 1 leaves the system unsatisfied."""
    for i in range(len(cs.witness)):
        bad = cs.copy()
        bad.witness[i] = (bad.witness[i] + 1) % R
        if not bad.is_satisfied():
            return i
    raise AssertionError("no witness whose change breaks the system")


def properties(cs, pk, vk):
    """The coverage properties this case carries."""
    idx = pk["index"]
    nc = cs.num_constraints
    nv = Domain(len(cs.instance)).size + len(cs.witness)
    H, K = Domain(vk["num_constraints"]).size, Domain(vk["num_non_zero"]).size
    got = {"instance_%d" % len(cs.instance)}
    got.add("vars_gt_rows" if nv > nc else "rows_gt_vars" if nc > nv else "rows_eq_vars")
    got.add("K_gt_H" if K > H else "K_lt_H" if K < H else "K_eq_H")
    for i in range(nc):
        ea, eb, ec = (not m[i] for m in (idx.a, idx.b, idx.c))
        if ea and eb and ec:
            got.add("row_all_empty")
        else:
            got.update(n for n, e in (("row_a_empty", ea), ("row_b_empty", eb), ("row_c_empty", ec)) if e)
    if any(not any(m) for m in (idx.a, idx.b, idx.c)):
        got.add("matrix_empty")
    for rows in (cs.a, cs.b, cs.c):
        for lc in rows:
            by_col = {}
            for coeff, var in lc:
                by_col.setdefault(var, []).append(coeff % R)
            for coeffs in by_col.values():
                if 0 in coeffs:
                    got.add("zero_coefficient")
                nz = [c for c in coeffs if c]
                if len(nz) >= 2:
                    got.add("cancelling_pair" if sum(nz) % R == 0 else "duplicate_column")
    if not any(cs.instance[1:]) and not any(cs.witness):
        got.add("zero_assignment")
    a0, b0, _ = cs.to_matrices()
    na, nb = sum(len(r) for r in a0), sum(len(r) for r in b0)
    got.add("nnz_a_gt_b" if na > nb else "nnz_a_lt_b" if na < nb else "nnz_a_eq_b")
    lens = [len(r) for m in (idx.a, idx.b) for r in m]
    got.update(n for n, ok in (("row_64", 64 in lens), ("row_65", 65 in lens), ("row_about_70", any(66 <= x <= 80 for x in lens)),
                               ("row_over_4", any(x > 4 for x in lens))) if ok)
    for m in (idx.a, idx.b, idx.c):
        use = {}
        for r in m:
            for _, col in r:
                use[col] = use.get(col, 0) + 1
        if use and max(use.values()) >= 65:
            got.add("column_in_65_rows")
    assert vk["num_non_zero"] >= 2
    if "column_in_65_rows" not in got:
        assert nc <= 64 and nv <= 80, (nc, nv)
    return sorted(got)


REQUIRED = (["instance_%d" % n for n in (1, 2, 3, 4, 6, 9, 17)]
            + ["vars_gt_rows", "rows_gt_vars", "rows_eq_vars", "K_gt_H", "K_eq_H", "K_lt_H",
               "row_a_empty", "row_b_empty", "row_c_empty", "row_all_empty", "matrix_empty", "zero_assignment",
               "nnz_a_gt_b", "nnz_a_lt_b", "nnz_a_eq_b", "row_64", "row_65", "row_about_70", "row_over_4", "column_in_65_rows"])
REQUIRED_IN_FIVE = ["duplicate_column", "cancelling_pair", "zero_coefficient"]


def run_case(item):
    name, params = item
    t = time.time()
    cs = M.ConstraintSystem()
    public = D.emit(cs, params)
    assert public == cs.instance[1:]
    assert cs.is_satisfied(), name
    sizes = srs_sizes(cs)
    rng = M.generate_rand()
    srs = M.generate_universal_srs(*sizes, rng)
    try:
        pk, vk = M.generate_proving_and_verifying_keys(srs, cs)
    except M.MarlinError as e:
        raise AssertionError("%s: the model cannot index it: %s" % (name, e))
    pbytes = M.serialize_proof(M.generate_proof(cs, pk, rng))
    assert M.verify_proof(vk, public, M.deserialize_proof(pbytes), rng), name
    if public:
        wrong = [(public[0] + 1) % R] + public[1:]
        assert not M.verify_proof(vk, wrong, M.deserialize_proof(pbytes), M.generate_rand()), name
    rec = {"name": name, "params": params, "srs": list(sizes), "max_degree": srs.max_degree,
           "num_constraints": vk["num_constraints"], "num_variables": vk["num_variables"], "num_non_zero": vk["num_non_zero"],
           "public_input": [hex(x) for x in public], "flip": find_flip(cs),
           "proof": pbytes.hex(), "vk": M.serialize_verifying_key(vk).hex()}
    return rec, properties(cs, pk, vk), time.time() - t


def main():
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        results = list(pool.map(run_case, D.CASES))
    carriers = {}
    for rec, props, secs in results:
        print(" %-26s %5.1fs  |H| %3d |K| %3d  %s" % (rec["name"], secs, Domain(rec["num_constraints"]).size,
                                                     Domain(rec["num_non_zero"]).size, " ".join(props)))
        for prop in props:
            carriers.setdefault(prop, []).append(rec["name"])
    print("coverage:")
    for prop in REQUIRED + REQUIRED_IN_FIVE:
        names = carriers.get(prop, [])
        print(" %-20s %2d  %s" % (prop, len(names), " ".join(names)))
        assert len(names) >= (5 if prop in REQUIRED_IN_FIVE else 1), "no case carries " + prop
    no_input = [rec["name"] for rec, _, _ in results if not rec["public_input"]]
    assert no_input == D.NO_PUBLIC_INPUT
    path = os.path.join(HERE, "differential.json")
    with open(path, "w") as f:
        json.dump({"cases": [rec for rec, _, _ in results]}, f, indent=0, separators=(",", ":"))
    print("wrote differential.json", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 150 * 1024


if __name__ == "__main__":
    main()

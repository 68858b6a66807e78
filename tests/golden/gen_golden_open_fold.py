#!/usr/bin/env python3
"""Golden proofs for the folded opening witnesses (tests/test_gpu_open_fold.py), written to tests/golden/marlin_open_fold.json.
Run from the repo root (about a minute of CPU per case):

    python tests/golden/gen_golden_open_fold.py

The prover is the independent Python model (oracle/pyref/marlin.py), nothing of the product runs here.  Two random sparse
circuits under an SRS of their own degree D = max(3|H| - 1, 3|K| - 3), so that the shifted powers are a sub-range of the powers
and the key has window tables (>= 512 powers):
  * wide_K: |K| = 256 > |H| = 128.  D = 3|K| - 3: the merged witness vector ends at D at BOTH query points, above the
    beta quotient (3|H| - 1 coefficients) as well as the gamma one;
  * wide_H: |K| = 64 < |H| = 256.  D = 3|H| - 1: at beta the shifted range lies inside the plain quotient, at gamma the
    merged vector is four times as long as the plain quotient.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (os.path.join(ROOT, "oracle"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from pyref import marlin as M  # noqa: E402
from pyref.poly import Domain  # noqa: E402

CASES = (("wide_K", dict(seed=31, num_inputs=3, free_witnesses=4, num_constraints=60), 128, 256),
         ("wide_H", dict(seed=32, num_inputs=3, free_witnesses=200, num_constraints=20), 256, 64))


def main():
    out = {}
    for name, kw, H, K in CASES:
        cs = M.random_sparse_circuit(**kw)
        assert cs.is_satisfied()
        ics = M.pad_and_square(cs)
        nnz = max(sum(len(r) for r in m) for m in ics.to_matrices())
        nv = len(ics.instance) + len(ics.witness)
        assert (Domain(max(nv, ics.num_constraints)).size, Domain(nnz).size) == (H, K), name
        sizes = (ics.num_constraints, nv, nnz)
        rng = M.generate_rand()
        srs = M.generate_universal_srs(*sizes, rng)
        assert srs.max_degree == max(3 * H - 1, 3 * K - 3)
        pk, vk = M.generate_proving_and_verifying_keys(srs, cs)
        proof = M.serialize_proof(M.generate_proof(cs, pk, rng))
        public = cs.instance[1:]
        assert M.verify_proof(vk, public, M.deserialize_proof(proof), rng)
        out[name] = {"circuit": kw, "srs": list(sizes), "max_degree": srs.max_degree, "H": H, "K": K,
                     "public_input": [hex(x) for x in public], "proof": proof.hex(), "vk": M.serialize_verifying_key(vk).hex()}
        print(name, sizes, srs.max_degree, len(proof), flush=True)
    with open(os.path.join(HERE, "marlin_open_fold.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates tests/golden/key_forms.json: the serialize_uncompressed form [U: ark-ec 0.3] of the proving and verifying keys of the
three circuits of pk_bytes.json (same SRS sizes, a fresh test_rng each), written by the serializer BELOW from the Python model's key
objects (oracle/pyref) — not by the library under test.  Run from the repo root:  python tests/golden/gen_golden_key_forms.py

The uncompressed layout is the compressed one (pyref.marlin.serialize_proving_key / serialize_verifying_key) with every point
widened: G1 = x || y (96 bytes), G2 = x.c0 || x.c1 || y.c0 || y.c1 (192 bytes), the infinity flag in bit 6 of the last byte, the
identity as (0, 1) resp. (0, (1, 0)).  Field elements, lengths, Option tags, labels, matrices and domains are the same.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))

from pyref import marlin as M  # noqa: E402
from pyref.poly import Domain  # noqa: E402


def ser_g1_unc(P):
    if P is None:
        b = bytearray(M.tb_fq(0) + M.tb_fq(1))
        b[95] |= 0x40
        return bytes(b)
    return M.tb_fq(P[0]) + M.tb_fq(P[1])


def ser_g2_unc(P):
    if P is None:
        b = bytearray(M.tb_fq(0) * 2 + M.tb_fq(1) + M.tb_fq(0))
        b[191] |= 0x40
        return bytes(b)
    x, y = P
    return M.tb_fq(x.c0) + M.tb_fq(x.c1) + M.tb_fq(y.c0) + M.tb_fq(y.c1)


def ser_commitment_unc(comm):
    c, s = comm
    return ser_g1_unc(c) + (b"\x01" + ser_g1_unc(s) if s is not None else b"\x00")


def serialize_verifying_key_unc(vk):
    u64 = M.ser_u64
    out = u64(vk["num_variables"]) + u64(vk["num_constraints"]) + u64(vk["num_non_zero"]) + u64(vk["num_instance_variables"])
    out += u64(len(vk["index_comms"])) + b"".join(ser_commitment_unc(c) for c in vk["index_comms"])
    pv = vk["verifier_key"]
    out += ser_g1_unc(pv["g"]) + ser_g1_unc(pv["gamma_g"]) + ser_g2_unc(pv["h"]) + ser_g2_unc(pv["beta_h"])
    out += b"\x01" + u64(len(pv["degree_bounds_and_shift_powers"]))
    for d, p in pv["degree_bounds_and_shift_powers"]:
        out += u64(d) + ser_g1_unc(p)
    return out + u64(pv["max_degree"]) + u64(pv["supported_degree"])


def serialize_proving_key_unc(pk):
    u64 = M.ser_u64
    vk, idx, ck = pk["vk"], pk["index"], pk["ck"]
    out = serialize_verifying_key_unc(vk)
    out += u64(len(pk["index_comm_rands"]))
    for _ in pk["index_comm_rands"]:
        out += M.ser_fr_vec([]) + b"\x00"
    out += u64(idx.num_variables) + u64(idx.num_constraints) + u64(idx.num_non_zero) + u64(idx.num_instance_variables)
    out += M.ser_matrix(idx.a) + M.ser_matrix(idx.b) + M.ser_matrix(idx.c)
    dk = Domain(idx.num_non_zero)
    db = Domain(3 * dk.size - 3)
    for m in "abc":
        ar = idx.arith[m]
        for n in ("row", "col", "val", "row_col"):
            out += M.ser_labeled_poly(m + "_" + n, ar[n])
        for dom, suf in ((dk, "_K"), (db, "_B")):
            for n in ("row", "col", "val"):
                out += M.ser_evals(ar[n + suf], dom)
        out += M.ser_evals(ar["row_col_B"], db)
    out += u64(len(ck.powers)) + b"".join(ser_g1_unc(p) for p in ck.powers)
    out += b"\x01" + u64(len(ck.shifted_powers)) + b"".join(ser_g1_unc(p) for p in ck.shifted_powers)
    out += u64(len(ck.powers_of_gamma_g)) + b"".join(ser_g1_unc(p) for p in ck.powers_of_gamma_g)
    out += b"\x01" + u64(len(ck.enforced_degree_bounds)) + b"".join(u64(d) for d in ck.enforced_degree_bounds)
    return out + u64(ck.max_degree)


def main():
    out = {}
    for name, cs, sizes in (("manual_constraints", M.manual_constraints_circuit(1, 1), (100, 25, 300)),
                            ("synthetic_8", M.synthetic_circuit(8, 3, 5), (8, 8, 8)),
                            ("random_sparse", M.random_sparse_circuit(seed=20261002), None)):
        if sizes is None:
            a_m, b_m, c_m = cs.to_matrices()
            sizes = (cs.num_constraints, len(cs.instance) + len(cs.witness), max(sum(len(r) for r in m) for m in (a_m, b_m, c_m)))
        srs = M.generate_universal_srs(*sizes, M.generate_rand())
        pk, vk = M.generate_proving_and_verifying_keys(srs, cs)
        pkb, vkb = serialize_proving_key_unc(pk), serialize_verifying_key_unc(vk)
        assert pkb.startswith(vkb)
        # "vk_compressed" / "vk_bytes": both forms of the (small) verifying key in full, so that the host tests need no device
        out[name] = {"srs": list(sizes),
                     "pk": {"len": len(pkb), "sha256": hashlib.sha256(pkb).hexdigest(), "head": pkb[:64].hex()},
                     "vk": {"len": len(vkb), "sha256": hashlib.sha256(vkb).hexdigest(), "head": vkb[:64].hex()},
                     "vk_bytes": vkb.hex(), "vk_compressed": M.serialize_verifying_key(vk).hex()}
        print(" key forms", name, len(pkb), len(vkb))
    path = os.path.join(HERE, "key_forms.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
    print("wrote key_forms.json", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

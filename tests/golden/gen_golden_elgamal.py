#!/usr/bin/env python3
"""Writes tests/golden/elgamal.json from tests/elgamal_model.py (the big-integer restatement of ark-crypto-primitives' ElGamal on
ed-on-BLS12-377, which the reference exercises in tests/encrypt.rs).  Run from the repo root:
python3 tests/golden/gen_golden_elgamal.py            (deterministic: every value comes from pyref's test_rng stream)

  * "generator": setup's draw from a fresh test_rng.
  * "valid": 64 tuples drawn from the same stream after it, each in the order of tests/encrypt.rs — keygen (sk, pk), a random
    message, the randomness r — with the model's ciphertext (c1, c2), and "c2_to_key0": c2 of the same (message, r) under
    valid[0]'s public key (c1 does not depend on the key), for the one-recipient path.
  * "edge": cases (scalar k, point P, message M) with a note.  Each holds the model's ciphertext (c1, c2) of pk = P, m = M, r = k,
    and the model's "plaintext" of sk = k, ciphertext (P, M), i.e. M - k P.  Scalars at the ends of the range, with zero bytes
    (rows the table walk skips) and with the nibble patterns that give the ladder's digits -7, 0 and 8 and the carry between
    nibbles; P and M at the identity, the points of order 2 and 4 and an on-curve point outside the prime subgroup; M = -(k P),
    where c2 is the identity; P = the generator.
All hex strings are the bytes as they cross the C ABI (little-endian values)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import elgamal_model as E
from pyref import rng as pyrng
from pyref.bls12_377 import R
from pyref.pedersen import ED_SUBGROUP_ORDER as L
from pyref.pedersen import ed_add, ed_mul, ed_on_curve, fr_sqrt


def le32(v):
    return v.to_bytes(32, "little").hex()


def pt(p):
    return E.point_bytes(p).hex()


def build():
    rng = pyrng.test_rng()
    G = E.setup(rng)
    assert ed_on_curve(G) and G != E.IDENTITY and ed_mul(G, L) == E.IDENTITY
    valid, key0 = [], None
    for i in range(64):
        pk, sk = E.keygen(G, rng)
        m = E.rand_plaintext(rng)
        r = E.rand_randomness(rng)
        key0 = key0 or pk
        c1, c2 = E.encrypt(G, pk, m, r)
        assert E.decrypt(sk, (c1, c2)) == m and ed_mul(m, L) == E.IDENTITY
        valid.append({"secret": le32(sk), "public_key": pt(pk), "message": pt(m), "randomness": le32(r), "c1": pt(c1), "c2": pt(c2),
                      "c2_to_key0": pt(E.encrypt(G, key0, m, r)[1])})
    assert valid[0]["c2_to_key0"] == valid[0]["c2"]

    i4 = fr_sqrt(R - 1)                      # a = -1: the points of order 4 are (+-sqrt(-1), 0), the point of order 2 is (0, -1)
    o2, o4a, o4b = (0, R - 1), (i4, 0), (R - i4, 0)
    assert ed_add(o2, o2) == E.IDENTITY and ed_add(o4a, o4a) == o2 and ed_add(o4b, o4b) == o2 and ed_add(o4a, o4b) == E.IDENTITY
    P, M = E.point_from_bytes(bytes.fromhex(valid[1]["public_key"])), E.point_from_bytes(bytes.fromhex(valid[1]["message"]))
    outside = ed_add(P, o4a)
    assert ed_on_curve(outside) and ed_mul(outside, L) != E.IDENTITY
    rnd = int.from_bytes(bytes.fromhex(valid[2]["randomness"]), "little")
    # e + 0x0777..7 nibble by nibble: nibble 0 (no carry in) is digit 0, nibble 8 digit 8, nibble 9 digit -7 with a carry out
    scalars = [("k = 0", 0), ("k = 1", 1), ("k = 2", 2), ("k = l - 1", L - 1), ("k = l - 2", L - 2),
               ("k: every odd byte zero", int.from_bytes(bytes(0xA7 if i % 2 == 0 else 0 for i in range(32)), "little")),
               ("k: only byte 30", 0xC3 << 240), ("k: only bytes 0 and 17", 0x5A | 0xFF << 136),
               ("k = 0x0111..1 (every digit 1)", int("0" + "1" * 63, 16)),
               ("k = 0x0388..8 (digits 8)", int("03" + "8" * 62, 16)),
               ("k = 0x0399..9 (digit -7, then -6 under the carry)", int("03" + "9" * 62, 16)),
               ("k = 0x0398 98.. (digits 8 and -7 alternate)", int("03" + "98" * 31, 16)),
               ("k = 0x0..0f (digit -1, carry into a zero nibble)", 0xF),
               ("k = 0x0409 09.. (zero nibbles between carries)", int("04" + "09" * 31, 16)),
               ("k = 0x0407 97.. (nibble 7 under a carry: digit 8)", int("04" + "07" + "97" * 30, 16)),
               ("k = l - 17 (top nibble 4, just below l)", L - 17),
               ("k = 2^250", 1 << 250)]
    assert all(0 <= k < L for _, k in scalars) and (L >> 248) == 4
    special = [("the identity", E.IDENTITY), ("the point of order 2", o2), ("a point of order 4", o4a),
               ("the other point of order 4", o4b), ("a point outside the prime subgroup", outside)]
    some = [("k = l - 1", L - 1), ("k random", rnd), ("k = 0x0399..9", int("03" + "9" * 62, 16))]
    cases = []

    def add(note, k, p, m):
        assert ed_on_curve(p) and ed_on_curve(m) and 0 <= k < L
        c1, c2 = E.encrypt(G, p, m, k)
        plain = E.decrypt(k, (p, m))
        cases.append({"note": note, "scalar": le32(k), "point": pt(p), "message": pt(m), "c1": pt(c1), "c2": pt(c2), "plaintext": pt(plain)})
    for name, k in scalars:
        add("subgroup point and message, " + name, k, P, M)
    n = 0
    for pname, p in special:
        for _ in range(2):
            kname, k = some[n % 3]
            n += 1
            add("point = %s, %s" % (pname, kname), k, p, M)
    for pname, p in special:
        for _ in range(2):
            kname, k = some[n % 3]
            n += 1
            add("message = %s, %s" % (pname, kname), k, P, p)
    add("point = message = the identity, k = 0", 0, E.IDENTITY, E.IDENTITY)
    add("point and message outside the prime subgroup, k = l - 1", L - 1, outside, ed_add(M, o2))
    for kname, k in some[1:]:
        add("message = -(k point): c2 is the identity, " + kname, k, P, E.ed_neg(ed_mul(P, k)))
        assert cases[-1]["c2"] == pt(E.IDENTITY)
    for kname, k in some[:2]:
        add("point = the generator, " + kname, k, G, M)
        assert cases[-1]["c2"] == pt(ed_add(M, E.point_from_bytes(bytes.fromhex(cases[-1]["c1"]))))
    assert len(cases) >= 40
    return {"note": "generated by tests/golden/gen_golden_elgamal.py from tests/elgamal_model.py; hex = the bytes of the C ABI",
            "generator": pt(G), "group_order": hex(L), "valid": valid, "edge": cases}


def main():
    out = build()
    path = os.path.join(ROOT, "tests", "golden", "elgamal.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote tests/golden/elgamal.json: %d tuples, %d edge cases, %d bytes" % (len(out["valid"]), len(out["edge"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()

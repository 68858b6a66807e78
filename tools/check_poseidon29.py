#!/usr/bin/env python3
"""Bit-level emulation of the Poseidon kernel's arithmetic (simpleworks_amd/csrc/poseidon.hip) on the multiplier model of
tools/check_ntt29.py: every uint32 limb operation and every 64-bit column sum is checked for wrap-around, the bounds stated at
the head of poseidon.hip are asserted where the kernel relies on them (t < 9r with limbs < 5 x 2^29, a matrix row < 6r with limbs
< 3 x 2^29, every product below 2^261 r), and the squeezed elements are compared with the big-integer model
tests/poseidon_model.py.  Parameter sets: every matrix entry and round key r - 1, the identity matrix with zero keys, the
reference's set; alpha 2 .. 65535; with and without partial rounds.  CPU only, about ten seconds of pure Python
(tests/test_poseidon29_emulation.py runs a subset); run: python tools/check_poseidon29.py"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import poseidon_model as P
from check_ntt29 import R, add, limbs, normalize, val
from check_ntt29 import mul as mul29

TO_MONT = limbs(pow(2, 522, R))   # row 0 of the kernel's table
ONE = limbs(1)
max_limb = 0


def mul(a, b):
    return mul29(a, b, top_bits=25)     # a normalised value < 9r < 2^257 leaves the top limb below 2^25


def bounded(a, limb_bound, value_bound):
    global max_limb
    assert all(x < limb_bound for x in a) and val(a) < value_bound * R
    max_limb = max(max_limb, max(a))
    return a


def row(v):
    return limbs(v * (1 << 261) % R)


def permute(params, s):
    full, partial, alpha, mds, ark = params
    top = alpha.bit_length() - 1
    for i in range(full + partial):
        is_full = i < full // 2 or i >= full // 2 + partial
        t = [bounded(add(s[k], row(ark[i][k])), 5 << 29, 9) for k in range(3)]
        for k in range(3 if is_full else 1):
            t[k] = normalize(t[k])
        a = list(t)
        for b in range(top - 1, -1, -1):
            for k in range(3 if is_full else 1):
                a[k] = mul(a[k], a[k])
            if (alpha >> b) & 1:
                for k in range(3 if is_full else 1):
                    a[k] = mul(a[k], t[k])
        s = [bounded(add(add(mul(a[0], row(mds[r][0])), mul(a[1], row(mds[r][1]))), mul(a[2], row(mds[r][2]))), 3 << 29, 6)
             for r in range(3)]
    return s


def hash_elements(params, elems, n_out):
    """The kernel's step loop: absorbing blocks of two, squeezing blocks of two, a permutation before every step but the first
    absorbing one.  elems: values < 2^256 (the kernel multiplies whatever it is given; an element >= r is flagged beside that)."""
    s = [limbs(0)] * 3
    in_blocks, out_blocks, out = (len(elems) + 1) // 2, (n_out + 1) // 2, []
    for step in range(in_blocks + out_blocks):
        if step > 0 or in_blocks == 0:
            s = permute(params, s)
        if step < in_blocks:
            s = list(s)
            s[0] = add(s[0], mul(limbs(elems[2 * step]), TO_MONT))
            if 2 * step + 1 < len(elems):
                s[1] = add(s[1], mul(limbs(elems[2 * step + 1]), TO_MONT))
        else:
            j = 2 * (step - in_blocks)
            out.append(val(mul(s[0], ONE)) % R)
            if j + 1 < n_out:
                out.append(val(mul(s[1], ONE)) % R)
    return out


def check(ref, fills=("r-1", "identity", "reference"), shapes=((8, 29), (8, 0), (2, 29), (2, 0)), alphas=(2, 3, 5, 17, 65535)):
    rnd = random.Random(1)
    cases = 0
    for fill in fills:
        for full, partial in (shapes if fill != "reference" else [(8, 29)]):
            for alpha in alphas:
                params = P.adversarial_params(fill, full, partial, alpha, ref)
                for item in ([R - 1, R - 1], [R - 1] * 5, [], [rnd.randrange(R) for _ in range(3)], [(1 << 256) - 1]):
                    assert hash_elements(params, item, 3) == P.hash_elements(params, [e % R for e in item], 3), (fill, full, partial, alpha)
                    cases += 1
    return cases


def main():
    ref = P.load_params(os.path.join(ROOT, "tests", "golden", "poseidon_params.json"))
    cases = check(ref)
    for n in (0, 11, 55, 300):
        data = P.poseidon_input(n, 0)
        assert hash_elements(ref, P.pack_bytes(data), 1)[0] == P.hash_bytes(ref, data)
    print("ok: %d sponges equal the model; largest limb %.3f x 2^29 (bound 5 x 2^29)" % (cases + 4, max_limb / (1 << 29)))


if __name__ == "__main__":
    main()

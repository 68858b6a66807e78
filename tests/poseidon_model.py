"""Big-integer restatement of the reference's Poseidon hash (TEST INFRASTRUCTURE ONLY; lives under tests/ because oracle/ is frozen).

What the reference states: src/hash/mod.rs:30-43 (PoseidonSponge<Fq>::new(&params), absorb(&input), squeeze one element) with the
parameters of src/hash/helpers.rs.  What ark-sponge 0.3.0 and ark-ff 0.3.0 do with that [U]: rate 2, capacity 1;
F::from_str reduces a decimal string mod r; round i adds ark[i], raises all three entries (full rounds: the first and last F / 2)
or state[0] alone (partial rounds) to alpha, then multiplies by mds; the rate section is state[0..2]; bytes are absorbed as
(length as u64 little-endian || input) in chunks of 31 bytes, each a little-endian integer."""
import hashlib
import json

from pyref.bls12_377 import R

RATE = 2


def load_params(path):
    """-> (full_rounds, partial_rounds, alpha, mds 3 x 3, ark (F + P) x 3), every string reduced mod r as F::from_str does."""
    with open(path) as f:
        d = json.load(f)
    return (d["full_rounds"], d["partial_rounds"], d["alpha"], [[int(s) % R for s in row] for row in d["mds"]],
            [[int(s) % R for s in row] for row in d["ark"]])


def permute(params, state):
    full, partial, alpha, mds, ark = params
    for i in range(full + partial):
        state = [(s + k) % R for s, k in zip(state, ark[i])]
        if i < full // 2 or i >= full // 2 + partial:
            state = [pow(s, alpha, R) for s in state]
        else:
            state[0] = pow(state[0], alpha, R)
        state = [sum(m * s for m, s in zip(row, state)) % R for row in mds]
    return state


def pack_bytes(data):
    """Absorb for [u8]: the elements that stand for a byte string."""
    buf = len(data).to_bytes(8, "little") + bytes(data)
    return [int.from_bytes(buf[i:i + 31], "little") for i in range(0, len(buf), 31)]


def hash_elements(params, elems, n_out=1):
    state, idx = [0, 0, 0], 0
    for e in elems:
        if idx == RATE:
            state, idx = permute(params, state), 0
        state[idx] = (state[idx] + e) % R
        idx += 1
    out, idx = [], RATE     # leaving the absorbing mode permutes
    while len(out) < n_out:
        if idx == RATE:
            state, idx = permute(params, state), 0
        out.append(state[idx])
        idx += 1
    return out


def hash_bytes(params, data):
    """poseidon2_hash(input) of the reference."""
    return hash_elements(params, pack_bytes(data), 1)[0]


# ---- how the fixture (tests/golden/gen_golden_poseidon.py) and the tests derive the inputs that are not stored
def poseidon_input(length, i):
    if length == 11 and i == 0:
        return b"Hello World"
    return hashlib.shake_128(b"poseidon fixture input %d %d" % (length, i)).digest(length)


def fr(label):
    return int.from_bytes(hashlib.sha512(label.encode()).digest(), "little") % R


def poseidon_pair(i):
    return [fr("poseidon fixture pair %d left" % i), fr("poseidon fixture pair %d right" % i)]


def adversarial_params(fill, full, partial, alpha, reference):
    n = full + partial
    if fill == "r-1":
        return full, partial, alpha, [[R - 1] * 3 for _ in range(3)], [[R - 1] * 3 for _ in range(n)]
    if fill == "identity":
        return full, partial, alpha, [[int(a == b) for b in range(3)] for a in range(3)], [[0] * 3 for _ in range(n)]
    assert fill == "reference"
    return full, partial, alpha, reference[3], reference[4][:n]

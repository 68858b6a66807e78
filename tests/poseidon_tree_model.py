"""Big-integer model of the Poseidon Merkle tree (TEST INFRASTRUCTURE ONLY), on top of tests/poseidon_model.py.  The tree is the
library's own definition, from the reference's sponge only:
    HL(leaf) = hash_bytes(params, leaf)               the reference's poseidon2_hash: length prefix, 31-byte chunks, one output
    H2(a, b) = hash_elements(params, [a, b], 1)[0]    state (a, b, 0), one permutation, state[0]
A tree is a list of levels, levels[0] the leaf digests, levels[-1] = [root]; the node array of the library is their concatenation.
One permutation costs about 0.6 ms here: trees of up to 256 leaves keep a test within seconds."""
import hashlib

import poseidon_model as P


def HL(params, leaf):
    return P.hash_bytes(params, bytes(leaf))


def H2(params, a, b):
    return P.hash_elements(params, [a, b], 1)[0]


def _up(params, level):
    return [H2(params, level[2 * i], level[2 * i + 1]) for i in range(len(level) // 2)]


def build(params, leaves):
    """leaves: a power of two (>= 2) of byte strings."""
    levels = [[HL(params, leaf) for leaf in leaves]]
    while len(levels[-1]) > 1:
        levels.append(_up(params, levels[-1]))
    return levels


def blank(params, height):
    """Every leaf digest is zero (not the hash of anything); level l + 1 is H2 of two equal nodes of level l."""
    levels, v = [], 0
    for l in range(height):
        levels.append([v] * (1 << (height - 1 - l)))
        v = H2(params, v, v)
    return levels


def update(params, levels, indices, leaves):
    """The updates in order, in place: arkworks' tree.update(i, leaf) once per pair."""
    for i, leaf in zip(indices, leaves):
        levels[0][i] = HL(params, leaf)
        for l in range(1, len(levels)):
            i >>= 1
            levels[l][i] = H2(params, levels[l - 1][2 * i], levels[l - 1][2 * i + 1])
    return levels


def path(levels, index):
    return [levels[l][(index >> l) ^ 1] for l in range(len(levels) - 1)]


def root_of(params, leaf, index, siblings):
    cur = HL(params, leaf)
    for l, s in enumerate(siblings):
        cur = H2(params, s, cur) if (index >> l) & 1 else H2(params, cur, s)
    return cur


def verify(params, root, leaf, index, siblings):
    return index >> len(siblings) == 0 and root_of(params, leaf, index, siblings) == root


def nodes(levels):
    return [v for level in levels for v in level]


def leaf(length, i, tag=0):
    """How the fixture and the tests derive the leaves that are not stored."""
    return hashlib.shake_128(b"poseidon tree leaf %d %d %d" % (length, i, tag)).digest(length)

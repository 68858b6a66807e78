// poseidon_tree_shape.h — the SHAPE of the membership circuit over a Poseidon Merkle tree (simpleworks_amd/workloads.py,
// build_poseidon_membership): how many variables and rows a parameter shape (full rounds, partial rounds, alpha), a tree height and
// a leaf length give, and where each group of witnesses starts.  Plain C++, no GPU headers, no library state: shared by
// host_abi.inc (swm_poseidon_tree_circuit_shape), by poseidon_tree_witness.hip (which lays the witness vector out by these
// offsets) and by tests/native/poseidon_tree_shape_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "poseidon_shape.h"

namespace swm {

// Instance: one, root, the 8 n leaf bits (byte-major, least significant first).
// Witness layout of one path, L = height - 1 levels, C = (3 full + partial) x chain values per permutation:
//   bits      b_0 .. b_{L-1}: bit l of the leaf index                                      L
//   siblings  s_0 .. s_{L-1}                                                               L
//   deltas    d_l = b_l (s_l - cur_l)                                                      L
//   leaf      the bytes-form sponge over the instance bits: P_leaf permutations            P_leaf C
//   levels    level l: one permutation over (cur_l + d_l, s_l - d_l, 0)                    L C
// Rows: a booleanity row per leaf bit, a row per leaf chain value, per level the booleanity of b_l, the row of d_l and C chain
// rows, and the root row.
static constexpr size_t PT_MIN_HEIGHT = 2, PT_MAX_HEIGHT = 31, PT_MAX_LEAF_LEN = 256;

struct PoseidonTreeShape {
    size_t height = 0, leaf_len = 0, levels = 0;
    size_t num_instance = 0, num_witness = 0, num_constraints = 0;
    size_t elems = 0;       // E = ceil((8 + leaf_len) / 31): elements the leaf sponge absorbs
    size_t leaf_perms = 0;  // P_leaf = ceil(E / 2)
    size_t sboxes = 0;      // 3 full + partial
    size_t chain = 0;       // m(alpha)
    size_t perm_values = 0; // C = sboxes x chain
    size_t bits_at = 0, siblings_at = 0, deltas_at = 0, leaf_at = 0, levels_at = 0;  // the five offsets
};

// false: outside the limits (the parameter limits of poseidon_shape, 2 <= height <= 31, 1 <= leaf_len <= 256), or a count that
// does not fit size_t.  The limits are tested one argument at a time before any sum of two of them is formed.
inline bool poseidon_tree_shape(size_t full, size_t partial, uint64_t alpha, size_t height, size_t leaf_len, PoseidonTreeShape* out) {
    if (height < PT_MIN_HEIGHT || height > PT_MAX_HEIGHT) return false;
    if (leaf_len < 1 || leaf_len > PT_MAX_LEAF_LEN) return false;
    PoseidonShape leaf;  // the leaf sponge is the bytes form of the hash circuit: its limits on the parameters are this circuit's
    if (!poseidon_shape(full, partial, alpha, true, leaf_len, 1, &leaf)) return false;
    PoseidonTreeShape s;
    s.height = height;
    s.leaf_len = leaf_len;
    s.levels = height - 1;
    s.elems = leaf.elems;
    s.leaf_perms = leaf.perms;
    s.sboxes = leaf.sboxes;
    s.chain = leaf.chain;
    if (!pc_mul(s.sboxes, s.chain, &s.perm_values)) return false;
    size_t perms = 0, values = 0, rows = 0;
    if (!pc_add(s.leaf_perms, s.levels, &perms) || !pc_mul(perms, s.perm_values, &values)) return false;
    s.bits_at = 0;
    s.siblings_at = s.levels;
    s.deltas_at = 2 * s.levels;
    s.leaf_at = 3 * s.levels;
    if (!pc_mul(s.leaf_perms, s.perm_values, &s.levels_at) || !pc_add(s.levels_at, s.leaf_at, &s.levels_at)) return false;
    s.num_instance = 2 + 8 * leaf_len;
    if (!pc_add(3 * s.levels, values, &s.num_witness)) return false;
    if (!pc_add(8 * leaf_len + 2 * s.levels + 1, values, &rows)) return false;
    s.num_constraints = rows;
    size_t item_bytes = 0;  // a witness vector is addressed in bytes
    if (!pc_mul(s.num_witness, 32, &item_bytes)) return false;
    *out = s;
    return true;
}

}  // namespace swm

// account_update_shape.h — the SHAPE of the account-update circuit (simpleworks_amd/workloads.py, build_account_update):
// State::register and State::update_balance of examples/simple-payments as one statement over a Poseidon account tree: "the leaf
// at `id` becomes key || new_balance, every other leaf stays".  Composed from poseidon_tree_shape.h (leaves of 72 bytes).  Plain
// C++, no GPU headers, no library state: shared by host_abi.inc (swm_account_update_circuit_shape), by account_update_witness.hip
// (which lays the witness vector out by these offsets) and by tests/native/account_update_shape_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "payment_shape.h"

namespace swm {

// Instance: one, old_root, new_root, id, key_x, key_y, old_balance, new_balance, fresh.
// Witness layout of one update, L, C and M = 3 L + (2 + L) C as in payment_shape.h, U = M - 2 L:
//   key bits     x then y, least significant first                                                       512
//   old balance  64 bits                                                                                 64
//   new balance  64 bits                                                                                 64
//   id bits                                                                                              8
//   cur_0        (1 - fresh) h: the old leaf's level-0 node, the zero digest for a blank leaf            1
//   old          the membership block against old_root: b_l | s_l | d_l | the leaf chain of h = HL(key || old_balance) | the
//                levels, walked from cur_0                                                               M
//   new          the update block over key || new_balance on the same b_l and s_l (deltas | leaf chain | levels), root row
//                against new_root                                                                        U
// The key is packed unreduced, with no strict-canonical check (the caveat of the Schnorr block's `dec` bits): the entry points
// refuse to register a coordinate >= r.
static constexpr size_t AU_INSTANCE = 9;
static constexpr size_t AU_KEY_BITS = 512;
static constexpr size_t AU_BOOLEANS = AU_KEY_BITS + 2 * PY_AMOUNT_BITS + PY_ID_BITS;  // 648
static constexpr size_t AU_BIT_WITNESSES = AU_BOOLEANS + 1;                             // with cur_0

struct AccountUpdateShape {
    size_t height = 0, levels = 0;
    size_t num_instance = 0, num_witness = 0, num_constraints = 0;
    size_t key_bits_at = 0, old_balance_at = 0, new_balance_at = 0, id_bits_at = 0, cur0_at = 0, old_at = 0, new_at = 0;
    size_t membership_witnesses = 0, update_witnesses = 0;                  // M, U
    size_t update_deltas_at = 0, update_leaf_at = 0, update_levels_at = 0;  // relative to the update block
    // named rows
    size_t pack_rows = 0, fresh_row = 0, fresh_balance_row = 0, old_rows = 0, mask_row = 0, old_root_row = 0, new_rows = 0, new_root_row = 0;
    PoseidonTreeShape tree;  // the membership block's own shape, offsets relative to old_at
};

// false: outside the limits (the parameter limits of poseidon_shape, 2 <= height <= 9), or a count that does not fit size_t.
inline bool account_update_shape(size_t full, size_t partial, uint64_t alpha, size_t height, AccountUpdateShape* out) {
    if (height < PY_MIN_HEIGHT || height > PY_MAX_HEIGHT) return false;
    AccountUpdateShape s;
    if (!poseidon_tree_shape(full, partial, alpha, height, PY_LEAF_LEN, &s.tree)) return false;
    const PoseidonTreeShape& t = s.tree;
    s.height = height;
    s.levels = height - 1;
    s.num_instance = AU_INSTANCE;
    s.membership_witnesses = t.num_witness;
    s.update_witnesses = t.num_witness - 2 * s.levels;
    s.update_deltas_at = 0;
    s.update_leaf_at = s.levels;
    s.update_levels_at = t.levels_at - 2 * s.levels;
    s.key_bits_at = 0;
    s.old_balance_at = AU_KEY_BITS;
    s.new_balance_at = s.old_balance_at + PY_AMOUNT_BITS;
    s.id_bits_at = s.new_balance_at + PY_AMOUNT_BITS;
    s.cur0_at = AU_BOOLEANS;
    s.old_at = AU_BIT_WITNESSES;
    if (!pc_add(s.old_at, s.membership_witnesses, &s.new_at)) return false;
    if (!pc_add(s.new_at, s.update_witnesses, &s.num_witness)) return false;
    // the membership block's rows after its index rows: the leaf chain, then per level booleanity, the delta row and the chain
    size_t leaf_rows = 0, level_rows = 0, update_level_rows = 0;
    if (!pc_mul(t.leaf_perms, t.perm_values, &leaf_rows)) return false;
    if (!pc_add(t.perm_values, 2, &level_rows) || !pc_mul(level_rows, s.levels, &level_rows)) return false;
    if (!pc_add(t.perm_values, 1, &update_level_rows) || !pc_mul(update_level_rows, s.levels, &update_level_rows)) return false;
    s.pack_rows = AU_BOOLEANS;
    s.fresh_row = s.pack_rows + 5;
    s.fresh_balance_row = s.fresh_row + 1;
    s.old_rows = s.fresh_balance_row + 1;
    if (!pc_add(s.old_rows + PY_ID_BITS, leaf_rows, &s.mask_row)) return false;
    if (!pc_add(s.mask_row + 1, level_rows, &s.old_root_row)) return false;
    s.new_rows = s.old_root_row + 1;
    if (!pc_add(s.new_rows, leaf_rows, &s.new_root_row) || !pc_add(s.new_root_row, update_level_rows, &s.new_root_row)) return false;
    if (!pc_add(s.new_root_row, 1, &s.num_constraints)) return false;
    size_t item_bytes = 0;  // a witness vector is addressed in bytes
    if (!pc_mul(s.num_witness, 32, &item_bytes)) return false;
    *out = s;
    return true;
}

}  // namespace swm

// pedersen_account_update_shape.h — the SHAPE of the account-update circuit over a Pedersen account tree
// (simpleworks_amd/workloads.py, build_pedersen_account_update): account_update_shape.h's statement and instance ("the leaf at `id`
// becomes key || new_balance, every other leaf stays") over the sections of pedersen_payment_shape.h and pedersen_transfer_shape.h.
// Plain C++, no GPU headers, no library state: shared by host_abi.inc (swm_pedersen_account_update_circuit_shape), by
// pedersen_account_update_witness.hip (which lays the witness vector out by these offsets) and by
// tests/native/pedersen_account_update_shape_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pedersen_transfer_shape.h"

namespace swm {

// Instance: one, old_root, new_root, id, key_x, key_y, old_balance, new_balance, fresh.
// Witness layout of one update, L = height - 1, M = 3450 + 3581 L, U = 3450 + 3579 L:
//   key bits     x then y, least significant first                                                       512
//   old balance  64 bits                                                                                 64
//   new balance  64 bits                                                                                 64
//   id bits                                                                                              8
//   masked bits  o_i = (1 - fresh) k_i: the old leaf's key bits, all zero for a registration             512
//   old          the membership section over o || old balance bits against old_root                      M
//   new          the update section over key bits || new balance bits on the same dir_l and s_l, its root row against new_root   U
// Over this tree the blank leaf is a member (the hash of 72 zero bytes is the identity's x = 0): no cur_0, no masked digest.
static constexpr size_t PAU_INSTANCE = 9;
static constexpr size_t PAU_KEY_BITS = 512;
static constexpr size_t PAU_BOOLEANS = PAU_KEY_BITS + 2 * PP_AMOUNT_BITS + PP_ID_BITS;  // 648
static constexpr size_t PAU_LOOSE_WITNESSES = PAU_BOOLEANS + PAU_KEY_BITS;              // 1160: with the masked bits

struct PedersenAccountUpdateShape {
    size_t height = 0, levels = 0;
    size_t num_instance = 0, num_witness = 0, num_constraints = 0;
    size_t key_bits_at = 0, old_balance_at = 0, new_balance_at = 0, id_bits_at = 0, masked_bits_at = 0, old_at = 0, new_at = 0;
    size_t membership_witnesses = 0, update_witnesses = 0;  // M, U
    size_t section_rows = 0, update_rows = 0;               // each with its root row
    // named rows
    size_t pack_rows = 0, fresh_row = 0, fresh_balance_row = 0, mask_rows = 0, old_rows = 0, old_root_row = 0, new_rows = 0, new_root_row = 0;
};

// false: 2 <= height <= 9 does not hold
inline bool pedersen_account_update_shape(size_t height, PedersenAccountUpdateShape* out) {
    PedersenTransferShape t;
    if (!pedersen_transfer_shape(height, false, &t)) return false;
    PedersenAccountUpdateShape s;
    s.height = t.height;
    s.levels = t.levels;
    s.num_instance = PAU_INSTANCE;
    s.membership_witnesses = t.membership_witnesses;
    s.update_witnesses = t.update_witnesses;
    s.section_rows = t.section_rows;
    s.update_rows = t.update_rows;
    s.key_bits_at = 0;
    s.old_balance_at = PAU_KEY_BITS;
    s.new_balance_at = s.old_balance_at + PP_AMOUNT_BITS;
    s.id_bits_at = s.new_balance_at + PP_AMOUNT_BITS;
    s.masked_bits_at = PAU_BOOLEANS;
    s.old_at = PAU_LOOSE_WITNESSES;
    s.new_at = s.old_at + s.membership_witnesses;
    s.num_witness = s.new_at + s.update_witnesses;
    // 648 booleanity rows, five packing rows, the two rows of fresh, 512 mask rows, the two sections
    s.pack_rows = PAU_BOOLEANS;
    s.fresh_row = s.pack_rows + 5;
    s.fresh_balance_row = s.fresh_row + 1;
    s.mask_rows = s.fresh_balance_row + 1;
    s.old_rows = s.mask_rows + PAU_KEY_BITS;
    s.old_root_row = s.old_rows + s.section_rows - 1;
    s.new_rows = s.old_root_row + 1;
    s.new_root_row = s.new_rows + s.update_rows - 1;
    s.num_constraints = s.new_root_row + 1;
    *out = s;
    return true;
}

}  // namespace swm

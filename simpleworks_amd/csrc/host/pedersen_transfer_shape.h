// pedersen_transfer_shape.h — the SHAPE of the transfer circuit over a Pedersen account tree (simpleworks_amd/workloads.py,
// build_pedersen_transfer): transfer_shape.h's statement (old_root -> new_root, R1 between them) over the sections of
// pedersen_payment_shape.h.  Plain C++, no GPU headers, no library state: shared by host_abi.inc
// (swm_pedersen_transfer_circuit_shape), by pedersen_transfer_witness.hip (which lays the witness vector out by these offsets; a block
// is cut into chunks by witness_chunks.h) and by tests/native/pedersen_transfer_shape_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pedersen_payment_shape.h"

namespace swm {

// Instance: one, old_root, new_root, sender, recipient, amount.
// Witness layout of one transfer, S and M as in pedersen_payment_shape.h, U = 3450 + 3579 L the witnesses of one update section:
//   schnorr | balance | diff | sender   as in the payment circuit, the sender's section against old_root            S + 128 + M
//   sender update     the debited leaf (Y.x || Y.y || diff): leaf hash (575 x 6) | L update levels                   U
//   r1                the intermediate root                                                                         1
//   recipient bits    the recipient's leaf IN THE TREE OF R1                                                        576
//   recipient         its section against r1                                                                        M
//   sum               64 bits of (rbalance + amount) mod 2^64                                                       64
//   recipient update  the credited leaf (key bits || sum)                                                           U
// An update level is a level of merkle_shape.h walked with the membership section's own dir_l and s_l: no dir and no sibling
// witness (left' | 2 x 256 bits | 511 x 6, every group two elements earlier) and no booleanity row of dir.
static constexpr size_t PT_INSTANCE = 6;
static constexpr size_t PT_UPDATE_LEVEL_WITNESSES = MW_LEVEL_WITNESSES - 2;  // 3579
static constexpr size_t PT_UPDATE_LEVEL_ROWS = MW_LEVEL_ROWS - 1;            // 3587
static constexpr size_t PT_UPDATE_LEVEL_BITS_AT = MW_LEVEL_BITS_AT - 2;      // 1: after left'
static constexpr size_t PT_UPDATE_LEVEL_ADDS_AT = MW_LEVEL_ADDS_AT - 2;      // 513
static constexpr size_t PT_BIT_WITNESSES = 3 * PP_AMOUNT_BITS + PP_LEAF_BITS + 1;  // 769: balance, diff, sum, recipient bits, r1

struct PedersenTransferShape {
    size_t height = 0, levels = 0;
    bool salted = false;
    size_t num_instance = 0, num_witness = 0, num_constraints = 0;
    size_t balance_at = 0, diff_at = 0, sender_at = 0, sender_update_at = 0, r1_at = 0, recipient_bits_at = 0, recipient_at = 0, sum_at = 0,
           recipient_update_at = 0;
    size_t membership_witnesses = 0, update_witnesses = 0;  // M, U
    size_t section_rows = 0, update_rows = 0;               // each with its root row
    // named rows
    size_t pack_row = 0, sender_root_row = 0, sender_r1_row = 0, recipient_r1_row = 0, sum_pack_row = 0, new_root_row = 0;
    PedersenPaymentShape payment;  // the Schnorr block and the sections' own shape
    // inside an update section: the leaf hash at 0, level l at update_levels_at + PT_UPDATE_LEVEL_WITNESSES l
    static constexpr size_t update_levels_at = PP_LEAF_WITNESSES;
};

// false: what pedersen_payment_shape refuses (2 <= height <= 9 does not hold)
inline bool pedersen_transfer_shape(size_t height, bool salted, PedersenTransferShape* out) {
    PedersenTransferShape s;
    if (!pedersen_payment_shape(height, salted, &s.payment)) return false;
    const PedersenPaymentShape& p = s.payment;
    s.height = p.height;
    s.levels = p.levels;
    s.salted = salted;
    s.num_instance = PT_INSTANCE;
    s.membership_witnesses = p.membership_witnesses;
    s.update_witnesses = PP_LEAF_WITNESSES + PT_UPDATE_LEVEL_WITNESSES * s.levels;
    s.section_rows = p.section_rows;
    s.update_rows = PP_LEAF_WITNESSES + PT_UPDATE_LEVEL_ROWS * s.levels + 1;
    s.balance_at = p.balance_at;
    s.diff_at = p.diff_at;
    s.sender_at = p.sender_at;
    s.sender_update_at = s.sender_at + s.membership_witnesses;
    s.r1_at = s.sender_update_at + s.update_witnesses;
    s.recipient_bits_at = s.r1_at + 1;
    s.recipient_at = s.recipient_bits_at + PP_LEAF_BITS;
    s.sum_at = s.recipient_at + s.membership_witnesses;
    s.recipient_update_at = s.sum_at + PP_AMOUNT_BITS;
    s.num_witness = s.recipient_update_at + s.update_witnesses;
    // booleanity of balance and diff, the packing row, three tie rows, the sender's section | its update | booleanity of the
    // recipient's bits, its section | booleanity of sum, the sum row | its update
    s.pack_row = p.schnorr.num_constraints + 2 * PP_AMOUNT_BITS;
    s.sender_root_row = s.pack_row + 1 + 3 + s.section_rows - 1;
    s.sender_r1_row = s.sender_root_row + s.update_rows;
    s.recipient_r1_row = s.sender_r1_row + PP_LEAF_BITS + s.section_rows;
    s.sum_pack_row = s.recipient_r1_row + PP_AMOUNT_BITS + 1;
    s.new_root_row = s.sum_pack_row + s.update_rows;
    s.num_constraints = s.new_root_row + 1;
    *out = s;
    return true;
}

}  // namespace swm

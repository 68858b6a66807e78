// transfer_shape.h — the SHAPE of the transfer circuit (simpleworks_amd/workloads.py, build_transfer): State::apply_transaction of
// examples/simple-payments read sequentially as one statement over a Poseidon account tree.  Composed from payment_shape.h: the
// payment circuit up to and with the sender's membership block, then the update blocks.  Plain C++, no GPU headers, no library
// state: shared by host_abi.inc (swm_transfer_circuit_shape), by transfer_witness.hip (which lays the witness vector out by these
// offsets) and by tests/native/transfer_shape_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "payment_shape.h"

namespace swm {

// Instance: one, old_root, new_root, sender, recipient, amount.
// Witness layout of one transfer, S and M as in payment_shape.h, U = M - 2 L the witnesses of one update block (deltas | leaf
// chain | levels: a membership block without bits and siblings of its own):
//   schnorr | balance | diff | sender      as in the payment circuit, the sender's block against old_root      S + 128 + M
//   sender update     the debited leaf (Y.x || Y.y || diff) walked with the sender block's b_l and s_l          U
//   r1                the intermediate root                                                                    1
//   recipient bits    the recipient's leaf IN THE TREE OF R1                                                   576
//   recipient         its membership block against r1                                                          M
//   sum               64 bits of (rbalance + amount) mod 2^64                                                  64
//   recipient update  the credited leaf (key bits || sum) walked with the recipient block's b_l and s_l         U
static constexpr size_t TR_INSTANCE = 6;
static constexpr size_t TR_BIT_WITNESSES = 3 * PY_AMOUNT_BITS + 8 * PY_LEAF_LEN + 1;  // 769: balance, diff, sum, recipient bits, r1

struct TransferShape {
    size_t height = 0, levels = 0;
    bool salted = false;
    size_t num_instance = 0, num_witness = 0, num_constraints = 0;
    size_t balance_at = 0, diff_at = 0, sender_at = 0, sender_update_at = 0, r1_at = 0, recipient_bits_at = 0, recipient_at = 0, sum_at = 0,
           recipient_update_at = 0;
    size_t membership_witnesses = 0, update_witnesses = 0;            // M, U
    size_t update_deltas_at = 0, update_leaf_at = 0, update_levels_at = 0;  // relative to an update block
    PaymentShape payment;  // schnorr and tree: the two blocks' own shapes
};

// false: outside payment_shape's limits, or a count that does not fit size_t.
inline bool transfer_shape(size_t full, size_t partial, uint64_t alpha, size_t height, bool salted, TransferShape* out) {
    TransferShape s;
    if (!payment_shape(full, partial, alpha, height, salted, &s.payment)) return false;
    const PaymentShape& p = s.payment;
    s.height = p.height;
    s.levels = p.levels;
    s.salted = salted;
    s.num_instance = TR_INSTANCE;
    s.membership_witnesses = p.membership_witnesses;
    s.update_witnesses = p.membership_witnesses - 2 * p.levels;
    s.update_deltas_at = 0;
    s.update_leaf_at = p.levels;
    s.update_levels_at = p.tree.levels_at - 2 * p.levels;
    s.balance_at = p.balance_at;
    s.diff_at = p.diff_at;
    s.sender_at = p.sender_at;
    if (!pc_add(s.sender_at, s.membership_witnesses, &s.sender_update_at)) return false;
    if (!pc_add(s.sender_update_at, s.update_witnesses, &s.r1_at)) return false;
    s.recipient_bits_at = s.r1_at + 1;
    if (!pc_add(s.recipient_bits_at, 8 * PY_LEAF_LEN, &s.recipient_at)) return false;
    if (!pc_add(s.recipient_at, s.membership_witnesses, &s.sum_at)) return false;
    if (!pc_add(s.sum_at, PY_AMOUNT_BITS, &s.recipient_update_at)) return false;
    if (!pc_add(s.recipient_update_at, s.update_witnesses, &s.num_witness)) return false;
    // an update block's rows: a membership block's without the eight index rows and the L booleanity rows of b_l
    const size_t block = p.tree.num_constraints - 8 * PY_LEAF_LEN + PY_ID_BITS;
    const size_t update = block - PY_ID_BITS - p.levels;
    size_t rows = 0;  // the payment's rows, booleanity of sum and its packing row, the two update blocks
    if (!pc_add(p.num_constraints, PY_AMOUNT_BITS + 1, &rows)) return false;
    if (!pc_add(rows, update, &rows) || !pc_add(rows, update, &rows)) return false;
    s.num_constraints = rows;
    size_t item_bytes = 0;  // a witness vector is addressed in bytes
    if (!pc_mul(s.num_witness, 32, &item_bytes)) return false;
    *out = s;
    return true;
}

}  // namespace swm

// payment_shape.h — the SHAPE of the payment circuit (simpleworks_amd/workloads.py, build_payment): Transaction::validate of
// examples/simple-payments as one statement over a Poseidon account tree.  Composed from schnorr_shape.h (messages of 10 bytes:
// sender || recipient || amount) and poseidon_tree_shape.h (leaves of 72 bytes: x || y || balance).  Plain C++, no GPU headers, no
// library state: shared by host_abi.inc (swm_payment_circuit_shape), by payment_witness.hip (which lays the witness vector out by
// these offsets) and by tests/native/payment_shape_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "poseidon_tree_shape.h"
#include "schnorr_shape.h"

namespace swm {

// Instance: one, root, sender, recipient, amount.
// Witness layout of one payment, S the Schnorr circuit's witnesses, M = 3 L + (2 + L) C those of one membership block:
//   schnorr         build_schnorr_verification over the 10-byte message, unchanged             S
//   balance         64 bits of the sender's balance                                            64
//   diff            64 bits of (balance - amount) mod 2^64                                     64
//   sender          the membership block of the sender's leaf (bits | siblings | deltas | leaf chain | levels)   M
//   recipient bits  the recipient's leaf, byte-major, least significant first                  576
//   recipient       the membership block of the recipient's leaf                               M
// The sender's leaf bits are no variables of their own: bytes 0 .. 63 are the `dec` bits of Y.x and Y.y, bytes 64 .. 71 the
// balance bits.
static constexpr size_t PY_MSG_LEN = 10, PY_LEAF_LEN = 72, PY_ID_BITS = 8, PY_AMOUNT_BITS = 64;
static constexpr size_t PY_MIN_HEIGHT = 2, PY_MAX_HEIGHT = PY_ID_BITS + 1;  // an id is one byte
static constexpr size_t PY_BIT_WITNESSES = 2 * PY_AMOUNT_BITS + 8 * PY_LEAF_LEN;  // 704: what is neither Schnorr's nor a membership's

struct PaymentShape {
    size_t height = 0, levels = 0;
    bool salted = false;
    size_t num_instance = 0, num_witness = 0, num_constraints = 0;
    size_t balance_at = 0, diff_at = 0, sender_at = 0, recipient_bits_at = 0, recipient_at = 0;
    size_t membership_witnesses = 0;  // M
    SchnorrShape schnorr;             // its offsets are the payment's: the block starts at 0
    PoseidonTreeShape tree;           // offsets relative to sender_at / recipient_at
};

// false: outside the limits (the parameter limits of poseidon_shape, 2 <= height <= 9), or a count that does not fit size_t.
inline bool payment_shape(size_t full, size_t partial, uint64_t alpha, size_t height, bool salted, PaymentShape* out) {
    if (height < PY_MIN_HEIGHT || height > PY_MAX_HEIGHT) return false;
    PaymentShape s;
    if (!schnorr_shape(PY_MSG_LEN, salted, &s.schnorr)) return false;
    if (!poseidon_tree_shape(full, partial, alpha, height, PY_LEAF_LEN, &s.tree)) return false;
    s.height = height;
    s.levels = height - 1;
    s.salted = salted;
    s.membership_witnesses = s.tree.num_witness;
    s.num_instance = 5;
    s.balance_at = s.schnorr.num_witness;
    s.diff_at = s.balance_at + PY_AMOUNT_BITS;
    s.sender_at = s.diff_at + PY_AMOUNT_BITS;
    if (!pc_add(s.sender_at, s.membership_witnesses, &s.recipient_bits_at)) return false;
    if (!pc_add(s.recipient_bits_at, 8 * PY_LEAF_LEN, &s.recipient_at)) return false;
    if (!pc_add(s.recipient_at, s.membership_witnesses, &s.num_witness)) return false;
    // a membership block's rows: eight index rows, then the membership circuit's without the booleanity of its leaf bits
    size_t block = 0, rows = 0;
    if (!pc_add(s.tree.num_constraints - 8 * PY_LEAF_LEN, PY_ID_BITS, &block)) return false;
    // booleanity of balance and diff, the packing row, three tie rows, the recipient's leaf bits
    if (!pc_add(s.schnorr.num_constraints, 2 * PY_AMOUNT_BITS + 1 + 3 + 8 * PY_LEAF_LEN, &rows)) return false;
    if (!pc_add(rows, block, &rows) || !pc_add(rows, block, &rows)) return false;
    s.num_constraints = rows;
    size_t item_bytes = 0;  // a witness vector is addressed in bytes
    if (!pc_mul(s.num_witness, 32, &item_bytes)) return false;
    *out = s;
    return true;
}

}  // namespace swm

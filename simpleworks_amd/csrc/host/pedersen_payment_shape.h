// pedersen_payment_shape.h — the SHAPE of the payment circuit over a Pedersen account tree (simpleworks_amd/workloads.py,
// build_pedersen_payment): Transaction::validate of examples/simple-payments as one statement over the reference's own tree, a
// leaf CRH of 144 windows of 4 bits and a two-to-one CRH of 128.  Composed from schnorr_shape.h (messages of 10 bytes) and the
// level of merkle_shape.h (MW_LEVEL_WITNESSES, MW_LEVEL_ROWS).  Plain C++, no GPU headers, no library state: shared by
// host_abi.inc (swm_pedersen_payment_circuit_shape), by pedersen_payment_witness.hip (which lays the witness vector out by these
// offsets) and by tests/native/pedersen_payment_shape_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "merkle_shape.h"
#include "schnorr_shape.h"

namespace swm {

// Instance: one, root, sender, recipient, amount.
// Witness layout of one payment, S the Schnorr circuit's witnesses, M = 3450 + 3581 L those of one membership section:
//   schnorr         build_schnorr_verification over the 10-byte message, unchanged             S
//   balance         64 bits of the sender's balance                                            64
//   diff            64 bits of (balance - amount) mod 2^64                                     64
//   sender          the sender's section: leaf hash (575 x 6) | L level blocks of merkle_shape.h   M
//   recipient bits  the recipient's leaf, byte-major, least significant first                  576
//   recipient       the recipient's section                                                    M
// The sender's leaf bits are no variables of their own: bytes 0 .. 63 are the `dec` bits of Y.x and Y.y, bytes 64 .. 71 the
// balance bits.  Rows of a section: the leaf hash's 3450, 3588 per level, eight index rows, the root row.
static constexpr size_t PP_MSG_LEN = 10, PP_LEAF_LEN = 72, PP_ID_BITS = 8, PP_AMOUNT_BITS = 64;
static constexpr size_t PP_MIN_HEIGHT = 2, PP_MAX_HEIGHT = PP_ID_BITS + 1;  // an id is one byte
static constexpr size_t PP_LEAF_BITS = 8 * PP_LEAF_LEN;                      // 576 = 144 windows of 4
static constexpr size_t PP_LEAF_WINDOWS = PP_LEAF_BITS / 4, PP_INNER_WINDOWS = 2 * MW_DIGEST_BITS / 4;
static constexpr size_t PP_LEAF_WITNESSES = (PP_LEAF_BITS - 1) * MW_COND_ADD;  // 3450
static constexpr size_t PP_BIT_WITNESSES = 2 * PP_AMOUNT_BITS + PP_LEAF_BITS;  // 704: what is neither Schnorr's nor a section's

struct PedersenPaymentShape {
    size_t height = 0, levels = 0;
    bool salted = false;
    size_t num_instance = 0, num_witness = 0, num_constraints = 0;
    size_t balance_at = 0, diff_at = 0, sender_at = 0, recipient_bits_at = 0, recipient_at = 0;
    size_t membership_witnesses = 0;  // M
    size_t section_rows = 0;
    SchnorrShape schnorr;             // its offsets are the payment's: the block starts at 0
    // inside a section: the leaf hash at 0, level l at levels_at + MW_LEVEL_WITNESSES l
    static constexpr size_t levels_at = PP_LEAF_WITNESSES;
};

// false: 2 <= height <= 9 does not hold
inline bool pedersen_payment_shape(size_t height, bool salted, PedersenPaymentShape* out) {
    if (height < PP_MIN_HEIGHT || height > PP_MAX_HEIGHT) return false;
    PedersenPaymentShape s;
    if (!schnorr_shape(PP_MSG_LEN, salted, &s.schnorr)) return false;
    s.height = height;
    s.levels = height - 1;
    s.salted = salted;
    s.membership_witnesses = PP_LEAF_WITNESSES + MW_LEVEL_WITNESSES * s.levels;
    s.section_rows = PP_LEAF_WITNESSES + MW_LEVEL_ROWS * s.levels + PP_ID_BITS + 1;
    s.num_instance = 5;
    s.balance_at = s.schnorr.num_witness;
    s.diff_at = s.balance_at + PP_AMOUNT_BITS;
    s.sender_at = s.diff_at + PP_AMOUNT_BITS;
    s.recipient_bits_at = s.sender_at + s.membership_witnesses;
    s.recipient_at = s.recipient_bits_at + PP_LEAF_BITS;
    s.num_witness = s.recipient_at + s.membership_witnesses;
    // booleanity of balance and diff, the packing row, three tie rows, the recipient's leaf bits, two sections
    s.num_constraints = s.schnorr.num_constraints + 2 * PP_AMOUNT_BITS + 1 + 3 + PP_LEAF_BITS + 2 * s.section_rows;
    *out = s;
    return true;
}

}  // namespace swm

// elgamal_shape.h — the SHAPE of the ElGamal encryption circuit (simpleworks_amd/workloads.py, build_elgamal_encryption): how
// many variables and rows it has and where each group of witnesses starts.  The circuit has no parameter: one shape.  Plain
// C++, no GPU headers, no library state: shared by host_abi.inc (swm_elgamal_circuit_shape), by elgamal_witness.hip (which lays
// the witness vector out by these offsets) and by tests/native/elgamal_shape_check.cpp.
#pragma once
#include <stddef.h>

namespace swm {

// Witness layout of one encryption (the order in which build_elgamal_encryption calls new_witness_variable); the instance is
// one, pk.x, pk.y, c1.x, c1.y, c2.x, c2.y:
//   key   xx, yy of pk                                          2          rows: x x, y y, on-curve           3
//   msg   m.x, m.y, xx, yy                                      4          the same three rows                3
//   rnd   256 bits of r, least significant first                256        a booleanity row each              256
//   fix   r G: steps 1 .. 255, t, b t, m1, m2, X3, Y3 each      255 x 6    a row per witness
//   dbl   P_{i+1} = 2 P_i, i = 0 .. 254: xy, xx, yy, x', y'     255 x 5    a row per witness
//   sel   Q_i = r_i P_i, i = 0 .. 255: qx, qy                   256 x 2    a row per witness
//   add   acc_i = acc_{i-1} + Q_i, i = 1 .. 255                 255 x 7    a row per witness
//   sum   m + acc_255                                           7          a row per witness
//   out   r G == c1, sum == c2, a row per coordinate            0                                             4
static constexpr size_t EW_SCALAR_BITS = 256;
static constexpr size_t EW_FIX_STEP = 6, EW_DBL_STEP = 5, EW_SEL_STEP = 2, EW_ADD_STEP = 7;
static constexpr size_t EW_KEY_AT = 0, EW_KEY_WITNESSES = 2;
static constexpr size_t EW_MSG_AT = EW_KEY_AT + EW_KEY_WITNESSES, EW_MSG_WITNESSES = 4;
static constexpr size_t EW_RND_AT = EW_MSG_AT + EW_MSG_WITNESSES;
static constexpr size_t EW_FIX_AT = EW_RND_AT + EW_SCALAR_BITS;
static constexpr size_t EW_DBL_AT = EW_FIX_AT + (EW_SCALAR_BITS - 1) * EW_FIX_STEP;
static constexpr size_t EW_SEL_AT = EW_DBL_AT + (EW_SCALAR_BITS - 1) * EW_DBL_STEP;
static constexpr size_t EW_ADD_AT = EW_SEL_AT + EW_SCALAR_BITS * EW_SEL_STEP;
static constexpr size_t EW_SUM_AT = EW_ADD_AT + (EW_SCALAR_BITS - 1) * EW_ADD_STEP;
static constexpr size_t EW_NUM_INSTANCE = 7;
static constexpr size_t EW_NUM_WITNESS = EW_SUM_AT + EW_ADD_STEP;
// the on-curve rows of key and message (3 each); a booleanity row per bit of r; a row per witness of the curve arithmetic; the
// four rows that compare with the claimed ciphertext
static constexpr size_t EW_OUT_ROWS = 4;
static constexpr size_t EW_NUM_CONSTRAINTS = 3 + 3 + EW_SCALAR_BITS + (EW_NUM_WITNESS - EW_FIX_AT) + EW_OUT_ROWS;

struct ElGamalShape {
    size_t num_instance = EW_NUM_INSTANCE, num_witness = EW_NUM_WITNESS, num_constraints = EW_NUM_CONSTRAINTS;
    size_t key_at = EW_KEY_AT, msg_at = EW_MSG_AT, rnd_at = EW_RND_AT, fix_at = EW_FIX_AT, dbl_at = EW_DBL_AT, sel_at = EW_SEL_AT,
           add_at = EW_ADD_AT, sum_at = EW_SUM_AT;
};

inline ElGamalShape elgamal_shape() { return ElGamalShape(); }

}  // namespace swm

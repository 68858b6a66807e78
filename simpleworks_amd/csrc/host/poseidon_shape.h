// poseidon_shape.h — the SHAPE of the Poseidon hash circuit (simpleworks_amd/workloads.py, build_poseidon_hash): how many
// variables and rows a parameter shape (full rounds, partial rounds, alpha), a form (bytes or elements) and the lengths give, and
// where each group of witnesses starts.  Plain C++, no GPU headers, no library state: shared by host_abi.inc
// (swm_poseidon_circuit_shape), by poseidon_witness.hip (which lays the witness vector out by these offsets) and by
// tests/native/poseidon_shape_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace swm {

// Witness layout of one item (the order in which build_poseidon_hash calls new_witness_variable):
//   bits      bytes form: 8 bits per input byte, byte-major, least significant first         8 n_in
//   elements  elements form: the absorbed elements                                           n_in
//   sponge    per permutation, per round, per S-box (3 in a full round, 1 in a partial one) the chain of x^alpha, left to
//             right over the bits of alpha below the top one: a square per bit, a product by x where it is set
//                                                                                            perms x sboxes x chain
// Rows: a booleanity row per bit, a row per chain value, a row per output.
static constexpr size_t PC_MAX_BYTES = 65536, PC_MAX_IN = 4096, PC_MAX_OUT = 16, PC_MAX_ROUNDS = 255;
static constexpr uint64_t PC_MAX_ALPHA = 65535;

struct PoseidonShape {
    bool bytes = false;
    size_t n_in = 0, n_out = 0;  // n_in: the input length in bytes in the bytes form
    size_t num_instance = 0, num_witness = 0, num_constraints = 0;
    size_t elems = 0;       // elements absorbed: ceil((8 + n_in) / 31), or n_in
    size_t perms = 0;       // P: permutations of one sponge
    size_t sboxes = 0;      // S = 3 full + partial: S-boxes per permutation
    size_t chain = 0;       // m(alpha) = floor(log2 alpha) + popcount(alpha) - 1: values per S-box
    size_t input_at = 0;    // the bits, or the elements
    size_t sponge_at = 0;   // the first chain value
};

inline bool pc_mul(size_t a, size_t b, size_t* out) { return !__builtin_mul_overflow(a, b, out); }
inline bool pc_add(size_t a, size_t b, size_t* out) { return !__builtin_add_overflow(a, b, out); }

// false: outside the limits (full rounds even and >= 2, at most PC_MAX_ROUNDS rounds in all, alpha 2 .. PC_MAX_ALPHA, n_in at
// most PC_MAX_BYTES bytes or PC_MAX_IN elements, n_out 1 .. PC_MAX_OUT and 1 in the bytes form), or a count that does not fit
// size_t.  The limits are tested one argument at a time before any sum of two of them is formed.
inline bool poseidon_shape(size_t full, size_t partial, uint64_t alpha, bool bytes, size_t n_in, size_t n_out, PoseidonShape* out) {
    if (full < 2 || (full & 1) || full > PC_MAX_ROUNDS || partial > PC_MAX_ROUNDS || full + partial > PC_MAX_ROUNDS) return false;
    if (alpha < 2 || alpha > PC_MAX_ALPHA) return false;
    if (n_in > (bytes ? PC_MAX_BYTES : PC_MAX_IN) || n_out < 1 || n_out > PC_MAX_OUT || (bytes && n_out != 1)) return false;
    PoseidonShape s;
    s.bytes = bytes;
    s.n_in = n_in;
    s.n_out = n_out;
    s.elems = bytes ? (8 + n_in + 30) / 31 : n_in;
    const size_t in_blocks = (s.elems + 1) / 2, out_blocks = (n_out + 1) / 2;
    s.perms = in_blocks + out_blocks - (in_blocks ? 1 : 0);
    s.sboxes = 3 * full + partial;
    size_t top = 0, ones = 0;
    for (uint64_t a = alpha; a; a >>= 1) {
        top++;
        ones += (size_t)(a & 1);
    }
    s.chain = (top - 1) + ones - 1;
    size_t values = 0, input = 0;
    if (!pc_mul(s.perms, s.sboxes, &values) || !pc_mul(values, s.chain, &values)) return false;
    if (!pc_mul(bytes ? 8 : 1, n_in, &input)) return false;
    s.input_at = 0;
    s.sponge_at = input;
    s.num_instance = 1 + n_out;
    if (!pc_add(input, values, &s.num_witness)) return false;
    if (!pc_add(bytes ? input : 0, values, &s.num_constraints) || !pc_add(s.num_constraints, n_out, &s.num_constraints)) return false;
    size_t item_bytes = 0;  // a witness vector is addressed in bytes
    if (!pc_mul(s.num_witness, 32, &item_bytes)) return false;
    *out = s;
    return true;
}

}  // namespace swm

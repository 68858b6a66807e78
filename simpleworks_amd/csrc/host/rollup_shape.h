// rollup_shape.h — the SHAPE of the rollup circuit (simpleworks_amd/workloads.py, build_rollup / build_pedersen_rollup): N
// sections of one transfer circuit linked through N - 1 witnessed roots, ONE statement old_root -> new_root.  Counts and offsets
// from the transfer shape's (num_witness, num_constraints) and N alone, so the same text serves both account trees.  Plain C++, no
// GPU headers, no library state: shared by host_abi.inc (swm_rollup_circuit_shape, swm_pedersen_rollup_circuit_shape), by
// rollup_witness.hip (which lays the block out as one z by these offsets) and by tests/native/rollup_shape_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace swm {

// Instance: one, old_root, new_root, then sender_k, recipient_k, amount_k for k = 0 .. N - 1.
// Witness: section k at k (W_t + 1): the transfer's W_t witnesses, then for k < N - 1 the root after transfer k (root_{k+1}).
// Rows: section k at k R_t: the transfer's rows with its old_root read as root_k (the instance's for k = 0), its new_root as
// root_{k+1} (the instance's for k = N - 1) and its sender, recipient, amount as those of index k.  No row is added.
static constexpr size_t RU_MIN_TRANSFERS = 1, RU_MAX_TRANSFERS = 64;
static constexpr size_t RU_FIXED_INSTANCE = 3, RU_ITEM_INSTANCE = 3;  // one, old_root, new_root | sender, recipient, amount

struct RollupShape {
    size_t transfers = 0;
    size_t item_witness = 0, item_constraints = 0;  // W_t, R_t
    size_t stride = 0;                              // W_t + 1
    size_t root_at = 0;                             // of a section's trailing root: W_t
    size_t num_instance = 0, num_witness = 0, num_constraints = 0;
    size_t section_at(size_t k) const { return k * stride; }
    size_t section_row(size_t k) const { return k * item_constraints; }
    size_t root_witness(size_t k) const { return (k - 1) * stride + root_at; }  // root_k, 1 <= k <= N - 1
    size_t item_instance(size_t k) const { return RU_FIXED_INSTANCE + RU_ITEM_INSTANCE * k; }
};

// false: N outside 1 .. 64, an empty transfer shape, or a count (the witness vector's bytes among them) that does not fit size_t.
inline bool rollup_shape(size_t item_witness, size_t item_constraints, size_t n, RollupShape* out) {
    if (n < RU_MIN_TRANSFERS || n > RU_MAX_TRANSFERS || item_witness == 0 || item_constraints == 0) return false;
    RollupShape s;
    s.transfers = n;
    s.item_witness = item_witness;
    s.item_constraints = item_constraints;
    s.root_at = item_witness;
    if (__builtin_add_overflow(item_witness, (size_t)1, &s.stride)) return false;
    size_t total = 0, bytes = 0;
    if (__builtin_mul_overflow(n, s.stride, &total)) return false;  // N (W_t + 1)
    if (__builtin_mul_overflow(total, (size_t)32, &bytes)) return false;  // a witness vector is addressed in bytes
    s.num_witness = total - 1;
    if (__builtin_mul_overflow(n, item_constraints, &s.num_constraints)) return false;
    s.num_instance = RU_FIXED_INSTANCE + RU_ITEM_INSTANCE * n;
    *out = s;
    return true;
}

}  // namespace swm

// merkle_shape.h — the SHAPE of the Pedersen Merkle-membership circuit (simpleworks_amd/workloads.py, build_merkle_membership
// with digest_bits = 256): how many variables and rows a tree height and a byte-operation count give, where each group of
// witnesses starts, and the index schedule of the byte-operation block.  Host only, no GPU, no library state: shared by
// host_abi.inc (swm_merkle_circuit_shape) and merkle_witness.hip (which lays the witness vector out by these offsets).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace swm {

// Witness layout of one path (the order in which build_merkle_membership calls new_witness_variable):
//   [0, 42)                          leaf hash: bits 1..7 of the leaf byte, six witnesses per conditional addition
//   42 + 3581 lvl, per level:        dir | sibling | left | 256 bits of left | 256 bits of right | 511 x 6 (bits 1..511)
//   42 + 3581 L .. + 8 ops           the result bits of the byte operations
static constexpr size_t MW_COND_ADD = 6;       // t, b t, m1, m2, X3, Y3
static constexpr size_t MW_LEAF_BITS = 8;
static constexpr size_t MW_DIGEST_BITS = 256;
static constexpr size_t MW_LEAF_WITNESSES = (MW_LEAF_BITS - 1) * MW_COND_ADD;                                   // 42
static constexpr size_t MW_LEVEL_BITS_AT = 3;                                                                    // after dir, sibling, left
static constexpr size_t MW_LEVEL_ADDS_AT = MW_LEVEL_BITS_AT + 2 * MW_DIGEST_BITS;                                // 515
static constexpr size_t MW_LEVEL_WITNESSES = MW_LEVEL_ADDS_AT + (2 * MW_DIGEST_BITS - 1) * MW_COND_ADD;          // 3581
// rows per level: dir booleanity, the select, per child 256 booleanity rows + the packing row + 3 canonical-range rows (bits
// 253..255), 511 x 6 rows of the conditional additions
static constexpr size_t MW_LEVEL_ROWS = 2 + 2 * (MW_DIGEST_BITS + 1 + 3) + (2 * MW_DIGEST_BITS - 1) * MW_COND_ADD;  // 3588
static constexpr size_t MW_NUM_INSTANCE = 1 + 1 + MW_LEAF_BITS;                                                  // one, root, 8 leaf bits
static constexpr size_t MW_MAX_HEIGHT = 64;          // the leaf index is a uint64_t
static constexpr size_t MW_MAX_POOL = 32768;         // bytes of the operation pool (64 per level + one per operation) held in LDS

struct MerkleShape {
    size_t levels = 0, ops = 0;
    size_t num_instance = 0, num_witness = 0, num_constraints = 0;
    size_t ops_at = 0;  // first witness of the byte-operation block
};

// false: height < 2, height > MW_MAX_HEIGHT, or a count that does not fit size_t arithmetic
inline bool merkle_shape(size_t height, size_t ops, MerkleShape* out) {
    if (height < 2 || height > MW_MAX_HEIGHT || ops > ((size_t)1 << 40)) return false;
    MerkleShape s;
    s.levels = height - 1;
    s.ops = ops;
    s.num_instance = MW_NUM_INSTANCE;
    s.ops_at = MW_LEAF_WITNESSES + MW_LEVEL_WITNESSES * s.levels;
    s.num_witness = s.ops_at + 8 * ops;
    // 8 booleanity rows of the public leaf bits, 42 rows of the leaf hash, the levels, the root row; an operation is 8 rows,
    // a shift (every third operation, starting with operation 0) 8 booleanity rows more
    s.num_constraints = MW_LEAF_BITS + MW_LEAF_WITNESSES + MW_LEVEL_ROWS * s.levels + 1 + 8 * ops + 8 * ((ops + 2) / 3);
    *out = s;
    return true;
}

// One byte operation: pool[pool_len_before + op] = f(pool[a], pool[b]); kind 0: a << shift, 1: a ^ b, 2: a & b
struct MerkleByteOp {
    uint16_t a, b;
    uint8_t kind, shift;
    uint16_t pad;
};
static_assert(sizeof(MerkleByteOp) == 8, "one 8-byte load per operation");

// The schedule depends on (levels, ops) only.  false: the pool does not fit MW_MAX_POOL bytes.
inline bool merkle_op_table(size_t levels, size_t ops, std::vector<MerkleByteOp>* out) {
    out->clear();
    const size_t base = 64 * levels;  // per level: the 32 bytes of left, then the 32 bytes of right
    if (base + ops > MW_MAX_POOL) return false;
    out->reserve(ops);
    for (size_t op = 0; op < ops; op++) {
        const size_t len = base + op;
        MerkleByteOp e;
        e.a = (uint16_t)((7 * op) % len);
        e.b = (uint16_t)((11 * op + 3) % len);
        e.kind = (uint8_t)(op % 3);
        e.shift = (uint8_t)(1 + op % 7);
        e.pad = 0;
        out->push_back(e);
    }
    return true;
}

}  // namespace swm

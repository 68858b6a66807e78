// merkle_shape_check.cpp — csrc/host/merkle_shape.h under -fsanitize=address,undefined (tests/test_merkle_witness_host.py): the
// shape arithmetic and the byte-operation schedule that csrc/merkle_witness.hip uploads and indexes LDS with.  Stand-alone: no
// GPU, no library.  Checks for every (height, ops) of a grid that the schedule's indices stay inside the pool as it grows, that
// the kinds and shifts are the builder's, and that the refusals are refusals.  Prints "ok <schedules> <entries>".
#include <stdio.h>
#include <stdlib.h>

#include "host/merkle_shape.h"

using namespace swm;

static void fail(const char* what, size_t height, size_t ops) {
    fprintf(stderr, "merkle_shape_check: %s (height %zu, ops %zu)\n", what, height, ops);
    exit(1);
}

int main() {
    size_t schedules = 0, entries = 0;
    MerkleShape s;
    const size_t bad_heights[] = {0, 1, MW_MAX_HEIGHT + 1, (size_t)1 << 40, ~(size_t)0};
    for (size_t h : bad_heights)
        if (merkle_shape(h, 0, &s)) fail("height accepted", h, 0);
    if (merkle_shape(5, ~(size_t)0, &s)) fail("operation count accepted", 5, ~(size_t)0);
    const size_t op_counts[] = {0, 1, 2, 3, 16, 127, 128, 129, 2400, 5000};
    for (size_t height = 2; height <= MW_MAX_HEIGHT; height++)
        for (size_t ops : op_counts) {
            if (!merkle_shape(height, ops, &s)) fail("shape refused", height, ops);
            if (s.levels != height - 1 || s.num_instance != 10 || s.num_witness != 42 + 3581 * s.levels + 8 * ops ||
                s.ops_at + 8 * ops != s.num_witness)
                fail("witness count", height, ops);
            size_t rows = 51 + 3588 * s.levels;
            for (size_t op = 0; op < ops; op++) rows += op % 3 == 0 ? 16 : 8;
            if (rows != s.num_constraints) fail("row count", height, ops);
            std::vector<MerkleByteOp> t;
            const bool fits = 64 * s.levels + ops <= MW_MAX_POOL;
            if (merkle_op_table(s.levels, ops, &t) != fits) fail("pool bound", height, ops);
            if (!fits) continue;
            if (t.size() != ops) fail("schedule length", height, ops);
            for (size_t op = 0; op < ops; op++) {
                const size_t len = 64 * s.levels + op;
                if (t[op].a != (7 * op) % len || t[op].b != (11 * op + 3) % len || t[op].a >= len || t[op].b >= len)
                    fail("operand index", height, ops);
                if (t[op].kind != op % 3 || t[op].shift != 1 + op % 7 || t[op].shift > 7) fail("kind / shift", height, ops);
            }
            schedules++;
            entries += ops;
        }
    std::vector<MerkleByteOp> t;
    if (merkle_op_table(1, MW_MAX_POOL, &t) || !t.empty()) fail("oversized pool accepted", 2, MW_MAX_POOL);
    if (!merkle_op_table(1, MW_MAX_POOL - 64, &t) || t.size() != MW_MAX_POOL - 64) fail("largest pool refused", 2, MW_MAX_POOL - 64);
    printf("ok %zu %zu\n", schedules, entries);
    return 0;
}

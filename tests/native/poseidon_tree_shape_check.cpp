// poseidon_tree_shape_check.cpp — csrc/host/poseidon_tree_shape.h against a brute-force count of what build_poseidon_membership
// allocates and emits, built with -fsanitize=address,undefined by tests/test_poseidon_tree_host.py.  Prints "ok <cases checked>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "host/poseidon_tree_shape.h"

using namespace swm;

static size_t checked = 0;

static void fail(const char* what, size_t a, size_t b, size_t c, size_t d, size_t e) {
    fprintf(stderr, "FAIL %s: full %zu partial %zu alpha %zu height %zu leaf_len %zu\n", what, a, b, c, d, e);
    exit(1);
}

// Walks the builder one witness at a time and marks every witness it allocates in `seen`, at the offset the header states.
static void walk(size_t full, size_t partial, uint64_t alpha, size_t height, size_t leaf_len) {
    PoseidonTreeShape s;
    if (!poseidon_tree_shape(full, partial, alpha, height, leaf_len, &s)) fail("refused", full, partial, (size_t)alpha, height, leaf_len);
    const size_t levels = height - 1;
    std::vector<unsigned char> seen(s.num_witness, 0);
    auto mark = [&](size_t at) {
        if (at >= seen.size()) fail("witness out of range", full, partial, (size_t)alpha, height, leaf_len);
        seen[at]++;
    };
    size_t rows = 0;
    for (size_t l = 0; l < levels; l++) {
        mark(s.bits_at + l);
        mark(s.siblings_at + l);
        mark(s.deltas_at + l);
    }
    rows += 8 * leaf_len;  // booleanity of the leaf bits
    // one permutation: a witness and a row per square and product, from `at` on; returns the first offset after it
    auto permute = [&](size_t at) {
        for (size_t round = 0; round < full + partial; round++) {
            const bool is_full = round < full / 2 || round >= full / 2 + partial;
            for (size_t k = 0; k < (is_full ? 3u : 1u); k++) {
                int top = 63;
                while (!((alpha >> top) & 1)) top--;
                for (int b = top - 1; b >= 0; b--)
                    for (int mul = 0; mul < (((alpha >> b) & 1) ? 2 : 1); mul++) {
                        mark(at++);
                        rows++;
                    }
            }
        }
        return at;
    };
    // the leaf sponge: the chunks of (8 length bytes || leaf), one byte at a time; a permutation before an element that finds the
    // rate full, and one before the output
    size_t elems = 0, in_chunk = 0, idx = 0, at = s.leaf_at, perms = 0;
    for (size_t pos = 0; pos < 8 + leaf_len; pos++) {
        if (in_chunk == 0) elems++;
        in_chunk = in_chunk + 1 == 31 ? 0 : in_chunk + 1;
    }
    for (size_t e = 0; e < elems; e++) {
        if (idx == 2) {
            at = permute(at);
            perms++;
            idx = 0;
        }
        idx++;
    }
    at = permute(at);
    perms++;
    if (at != s.levels_at || perms != s.leaf_perms || elems != s.elems) fail("leaf sponge", full, partial, (size_t)alpha, height, leaf_len);
    for (size_t l = 0; l < levels; l++) {
        rows += 2;  // booleanity of b_l, the row of d_l
        if (at != s.levels_at + l * s.perm_values) fail("level offset", full, partial, (size_t)alpha, height, leaf_len);
        at = permute(at);
    }
    rows++;  // the root
    if (at != s.num_witness || rows != s.num_constraints || s.num_instance != 2 + 8 * leaf_len)
        fail("counts", full, partial, (size_t)alpha, height, leaf_len);
    if (s.bits_at != 0 || s.siblings_at != levels || s.deltas_at != 2 * levels || s.leaf_at != 3 * levels || s.levels != levels)
        fail("offsets", full, partial, (size_t)alpha, height, leaf_len);
    for (size_t i = 0; i < seen.size(); i++)
        if (seen[i] != 1) fail("a witness not written exactly once", full, partial, (size_t)alpha, height, leaf_len);
    checked++;
}

static void refused(size_t full, size_t partial, uint64_t alpha, size_t height, size_t leaf_len) {
    PoseidonTreeShape s;
    s.num_witness = 12345;
    if (poseidon_tree_shape(full, partial, alpha, height, leaf_len, &s) || s.num_witness != 12345)
        fail("accepted, or wrote on refusal", full, partial, (size_t)alpha, height, leaf_len);
    checked++;
}

int main() {
    for (size_t n = 1; n <= PT_MAX_LEAF_LEN; n++) walk(8, 29, 17, n % 30 + 2, n);
    for (size_t h = PT_MIN_HEIGHT; h <= PT_MAX_HEIGHT; h++) {
        walk(8, 29, 17, h, 1);
        walk(8, 29, 17, h, 72);
    }
    const uint64_t alphas[] = {2, 3, 5, 17, 65535};
    const size_t shapes[][2] = {{8, 29}, {8, 0}, {2, 29}, {2, 0}};
    for (uint64_t alpha : alphas)
        for (const auto& sh : shapes) {
            walk(sh[0], sh[1], alpha, 2, 23);
            walk(sh[0], sh[1], alpha, 6, 55);
        }
    // the worked numbers
    PoseidonTreeShape s;
    if (!poseidon_tree_shape(8, 29, 17, 4, 1, &s) || s.num_instance != 10 || s.num_witness != 1069 || s.num_constraints != 1075) fail("1 / 4", 8, 29, 17, 4, 1);
    if (!poseidon_tree_shape(8, 29, 17, 19, 72, &s) || s.num_instance != 578 || s.num_witness != 5354 || s.num_constraints != 5913)
        fail("72 / 19", 8, 29, 17, 19, 72);
    // the largest legal shapes
    walk(8, 247, 65535, PT_MAX_HEIGHT, PT_MAX_LEAF_LEN);
    walk(254, 1, 65535, PT_MAX_HEIGHT, PT_MAX_LEAF_LEN);
    // the limits, one argument at a time
    refused(8, 29, 17, 1, 1);
    refused(8, 29, 17, 0, 1);
    refused(8, 29, 17, PT_MAX_HEIGHT + 1, 1);
    refused(8, 29, 17, 4, 0);
    refused(8, 29, 17, 4, PT_MAX_LEAF_LEN + 1);
    refused(7, 29, 17, 4, 1);
    refused(0, 29, 17, 4, 1);
    refused(8, 248, 17, 4, 1);
    refused(256, 0, 17, 4, 1);
    refused(8, 29, 1, 4, 1);
    refused(8, 29, 0, 4, 1);
    refused(8, 29, 65536, 4, 1);
    // arguments near SIZE_MAX: refused by the limits, before any sum or product of two of them can wrap
    refused(SIZE_MAX, 29, 17, 4, 1);
    refused(SIZE_MAX - 1, 2, 17, 4, 1);
    refused(8, SIZE_MAX, 17, 4, 1);
    refused(8, SIZE_MAX - 7, 17, 4, 1);
    refused(8, 29, UINT64_MAX, 4, 1);
    refused(8, 29, 17, SIZE_MAX, 1);
    refused(8, 29, 17, 4, SIZE_MAX);
    refused(8, 29, 17, 4, SIZE_MAX - 8);
    refused(SIZE_MAX, SIZE_MAX, UINT64_MAX, SIZE_MAX, SIZE_MAX);
    printf("ok %zu\n", checked);
    return 0;
}

// account_update_shape_check.cpp — csrc/host/account_update_shape.h against the membership shape it is composed from, against the
// formulas of build_account_update and against the numbers of workloads.account_update_circuit_layout() handed over on the command
// line, built with -fsanitize=address,undefined by tests/test_account_update_circuit_host.py.  Every witness of an update belongs to
// exactly one group: the groups are marked into one array, which must come out covered once everywhere.  Arguments: groups of 21
// numbers, a height and the 20 layout values in the order of the test's LAYOUT_KEYS, for the reference's parameters (8 + 29 rounds,
// alpha 17).  Prints "ok <cases checked>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "host/account_update_shape.h"

using namespace swm;

static size_t checked = 0;

static void fail(const char* what, size_t a, size_t b, size_t c, size_t d) {
    fprintf(stderr, "FAIL %s: full %zu partial %zu alpha %zu height %zu\n", what, a, b, c, d);
    exit(1);
}

static void walk(size_t full, size_t partial, uint64_t alpha, size_t height) {
    AccountUpdateShape s;
    PoseidonTreeShape pt;
    if (!account_update_shape(full, partial, alpha, height, &s)) fail("refused", full, partial, (size_t)alpha, height);
    if (!poseidon_tree_shape(full, partial, alpha, height, PY_LEAF_LEN, &pt)) fail("the tree's shape", full, partial, (size_t)alpha, height);
    const size_t L = height - 1, C = pt.perm_values, M = 3 * L + (2 + L) * C, U = M - 2 * L;
    if (pt.leaf_perms != 2 || s.membership_witnesses != M || s.update_witnesses != U || U != L + (2 + L) * C || s.tree.num_witness != M)
        fail("block sizes", full, partial, (size_t)alpha, height);
    if (s.num_instance != 9 || s.num_witness != 649 + 2 * M - 2 * L ||
        s.num_constraints != 655 + (8 + 2 * C + 1 + L * (2 + C) + 1) + (2 * C + L * (1 + C) + 1))
        fail("counts", full, partial, (size_t)alpha, height);
    if (s.levels != L || s.height != height || AU_BOOLEANS != 648 || AU_BIT_WITNESSES != 649)
        fail("the head", full, partial, (size_t)alpha, height);
    if (s.update_deltas_at != 0 || s.update_leaf_at != L || s.update_levels_at != L + 2 * C || s.update_levels_at + L * C != U)
        fail("the update block's offsets", full, partial, (size_t)alpha, height);
    std::vector<unsigned char> seen(s.num_witness, 0);
    auto mark = [&](size_t at, size_t n) {
        for (size_t i = 0; i < n; i++) {
            if (at + i >= seen.size()) fail("witness out of range", full, partial, (size_t)alpha, height);
            seen[at + i]++;
        }
    };
    mark(s.key_bits_at, AU_KEY_BITS);
    mark(s.old_balance_at, PY_AMOUNT_BITS);
    mark(s.new_balance_at, PY_AMOUNT_BITS);
    mark(s.id_bits_at, PY_ID_BITS);
    mark(s.cur0_at, 1);
    mark(s.old_at + pt.bits_at, L);
    mark(s.old_at + pt.siblings_at, L);
    mark(s.old_at + pt.deltas_at, L);
    mark(s.old_at + pt.leaf_at, 2 * C);
    mark(s.old_at + pt.levels_at, L * C);
    mark(s.new_at + s.update_deltas_at, L);
    mark(s.new_at + s.update_leaf_at, 2 * C);
    mark(s.new_at + s.update_levels_at, L * C);
    for (size_t i = 0; i < seen.size(); i++)
        if (seen[i] != 1) fail("a witness not covered exactly once", full, partial, (size_t)alpha, height);
    // the rows: 648 booleanity rows, five packing rows, the two rows of fresh, the two blocks
    if (s.pack_rows != 648 || s.fresh_row != 653 || s.fresh_balance_row != 654 || s.old_rows != 655 || s.mask_row != 655 + 8 + 2 * C ||
        s.old_root_row != s.mask_row + 1 + L * (2 + C) || s.new_rows != s.old_root_row + 1 ||
        s.new_root_row != s.new_rows + 2 * C + L * (1 + C) || s.num_constraints != s.new_root_row + 1)
        fail("named rows", full, partial, (size_t)alpha, height);
    checked++;
}

static void refused(size_t full, size_t partial, uint64_t alpha, size_t height) {
    AccountUpdateShape s;
    s.num_witness = 12345;
    if (account_update_shape(full, partial, alpha, height, &s) || s.num_witness != 12345)
        fail("accepted, or wrote on refusal", full, partial, (size_t)alpha, height);
    checked++;
}

// a group of the command line: the header's numbers are the Python layout's
static void against_layout(char** v) {
    const size_t height = strtoull(v[0], nullptr, 10);
    AccountUpdateShape s;
    if (!account_update_shape(8, 29, 17, height, &s)) fail("refused", 8, 29, 17, height);
    const size_t have[20] = {s.num_instance, s.num_witness,       s.num_constraints,  s.key_bits_at,          s.old_balance_at,
                             s.new_balance_at, s.id_bits_at,      s.cur0_at,          s.old_at,               s.new_at,
                             s.membership_witnesses, s.update_witnesses, s.pack_rows, s.fresh_row,            s.fresh_balance_row,
                             s.old_rows,       s.mask_row,        s.old_root_row,     s.new_rows,             s.new_root_row};
    for (int k = 0; k < 20; k++)
        if (have[k] != strtoull(v[1 + k], nullptr, 10)) {
            fprintf(stderr, "FAIL the layout's value %d at height %zu: the header has %zu, the layout %s\n", k, height, have[k], v[1 + k]);
            exit(1);
        }
    checked++;
}

int main(int argc, char** argv) {
    if ((argc - 1) % 21 != 0) {
        fprintf(stderr, "usage: groups of 21 numbers (a height, 20 layout values)\n");
        return 2;
    }
    for (int g = 1; g < argc; g += 21) against_layout(argv + g);
    const uint64_t alphas[] = {2, 3, 5, 17, 65535};
    const size_t shapes[][2] = {{8, 29}, {8, 0}, {2, 29}, {2, 0}, {8, 247}, {254, 1}};
    for (size_t h = PY_MIN_HEIGHT; h <= PY_MAX_HEIGHT; h++)
        for (uint64_t alpha : alphas)
            for (const auto& sh : shapes) walk(sh[0], sh[1], alpha, h);
    // the worked numbers: the reference's parameters at the maximum height
    AccountUpdateShape s;
    if (!account_update_shape(8, 29, 17, 9, &s) || s.num_instance != 9 || s.num_witness != 5981 || s.num_constraints != 5990)
        fail("height 9", 8, 29, 17, 9);
    // the limits, one argument at a time
    refused(8, 29, 17, 1);
    refused(8, 29, 17, 0);
    refused(8, 29, 17, PY_MAX_HEIGHT + 1);
    refused(8, 29, 17, 31);
    refused(7, 29, 17, 4);
    refused(0, 29, 17, 4);
    refused(8, 248, 17, 4);
    refused(256, 0, 17, 4);
    refused(8, 29, 1, 4);
    refused(8, 29, 0, 4);
    refused(8, 29, 65536, 4);
    // arguments near SIZE_MAX: refused by the limits, before any sum or product of two of them can wrap
    refused(SIZE_MAX, 29, 17, 4);
    refused(SIZE_MAX - 1, 2, 17, 4);
    refused(8, SIZE_MAX, 17, 4);
    refused(8, SIZE_MAX - 7, 17, 4);
    refused(8, 29, UINT64_MAX, 4);
    refused(8, 29, 17, SIZE_MAX);
    printf("ok %zu\n", checked);
    return 0;
}

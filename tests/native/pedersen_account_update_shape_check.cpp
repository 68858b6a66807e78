// pedersen_account_update_shape_check.cpp — csrc/host/pedersen_account_update_shape.h against the section shapes it is composed
// from, against the formulas of build_pedersen_account_update and against the numbers of
// workloads.pedersen_account_update_circuit_layout() handed over on the command line, built with -fsanitize=address,undefined by
// tests/test_pedersen_account_update_circuit_host.py.  Every witness of an update belongs to exactly one group: the groups are
// marked into one array, which must come out covered once everywhere.  Arguments: groups of 24 numbers, a height and the 23 layout
// values in the order of the test's LAYOUT_KEYS.  Prints "ok <cases checked>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "host/pedersen_account_update_shape.h"

using namespace swm;

static size_t checked = 0;
static constexpr int LAYOUT_VALUES = 23;

static void fail(const char* what, size_t height) {
    fprintf(stderr, "FAIL %s: height %zu\n", what, height);
    exit(1);
}

static void walk(size_t height) {
    PedersenAccountUpdateShape s;
    PedersenTransferShape t;
    if (!pedersen_account_update_shape(height, &s)) fail("refused", height);
    if (!pedersen_transfer_shape(height, false, &t)) fail("the transfer's shape", height);
    const size_t L = height - 1, M = 3450 + 3581 * L, U = 3450 + 3579 * L;
    if (s.membership_witnesses != M || s.update_witnesses != U || t.membership_witnesses != M || t.update_witnesses != U)
        fail("section sizes", height);
    if (s.section_rows != 3459 + 3588 * L || s.update_rows != 3451 + 3587 * L || s.section_rows != t.section_rows ||
        s.update_rows != t.update_rows)
        fail("section rows", height);
    if (s.num_instance != 9 || s.num_witness != 1160 + M + U || s.num_constraints != 1167 + (3459 + 3588 * L) + (3451 + 3587 * L))
        fail("counts", height);
    if (s.levels != L || s.height != height || PAU_BOOLEANS != 648 || PAU_LOOSE_WITNESSES != 1160) fail("the head", height);
    std::vector<unsigned char> seen(s.num_witness, 0);
    auto mark = [&](size_t at, size_t n) {
        for (size_t i = 0; i < n; i++) {
            if (at + i >= seen.size()) fail("witness out of range", height);
            seen[at + i]++;
        }
    };
    mark(s.key_bits_at, PAU_KEY_BITS);
    mark(s.old_balance_at, PP_AMOUNT_BITS);
    mark(s.new_balance_at, PP_AMOUNT_BITS);
    mark(s.id_bits_at, PP_ID_BITS);
    mark(s.masked_bits_at, PAU_KEY_BITS);
    // the membership section: the leaf hash, then per level dir | sibling | left | 512 bits | 511 x 6
    mark(s.old_at, PP_LEAF_WITNESSES);
    for (size_t l = 0; l < L; l++) {
        const size_t at = s.old_at + PedersenPaymentShape::levels_at + MW_LEVEL_WITNESSES * l;
        mark(at, MW_LEVEL_BITS_AT);
        mark(at + MW_LEVEL_BITS_AT, MW_LEVEL_ADDS_AT - MW_LEVEL_BITS_AT);
        mark(at + MW_LEVEL_ADDS_AT, MW_LEVEL_WITNESSES - MW_LEVEL_ADDS_AT);
    }
    // the update section: the leaf hash, then per level left | 512 bits | 511 x 6
    mark(s.new_at, PP_LEAF_WITNESSES);
    for (size_t l = 0; l < L; l++) {
        const size_t at = s.new_at + PedersenTransferShape::update_levels_at + PT_UPDATE_LEVEL_WITNESSES * l;
        mark(at, PT_UPDATE_LEVEL_BITS_AT);
        mark(at + PT_UPDATE_LEVEL_BITS_AT, PT_UPDATE_LEVEL_ADDS_AT - PT_UPDATE_LEVEL_BITS_AT);
        mark(at + PT_UPDATE_LEVEL_ADDS_AT, PT_UPDATE_LEVEL_WITNESSES - PT_UPDATE_LEVEL_ADDS_AT);
    }
    for (size_t i = 0; i < seen.size(); i++)
        if (seen[i] != 1) fail("a witness not covered exactly once", height);
    // the rows: 648 booleanity rows, five packing rows, the two rows of fresh, 512 mask rows, the two sections
    if (s.pack_rows != 648 || s.fresh_row != 653 || s.fresh_balance_row != 654 || s.mask_rows != 655 || s.old_rows != 1167 ||
        s.old_root_row != s.old_rows + s.section_rows - 1 || s.new_rows != s.old_root_row + 1 ||
        s.new_root_row != s.new_rows + s.update_rows - 1 || s.num_constraints != s.new_root_row + 1)
        fail("named rows", height);
    checked++;
}

static void refused(size_t height) {
    PedersenAccountUpdateShape s;
    s.num_witness = 12345;
    if (pedersen_account_update_shape(height, &s) || s.num_witness != 12345) fail("accepted, or wrote on refusal", height);
    checked++;
}

// a group of the command line: the header's numbers are the Python layout's
static void against_layout(char** v) {
    const size_t height = strtoull(v[0], nullptr, 10);
    PedersenAccountUpdateShape s;
    if (!pedersen_account_update_shape(height, &s)) fail("refused", height);
    const size_t have[LAYOUT_VALUES] = {s.num_instance,   s.num_witness,  s.num_constraints,     s.key_bits_at,      s.old_balance_at,
                                        s.new_balance_at, s.id_bits_at,   s.masked_bits_at,      s.old_at,           s.new_at,
                                        s.membership_witnesses, s.update_witnesses, s.section_rows, s.update_rows,   s.pack_rows,
                                        s.fresh_row,      s.fresh_balance_row, s.mask_rows,      s.old_rows,         s.old_root_row,
                                        s.new_rows,       s.new_root_row, s.levels};
    for (int k = 0; k < LAYOUT_VALUES; k++)
        if (have[k] != strtoull(v[1 + k], nullptr, 10)) {
            fprintf(stderr, "FAIL the layout's value %d at height %zu: the header has %zu, the layout %s\n", k, height, have[k], v[1 + k]);
            exit(1);
        }
    checked++;
}

int main(int argc, char** argv) {
    if ((argc - 1) % (LAYOUT_VALUES + 1) != 0) {
        fprintf(stderr, "usage: groups of %d numbers (a height, %d layout values)\n", LAYOUT_VALUES + 1, LAYOUT_VALUES);
        return 2;
    }
    for (int g = 1; g < argc; g += LAYOUT_VALUES + 1) against_layout(argv + g);
    for (size_t h = PP_MIN_HEIGHT; h <= PP_MAX_HEIGHT; h++) walk(h);
    // the worked numbers at the maximum height: |H| = 2^16 with 59 rows to spare
    PedersenAccountUpdateShape s;
    if (!pedersen_account_update_shape(9, &s) || s.num_instance != 9 || s.num_witness != 65340 || s.num_constraints != 65477 ||
        s.num_constraints > 65536)
        fail("height 9", 9);
    checked++;
    refused(0);
    refused(1);
    refused(PP_MAX_HEIGHT + 1);
    refused(31);
    refused(SIZE_MAX);
    printf("ok %zu\n", checked);
    return 0;
}

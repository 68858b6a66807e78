// transfer_shape_check.cpp — csrc/host/transfer_shape.h against the payment shape it is composed from and against the formulas of
// build_transfer, built with -fsanitize=address,undefined by tests/test_transfer_circuit_host.py.  Every witness of a transfer
// belongs to exactly one group: the groups are marked into one array, which must come out covered once everywhere.  Prints
// "ok <cases checked>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "host/transfer_shape.h"

using namespace swm;

static size_t checked = 0;

static void fail(const char* what, size_t a, size_t b, size_t c, size_t d, size_t e) {
    fprintf(stderr, "FAIL %s: full %zu partial %zu alpha %zu height %zu salted %zu\n", what, a, b, c, d, e);
    exit(1);
}

static void walk(size_t full, size_t partial, uint64_t alpha, size_t height, bool salted) {
    TransferShape s;
    PaymentShape py;
    if (!transfer_shape(full, partial, alpha, height, salted, &s)) fail("refused", full, partial, (size_t)alpha, height, salted);
    if (!payment_shape(full, partial, alpha, height, salted, &py)) fail("the payment's shape", full, partial, (size_t)alpha, height, salted);
    const PoseidonTreeShape& pt = py.tree;
    const size_t L = height - 1, C = pt.perm_values, M = 3 * L + (2 + L) * C, U = M - 2 * L, S = py.schnorr.num_witness;
    if (s.membership_witnesses != M || s.update_witnesses != U || U != L + (2 + L) * C)
        fail("block sizes", full, partial, (size_t)alpha, height, salted);
    if (s.num_instance != 6 || s.num_witness != S + 769 + 4 * M - 4 * L ||
        s.num_constraints != py.schnorr.num_constraints + 773 + 2 * (8 + 2 * C + L * (2 + C) + 1) + 2 * (2 * C + L * (1 + C) + 1))
        fail("counts", full, partial, (size_t)alpha, height, salted);
    if (s.levels != L || s.height != height || s.salted != salted || s.payment.num_witness != py.num_witness ||
        s.balance_at != py.balance_at || s.diff_at != py.diff_at || s.sender_at != py.sender_at)
        fail("the payment's part", full, partial, (size_t)alpha, height, salted);
    if (s.update_deltas_at != 0 || s.update_leaf_at != L || s.update_levels_at != L + 2 * C || s.update_levels_at + L * C != U)
        fail("an update block's offsets", full, partial, (size_t)alpha, height, salted);
    std::vector<unsigned char> seen(s.num_witness, 0);
    auto mark = [&](size_t at, size_t n) {
        for (size_t i = 0; i < n; i++) {
            if (at + i >= seen.size()) fail("witness out of range", full, partial, (size_t)alpha, height, salted);
            seen[at + i]++;
        }
    };
    mark(0, S);
    mark(s.balance_at, PY_AMOUNT_BITS);
    mark(s.diff_at, PY_AMOUNT_BITS);
    for (size_t base : {s.sender_at, s.recipient_at}) {
        mark(base + pt.bits_at, L);
        mark(base + pt.siblings_at, L);
        mark(base + pt.deltas_at, L);
        mark(base + pt.leaf_at, 2 * C);
        mark(base + pt.levels_at, L * C);
    }
    for (size_t base : {s.sender_update_at, s.recipient_update_at}) {
        mark(base + s.update_deltas_at, L);
        mark(base + s.update_leaf_at, 2 * C);
        mark(base + s.update_levels_at, L * C);
    }
    mark(s.r1_at, 1);
    mark(s.recipient_bits_at, 8 * PY_LEAF_LEN);
    mark(s.sum_at, PY_AMOUNT_BITS);
    for (size_t i = 0; i < seen.size(); i++)
        if (seen[i] != 1) fail("a witness not covered exactly once", full, partial, (size_t)alpha, height, salted);
    if (!(s.sender_at < s.sender_update_at && s.sender_update_at < s.r1_at && s.r1_at < s.recipient_bits_at &&
          s.recipient_bits_at < s.recipient_at && s.recipient_at < s.sum_at && s.sum_at < s.recipient_update_at &&
          s.recipient_update_at < s.num_witness))
        fail("order", full, partial, (size_t)alpha, height, salted);
    if (TR_BIT_WITNESSES != 769) fail("bit witnesses", full, partial, (size_t)alpha, height, salted);
    checked++;
}

static void refused(size_t full, size_t partial, uint64_t alpha, size_t height, bool salted) {
    TransferShape s;
    s.num_witness = 12345;
    if (transfer_shape(full, partial, alpha, height, salted, &s) || s.num_witness != 12345)
        fail("accepted, or wrote on refusal", full, partial, (size_t)alpha, height, salted);
    checked++;
}

int main() {
    const uint64_t alphas[] = {2, 3, 5, 17, 65535};
    const size_t shapes[][2] = {{8, 29}, {8, 0}, {2, 29}, {2, 0}, {8, 247}, {254, 1}};
    for (size_t h = PY_MIN_HEIGHT; h <= PY_MAX_HEIGHT; h++)
        for (int salted = 0; salted < 2; salted++)
            for (uint64_t alpha : alphas)
                for (const auto& sh : shapes) walk(sh[0], sh[1], alpha, h, salted != 0);
    // the worked numbers: the reference's parameters at the maximum height
    TransferShape s;
    if (!transfer_shape(8, 29, 17, 9, false, &s) || s.num_instance != 6 || s.num_witness != 82578 || s.num_constraints != 83569)
        fail("height 9", 8, 29, 17, 9, 0);
    // the limits, one argument at a time
    refused(8, 29, 17, 1, false);
    refused(8, 29, 17, 0, false);
    refused(8, 29, 17, PY_MAX_HEIGHT + 1, false);
    refused(8, 29, 17, 31, true);
    refused(7, 29, 17, 4, false);
    refused(0, 29, 17, 4, false);
    refused(8, 248, 17, 4, false);
    refused(256, 0, 17, 4, false);
    refused(8, 29, 1, 4, false);
    refused(8, 29, 0, 4, true);
    refused(8, 29, 65536, 4, false);
    // arguments near SIZE_MAX: refused by the limits, before any sum or product of two of them can wrap
    refused(SIZE_MAX, 29, 17, 4, false);
    refused(SIZE_MAX - 1, 2, 17, 4, false);
    refused(8, SIZE_MAX, 17, 4, false);
    refused(8, SIZE_MAX - 7, 17, 4, true);
    refused(8, 29, UINT64_MAX, 4, false);
    refused(8, 29, 17, SIZE_MAX, false);
    refused(SIZE_MAX, SIZE_MAX, UINT64_MAX, SIZE_MAX, true);
    printf("ok %zu\n", checked);
    return 0;
}

// payment_shape_check.cpp — csrc/host/payment_shape.h against the two shapes it is composed from and against the formulas of
// build_payment, built with -fsanitize=address,undefined by tests/test_payment_circuit_host.py.  Every witness of a payment belongs
// to exactly one group: the groups are marked into one array, which must come out covered once everywhere.  Prints
// "ok <cases checked>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "host/payment_shape.h"

using namespace swm;

static size_t checked = 0;

static void fail(const char* what, size_t a, size_t b, size_t c, size_t d, size_t e) {
    fprintf(stderr, "FAIL %s: full %zu partial %zu alpha %zu height %zu salted %zu\n", what, a, b, c, d, e);
    exit(1);
}

static void walk(size_t full, size_t partial, uint64_t alpha, size_t height, bool salted) {
    PaymentShape s;
    if (!payment_shape(full, partial, alpha, height, salted, &s)) fail("refused", full, partial, (size_t)alpha, height, salted);
    SchnorrShape sv;
    PoseidonTreeShape pt;
    if (!schnorr_shape(PY_MSG_LEN, salted, &sv) || !poseidon_tree_shape(full, partial, alpha, height, PY_LEAF_LEN, &pt))
        fail("a block's shape", full, partial, (size_t)alpha, height, salted);
    const size_t L = height - 1, C = pt.perm_values, M = 3 * L + (2 + L) * C;
    if (pt.leaf_perms != 2 || pt.num_witness != M || s.membership_witnesses != M) fail("membership block", full, partial, (size_t)alpha, height, salted);
    if (s.num_instance != 5 || s.num_witness != sv.num_witness + 704 + 2 * M ||
        s.num_constraints != sv.num_constraints + 708 + 2 * (8 + 2 * C + L * (2 + C) + 1))
        fail("counts", full, partial, (size_t)alpha, height, salted);
    if (s.levels != L || s.height != height || s.salted != salted || s.schnorr.num_witness != sv.num_witness || s.schnorr.dec_at != sv.dec_at ||
        s.tree.levels_at != pt.levels_at || s.tree.leaf_len != PY_LEAF_LEN)
        fail("the blocks' shapes inside", full, partial, (size_t)alpha, height, salted);
    std::vector<unsigned char> seen(s.num_witness, 0);
    auto mark = [&](size_t at, size_t n) {
        for (size_t i = 0; i < n; i++) {
            if (at + i >= seen.size()) fail("witness out of range", full, partial, (size_t)alpha, height, salted);
            seen[at + i]++;
        }
    };
    mark(0, sv.num_witness);
    mark(s.balance_at, PY_AMOUNT_BITS);
    mark(s.diff_at, PY_AMOUNT_BITS);
    for (size_t base : {s.sender_at, s.recipient_at}) {
        mark(base + pt.bits_at, L);
        mark(base + pt.siblings_at, L);
        mark(base + pt.deltas_at, L);
        mark(base + pt.leaf_at, 2 * C);
        mark(base + pt.levels_at, L * C);
    }
    mark(s.recipient_bits_at, 8 * PY_LEAF_LEN);
    for (size_t i = 0; i < seen.size(); i++)
        if (seen[i] != 1) fail("a witness not covered exactly once", full, partial, (size_t)alpha, height, salted);
    if (!(s.balance_at < s.diff_at && s.diff_at < s.sender_at && s.sender_at < s.recipient_bits_at && s.recipient_bits_at < s.recipient_at &&
          s.recipient_at < s.num_witness))
        fail("order", full, partial, (size_t)alpha, height, salted);
    checked++;
}

static void refused(size_t full, size_t partial, uint64_t alpha, size_t height, bool salted) {
    PaymentShape s;
    s.num_witness = 12345;
    if (payment_shape(full, partial, alpha, height, salted, &s) || s.num_witness != 12345)
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
    PaymentShape s;
    if (!payment_shape(8, 29, 17, 9, false, &s) || s.num_instance != 5 || s.num_witness != 77197 || s.num_constraints != 78186)
        fail("height 9", 8, 29, 17, 9, 0);
    if (!payment_shape(8, 29, 17, 4, false, &s) || s.num_witness != 74517 || s.num_constraints != 75516 || s.balance_at != 71145 ||
        s.sender_at != 71273 || s.recipient_bits_at != 72607 || s.recipient_at != 73183)
        fail("height 4", 8, 29, 17, 4, 0);
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

// pedersen_payment_shape_check.cpp — csrc/host/pedersen_payment_shape.h printed for every height and both salt settings, and held
// to a cover of [0, num_witness) by its groups.  Built with -fsanitize=address,undefined and run by
// tests/test_pedersen_payment_circuit_host.py, which compares every printed line with workloads.pedersen_payment_circuit_layout.
// One line per shape: "shape height salted num_instance num_witness num_constraints balance diff sender recipient_bits recipient
// membership_witnesses section_rows"; then "ok <cases checked>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "host/pedersen_payment_shape.h"

using namespace swm;

static size_t checked = 0;

static void fail(const char* what, size_t height, size_t salted) {
    fprintf(stderr, "FAIL %s: height %zu salted %zu\n", what, height, salted);
    exit(1);
}

static void walk(size_t height, bool salted) {
    PedersenPaymentShape s;
    if (!pedersen_payment_shape(height, salted, &s)) fail("refused", height, salted);
    SchnorrShape sv;
    if (!schnorr_shape(PP_MSG_LEN, salted, &sv)) fail("the Schnorr block's shape", height, salted);
    const size_t L = height - 1, M = 3450 + 3581 * L;
    if (s.membership_witnesses != M || s.levels != L || s.height != height || s.salted != salted) fail("section", height, salted);
    if (s.num_instance != 5 || s.num_witness != sv.num_witness + 704 + 2 * M ||
        s.num_constraints != sv.num_constraints + 708 + 2 * (3459 + 3588 * L))
        fail("counts", height, salted);
    std::vector<unsigned char> seen(s.num_witness, 0);
    auto mark = [&](size_t at, size_t n) {
        for (size_t i = 0; i < n; i++) {
            if (at + i >= seen.size()) fail("witness out of range", height, salted);
            seen[at + i]++;
        }
    };
    mark(0, sv.num_witness);
    mark(s.balance_at, PP_AMOUNT_BITS);
    mark(s.diff_at, PP_AMOUNT_BITS);
    for (size_t base : {s.sender_at, s.recipient_at}) {
        mark(base, PP_LEAF_WITNESSES);
        for (size_t l = 0; l < L; l++) {
            const size_t at = base + PedersenPaymentShape::levels_at + MW_LEVEL_WITNESSES * l;
            mark(at, MW_LEVEL_BITS_AT);
            mark(at + MW_LEVEL_BITS_AT, 2 * MW_DIGEST_BITS);
            mark(at + MW_LEVEL_ADDS_AT, (2 * MW_DIGEST_BITS - 1) * MW_COND_ADD);
        }
    }
    mark(s.recipient_bits_at, PP_LEAF_BITS);
    for (size_t i = 0; i < seen.size(); i++)
        if (seen[i] != 1) fail("a witness not covered exactly once", height, salted);
    printf("shape %zu %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", height, salted ? 1 : 0, s.num_instance, s.num_witness, s.num_constraints,
           s.balance_at, s.diff_at, s.sender_at, s.recipient_bits_at, s.recipient_at, s.membership_witnesses, s.section_rows);
    checked++;
}

static void refused(size_t height, bool salted) {
    PedersenPaymentShape s;
    s.num_witness = 12345;
    if (pedersen_payment_shape(height, salted, &s) || s.num_witness != 12345) fail("accepted, or wrote on refusal", height, salted);
    checked++;
}

int main() {
    for (size_t h = PP_MIN_HEIGHT; h <= PP_MAX_HEIGHT; h++)
        for (int salted = 0; salted < 2; salted++) walk(h, salted != 0);
    refused(0, false);
    refused(1, true);
    refused(PP_MAX_HEIGHT + 1, false);
    refused(SIZE_MAX, true);
    printf("ok %zu\n", checked);
    return 0;
}

// rollup_shape_check.cpp — csrc/host/rollup_shape.h against the two transfer shapes it sits on and against the layout contract of
// build_rollup, built with -fsanitize=address,undefined by tests/test_rollup_circuit_host.py.  Every witness of a block belongs to
// exactly one section or is one linking root: both are marked into one array, which must come out covered once everywhere; the
// same for the rows and for the instance.  Prints "ok <cases checked>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "host/pedersen_transfer_shape.h"
#include "host/rollup_shape.h"
#include "host/transfer_shape.h"

using namespace swm;

static size_t checked = 0;

static void fail(const char* what, size_t w, size_t r, size_t n) {
    fprintf(stderr, "FAIL %s: item witnesses %zu rows %zu transfers %zu\n", what, w, r, n);
    exit(1);
}

static void walk(size_t w, size_t r, size_t n) {
    RollupShape s;
    if (!rollup_shape(w, r, n, &s)) fail("refused", w, r, n);
    if (s.transfers != n || s.item_witness != w || s.item_constraints != r || s.stride != w + 1 || s.root_at != w) fail("the item", w, r, n);
    if (s.num_instance != 3 + 3 * n || s.num_witness != n * (w + 1) - 1 || s.num_constraints != n * r) fail("counts", w, r, n);
    std::vector<unsigned char> seen(s.num_witness, 0), rows(s.num_constraints, 0), inst(s.num_instance, 0);
    auto mark = [&](std::vector<unsigned char>& a, size_t at, size_t count, const char* what) {
        for (size_t i = 0; i < count; i++) {
            if (at + i >= a.size()) fail(what, w, r, n);
            a[at + i]++;
        }
    };
    mark(inst, 0, RU_FIXED_INSTANCE, "instance out of range");
    for (size_t k = 0; k < n; k++) {
        mark(seen, s.section_at(k), w, "witness out of range");
        if (k >= 1) {
            mark(seen, s.root_witness(k), 1, "root out of range");
            if (s.root_witness(k) != s.section_at(k) - 1 || s.root_witness(k) != s.section_at(k - 1) + s.root_at) fail("a root's place", w, r, n);
        }
        mark(rows, s.section_row(k), r, "row out of range");
        mark(inst, s.item_instance(k), RU_ITEM_INSTANCE, "instance out of range");
    }
    for (unsigned char c : seen)
        if (c != 1) fail("a witness not covered exactly once", w, r, n);
    for (unsigned char c : rows)
        if (c != 1) fail("a row not covered exactly once", w, r, n);
    for (unsigned char c : inst)
        if (c != 1) fail("an instance variable not covered exactly once", w, r, n);
    checked++;
}

static void refused(size_t w, size_t r, size_t n) {
    RollupShape s;
    s.num_witness = 12345;
    if (rollup_shape(w, r, n, &s) || s.num_witness != 12345) fail("accepted, or wrote on refusal", w, r, n);
    checked++;
}

int main() {
    // over both trees' transfer shapes at every height; the block sizes the documents speak of and the two ends
    const size_t sizes[] = {1, 2, 3, 5, 8, 12, 63, 64};
    for (int salted = 0; salted < 2; salted++) {
        for (size_t h = PY_MIN_HEIGHT; h <= PY_MAX_HEIGHT; h++) {
            TransferShape t;
            if (!transfer_shape(8, 29, 17, h, salted != 0, &t)) fail("the transfer's shape", h, 0, 0);
            for (size_t n : sizes) walk(t.num_witness, t.num_constraints, n);
        }
        for (size_t h = PP_MIN_HEIGHT; h <= PP_MAX_HEIGHT; h++) {
            PedersenTransferShape t;
            if (!pedersen_transfer_shape(h, salted != 0, &t)) fail("the Pedersen transfer's shape", h, 0, 0);
            for (size_t n : sizes) walk(t.num_witness, t.num_constraints, n);
        }
    }
    walk(1, 1, 1);
    walk(1, 1, 64);
    // the worked numbers: eight and twelve transfers at height 9 over the Poseidon tree fit |H| = 2^20, five over the Pedersen tree
    RollupShape s;
    if (!rollup_shape(82578, 83569, 8, &s) || s.num_instance != 27 || s.num_witness != 660631 || s.num_constraints != 668552)
        fail("eight at height 9", 82578, 83569, 8);
    if (s.num_instance + s.num_witness != 660658) fail("eight at height 9: variables", 82578, 83569, 8);
    if (!rollup_shape(82578, 83569, 12, &s) || s.num_constraints > ((size_t)1 << 20) || s.num_instance + s.num_witness > ((size_t)1 << 20))
        fail("twelve at height 9", 82578, 83569, 12);
    if (!rollup_shape(82578, 83569, 13, &s) || s.num_constraints <= ((size_t)1 << 20)) fail("thirteen at height 9", 82578, 83569, 13);
    if (!rollup_shape(200274, 201521, 5, &s) || s.num_constraints > ((size_t)1 << 20)) fail("five over the Pedersen tree", 200274, 201521, 5);
    if (!rollup_shape(200274, 201521, 6, &s) || s.num_constraints <= ((size_t)1 << 20)) fail("six over the Pedersen tree", 200274, 201521, 6);
    // the limits
    refused(82578, 83569, 0);
    refused(82578, 83569, 65);
    refused(82578, 83569, SIZE_MAX);
    refused(0, 83569, 8);
    refused(82578, 0, 8);
    // N (W_t + 1), its bytes, N R_t: refused before they wrap
    refused(SIZE_MAX, 1, 1);
    refused(SIZE_MAX - 1, 1, 2);
    refused(SIZE_MAX / 2, 1, 2);
    refused(SIZE_MAX / 32, 1, 1);
    refused(SIZE_MAX / 64, 1, 2);
    refused(SIZE_MAX / 64, 1, 64);
    refused(1, SIZE_MAX, 2);
    refused(1, SIZE_MAX / 2 + 1, 2);
    refused(1, SIZE_MAX / 64 + 1, 64);
    // the largest counts that fit are taken
    if (!rollup_shape(1, SIZE_MAX / 64, 64, &s) || s.num_constraints != (SIZE_MAX / 64) * 64) fail("the most rows", 1, SIZE_MAX / 64, 64);
    if (!rollup_shape(SIZE_MAX / 32 - 1, 1, 1, &s) || s.num_witness != SIZE_MAX / 32 - 1) fail("the most witnesses", SIZE_MAX / 32 - 1, 1, 1);
    checked += 2;
    printf("ok %zu\n", checked);
    return 0;
}

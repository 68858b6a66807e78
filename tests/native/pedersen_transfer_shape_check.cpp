// pedersen_transfer_shape_check.cpp — csrc/host/pedersen_transfer_shape.h printed for every height and both salt settings, held to
// the formulas and to a cover of [0, num_witness) by its groups, and the chunk planner every circuit unit cuts a batch by
// (csrc/host/witness_chunks.h) on small caps and on the library's own.  Built with
// -fsanitize=address,undefined and run by tests/test_pedersen_transfer_circuit_host.py, which compares every printed line with
// workloads.pedersen_transfer_circuit_layout and with its own plan.
// One line per shape: "shape height salted num_instance num_witness num_constraints balance diff sender sender_update r1
// recipient_bits recipient sum recipient_update membership_witnesses update_witnesses section_rows update_rows pack_row
// sender_root_row sender_r1_row recipient_r1_row sum_pack_row new_root_row"; one line per plan: "plan item_bytes count cap_bytes
// base:count ..."; "stage <WITNESS_STAGE_BYTES>"; then "ok <cases checked>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "host/pedersen_transfer_shape.h"
#include "host/witness_chunks.h"

using namespace swm;

static size_t checked = 0;

static void fail(const char* what, size_t a, size_t b) {
    fprintf(stderr, "FAIL %s: %zu %zu\n", what, a, b);
    exit(1);
}

static void walk(size_t height, bool salted) {
    PedersenTransferShape s;
    if (!pedersen_transfer_shape(height, salted, &s)) fail("refused", height, salted);
    SchnorrShape sv;
    if (!schnorr_shape(PP_MSG_LEN, salted, &sv)) fail("the Schnorr block's shape", height, salted);
    const size_t L = height - 1, M = 3450 + 3581 * L, U = 3450 + 3579 * L;
    if (s.membership_witnesses != M || s.update_witnesses != U || s.levels != L || s.height != height || s.salted != salted)
        fail("sections", height, salted);
    if (s.num_instance != 6 || s.num_witness != sv.num_witness + 769 + 2 * M + 2 * U ||
        s.num_constraints != sv.num_constraints + 773 + 2 * (3459 + 3588 * L) + 2 * (3451 + 3587 * L))
        fail("counts", height, salted);
    if (PT_BIT_WITNESSES != 769 || s.num_witness != sv.num_witness + PT_BIT_WITNESSES + 2 * M + 2 * U) fail("bit witnesses", height, salted);
    // the sender's side is the payment circuit's
    const PedersenPaymentShape& p = s.payment;
    if (s.balance_at != p.balance_at || s.diff_at != p.diff_at || s.sender_at != p.sender_at || s.sender_update_at != p.recipient_bits_at)
        fail("the payment circuit's offsets", height, salted);
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
    mark(s.sum_at, PP_AMOUNT_BITS);
    mark(s.r1_at, 1);
    mark(s.recipient_bits_at, PP_LEAF_BITS);
    for (size_t base : {s.sender_at, s.recipient_at}) {
        mark(base, PP_LEAF_WITNESSES);
        for (size_t l = 0; l < L; l++) {
            const size_t at = base + PedersenPaymentShape::levels_at + MW_LEVEL_WITNESSES * l;
            mark(at, MW_LEVEL_BITS_AT);
            mark(at + MW_LEVEL_BITS_AT, 2 * MW_DIGEST_BITS);
            mark(at + MW_LEVEL_ADDS_AT, (2 * MW_DIGEST_BITS - 1) * MW_COND_ADD);
        }
    }
    for (size_t base : {s.sender_update_at, s.recipient_update_at}) {
        mark(base, PP_LEAF_WITNESSES);
        for (size_t l = 0; l < L; l++) {
            const size_t at = base + PedersenTransferShape::update_levels_at + PT_UPDATE_LEVEL_WITNESSES * l;
            mark(at, PT_UPDATE_LEVEL_BITS_AT);
            mark(at + PT_UPDATE_LEVEL_BITS_AT, 2 * MW_DIGEST_BITS);
            mark(at + PT_UPDATE_LEVEL_ADDS_AT, (2 * MW_DIGEST_BITS - 1) * MW_COND_ADD);
        }
    }
    for (size_t i = 0; i < seen.size(); i++)
        if (seen[i] != 1) fail("a witness not covered exactly once", height, i);
    if (!(s.pack_row < s.sender_root_row && s.sender_root_row < s.sender_r1_row && s.sender_r1_row < s.recipient_r1_row &&
          s.recipient_r1_row < s.sum_pack_row && s.sum_pack_row < s.new_root_row && s.new_root_row + 1 == s.num_constraints))
        fail("the named rows' order", height, salted);
    printf("shape %zu %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", height, salted ? 1 : 0,
           s.num_instance, s.num_witness, s.num_constraints, s.balance_at, s.diff_at, s.sender_at, s.sender_update_at, s.r1_at,
           s.recipient_bits_at, s.recipient_at, s.sum_at, s.recipient_update_at, s.membership_witnesses, s.update_witnesses, s.section_rows,
           s.update_rows, s.pack_row, s.sender_root_row, s.sender_r1_row, s.recipient_r1_row, s.sum_pack_row, s.new_root_row);
    checked++;
}

static void refused(size_t height, bool salted) {
    PedersenTransferShape s;
    s.num_witness = 12345;
    if (pedersen_transfer_shape(height, salted, &s) || s.num_witness != 12345) fail("accepted, or wrote on refusal", height, salted);
    checked++;
}

// every plan: consecutive chunks from 0 that cover [0, count), each within the cap unless it holds one transfer, all but the last
// equally long
static void plan(size_t item_bytes, size_t count, size_t cap_bytes) {
    std::vector<WitnessChunk> chunks(3);  // stale entries must go
    if (!witness_chunk_plan(item_bytes, count, cap_bytes, &chunks)) fail("plan refused", item_bytes, count);
    size_t next = 0;
    for (size_t i = 0; i < chunks.size(); i++) {
        const WitnessChunk& c = chunks[i];
        if (c.base != next || c.count == 0) fail("chunks not consecutive", item_bytes, count);
        if (c.count > 1 && c.count > cap_bytes / item_bytes) fail("a chunk above the cap", item_bytes, count);
        if (i + 1 < chunks.size() && c.count != chunks[0].count) fail("a short chunk before the last", item_bytes, count);
        next += c.count;
    }
    if (next != count || (count == 0) != chunks.empty()) fail("the chunks do not cover the block", item_bytes, count);
    printf("plan %zu %zu %zu", item_bytes, count, cap_bytes);
    for (const WitnessChunk& c : chunks) printf(" %zu:%zu", c.base, c.count);
    printf("\n");
    checked++;
}

int main() {
    for (size_t h = PP_MIN_HEIGHT; h <= PP_MAX_HEIGHT; h++)
        for (int salted = 0; salted < 2; salted++) walk(h, salted != 0);
    refused(0, false);
    refused(1, true);
    refused(PP_MAX_HEIGHT + 1, false);
    refused(SIZE_MAX, true);
    PedersenTransferShape s;
    if (!pedersen_transfer_shape(3, false, &s)) fail("height 3", 3, 0);
    const size_t item = 32 * s.num_witness;
    for (size_t count : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)7, (size_t)8, (size_t)9, (size_t)65})
        for (size_t cap : {(size_t)0, item - 1, item, 2 * item - 1, 2 * item, 3 * item + 5, 8 * item, 100 * item}) plan(item, count, cap);
    if (!pedersen_transfer_shape(9, false, &s)) fail("height 9", 9, 0);
    plan(32 * s.num_witness, 1000, WITNESS_STAGE_BYTES);  // the library's own cap
    plan(1, 5, SIZE_MAX);
    plan(SIZE_MAX, 3, SIZE_MAX - 1);
    std::vector<WitnessChunk> none(2);
    if (witness_chunk_plan(0, 4, 100, &none) || !none.empty() || witness_chunk_items(0, 100) != 0) fail("item_bytes 0", 0, 4);
    for (const WitnessChunk c : WitnessChunks(0, 4)) fail("a chunk of no items", c.base, c.count);
    checked++;
    printf("stage %zu\n", (size_t)WITNESS_STAGE_BYTES);
    printf("ok %zu\n", checked);
    return 0;
}

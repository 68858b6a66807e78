// poseidon_shape_check.cpp — csrc/host/poseidon_shape.h against a brute-force walk of the sponge schedule and of the S-box chain,
// built with -fsanitize=address,undefined by tests/test_poseidon_circuit_host.py.  Prints "ok <cases checked>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "host/poseidon_shape.h"

using namespace swm;

static size_t checked = 0;

static void fail(const char* what, size_t a, size_t b, size_t c, size_t d, size_t e) {
    fprintf(stderr, "FAIL %s: full %zu partial %zu alpha %zu n_in %zu n_out %zu\n", what, a, b, c, d, e);
    exit(1);
}

// Walks what build_poseidon_hash does, one step at a time, and marks every witness it allocates in `seen`.
static void walk(size_t full, size_t partial, uint64_t alpha, bool bytes, size_t n_in, size_t n_out) {
    PoseidonShape s;
    if (!poseidon_shape(full, partial, alpha, bytes, n_in, n_out, &s)) fail("refused", full, partial, (size_t)alpha, n_in, n_out);
    // the elements absorbed: the chunks of (8 length bytes || input), counted one byte at a time
    size_t elems = 0;
    if (bytes) {
        size_t in_chunk = 0;
        for (size_t pos = 0; pos < 8 + n_in; pos++) {
            if (in_chunk == 0) elems++;
            in_chunk = in_chunk + 1 == 31 ? 0 : in_chunk + 1;
        }
    } else {
        elems = n_in;
    }
    size_t witnesses = bytes ? 8 * n_in : n_in, rows = bytes ? 8 * n_in : 0, perms = 0;
    const size_t sponge_at = witnesses;
    std::vector<unsigned char> seen(s.num_witness, 0);
    for (size_t i = 0; i < sponge_at; i++) {
        if (i >= seen.size()) fail("input witness out of range", full, partial, (size_t)alpha, n_in, n_out);
        seen[i]++;
    }
    auto permute = [&] {
        perms++;
        for (size_t round = 0; round < full + partial; round++) {
            const bool is_full = round < full / 2 || round >= full / 2 + partial;
            for (size_t k = 0; k < (is_full ? 3u : 1u); k++) {
                int top = 63;
                while (!((alpha >> top) & 1)) top--;
                for (int b = top - 1; b >= 0; b--) {
                    for (int mul = 0; mul < (((alpha >> b) & 1) ? 2 : 1); mul++) {
                        if (witnesses >= seen.size()) fail("chain witness out of range", full, partial, (size_t)alpha, n_in, n_out);
                        seen[witnesses++]++;
                        rows++;
                    }
                }
            }
        }
    };
    // the sponge of ark-sponge 0.3.0: absorb, then squeeze
    size_t idx = 0;
    for (size_t e = 0; e < elems; e++) {
        if (idx == 2) {
            permute();
            idx = 0;
        }
        idx++;
    }
    idx = 2;
    for (size_t j = 0; j < n_out; j++) {
        if (idx == 2) {
            permute();
            idx = 0;
        }
        idx++;
        rows++;
    }
    if (s.elems != elems || s.perms != perms) fail("schedule", full, partial, (size_t)alpha, n_in, n_out);
    if (s.num_instance != 1 + n_out || s.num_witness != witnesses || s.num_constraints != rows) fail("counts", full, partial, (size_t)alpha, n_in, n_out);
    if (s.input_at != 0 || s.sponge_at != sponge_at) fail("offsets", full, partial, (size_t)alpha, n_in, n_out);
    if (s.perms * s.sboxes * s.chain != witnesses - sponge_at || s.sboxes != 3 * full + partial) fail("products", full, partial, (size_t)alpha, n_in, n_out);
    for (size_t i = 0; i < seen.size(); i++)
        if (seen[i] != 1) fail("a witness not written exactly once", full, partial, (size_t)alpha, n_in, n_out);
    checked++;
}

static void refused(size_t full, size_t partial, uint64_t alpha, bool bytes, size_t n_in, size_t n_out) {
    PoseidonShape s;
    s.num_witness = 12345;
    if (poseidon_shape(full, partial, alpha, bytes, n_in, n_out, &s) || s.num_witness != 12345)
        fail("accepted, or wrote on refusal", full, partial, (size_t)alpha, n_in, n_out);
    checked++;
}

int main() {
    for (size_t n = 0; n <= 400; n++) walk(8, 29, 17, true, n, 1);
    for (size_t n_in = 0; n_in <= 64; n_in++)
        for (size_t n_out = 1; n_out <= 16; n_out++) walk(8, 29, 17, false, n_in, n_out);
    const uint64_t alphas[] = {2, 3, 5, 17, 65535};
    const size_t shapes[][2] = {{8, 29}, {8, 0}, {2, 29}, {2, 0}};
    for (uint64_t alpha : alphas)
        for (const auto& sh : shapes) {
            walk(sh[0], sh[1], alpha, true, 11, 1);
            walk(sh[0], sh[1], alpha, true, 55, 1);
            walk(sh[0], sh[1], alpha, false, 5, 3);
        }
    // the largest legal shapes
    walk(8, 29, 17, true, PC_MAX_BYTES, 1);
    walk(8, 247, 65535, false, PC_MAX_IN, PC_MAX_OUT);
    walk(254, 1, 65535, true, PC_MAX_BYTES, 1);
    // the limits
    refused(8, 29, 17, true, PC_MAX_BYTES + 1, 1);
    refused(8, 29, 17, false, PC_MAX_IN + 1, 1);
    refused(8, 29, 17, false, 1, 0);
    refused(8, 29, 17, false, 1, 17);
    refused(8, 29, 17, true, 1, 2);
    refused(7, 29, 17, true, 1, 1);
    refused(0, 29, 17, true, 1, 1);
    refused(8, 248, 17, true, 1, 1);
    refused(256, 0, 17, true, 1, 1);
    refused(8, 29, 1, true, 1, 1);
    refused(8, 29, 0, true, 1, 1);
    refused(8, 29, 65536, true, 1, 1);
    // arguments near SIZE_MAX: refused by the limits, before any sum or product of two of them can wrap
    refused(SIZE_MAX, 29, 17, true, 1, 1);
    refused(SIZE_MAX - 1, 2, 17, true, 1, 1);
    refused(8, SIZE_MAX, 17, true, 1, 1);
    refused(8, SIZE_MAX - 7, 17, true, 1, 1);
    refused(8, 29, UINT64_MAX, true, 1, 1);
    refused(8, 29, 17, true, SIZE_MAX, 1);
    refused(8, 29, 17, true, SIZE_MAX - 8, 1);
    refused(8, 29, 17, false, SIZE_MAX / 32 + 1, 1);
    refused(8, 29, 17, false, 1, SIZE_MAX);
    refused(SIZE_MAX, SIZE_MAX, UINT64_MAX, false, SIZE_MAX, SIZE_MAX);
    // the guard itself
    size_t v = 0;
    if (pc_mul(SIZE_MAX / 2 + 1, 2, &v) || pc_add(SIZE_MAX, 1, &v) || !pc_mul(SIZE_MAX / 2, 2, &v) || v != SIZE_MAX - 1 || !pc_add(SIZE_MAX - 1, 1, &v) ||
        v != SIZE_MAX) {
        fprintf(stderr, "FAIL overflow guard\n");
        return 1;
    }
    printf("ok %zu\n", checked);
    return 0;
}

// blake2s_shape_check.cpp — csrc/host/blake2s_shape.h under -fsanitize=address,undefined (tests/test_blake2s_circuit_host.py): the
// counts and offsets of the Blake2s hash circuit, the witness-to-recorded-word map and the message-word reader that
// csrc/blake2s.hip and csrc/blake2s_witness.hip work by.  Stand-alone: no GPU, no library.  Checks
//   - for every input_len in 0 .. 200 and 65536 the three counts and the two offsets against a brute-force walk of the layout;
//   - that bh_b2s_source inverts sv_b2s_slot on all 21472 witnesses of a block;
//   - for input_len 0, 1, 32, 64, 65, 129 and batches of 1 and 3 items (items 1 and 2 of an odd length are not word-aligned) the
//     witness bits expanded on the host the way the kernel expands them — message words through bh_message_word out of a heap
//     buffer of exactly count x input_len bytes, so that a read past its end is an ASan report, blocks through
//     sv_b2s_compress_record, witnesses in storage order through bh_b2s_source: the message bits are the input's, every witness
//     equals the bit sv_b2s_slot places there, and the digest bits at digest_at are csrc/host/blake2s.h's digest;
//   - the refusals above 65536 up to SIZE_MAX.
// Prints "ok <shapes> <items>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "host/blake2s.h"
#include "host/blake2s_shape.h"

using namespace swm;

static void fail(const char* what, size_t input_len, size_t item) {
    fprintf(stderr, "blake2s_shape_check: %s (input_len %zu, item %zu)\n", what, input_len, item);
    exit(1);
}

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint32_t next_u32() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 32);
}

// the layout walked group by group, nothing multiplied out
static void walk(size_t input_len, size_t* witnesses, size_t* rows, size_t* b2s_at, size_t* digest_at) {
    size_t w = 0, r = 0;
    for (size_t i = 0; i < input_len; i++)
        for (int b = 0; b < 8; b++) {
            w++;  // the bit
            r++;  // its booleanity row
        }
    *b2s_at = w;
    size_t blocks = 0;
    for (size_t done = 0; blocks == 0 || done < input_len; done += 64) blocks++;
    for (size_t blk = 0; blk < blocks; blk++) {
        for (int g = 0; g < 80; g++)
            for (int half = 0; half < 2; half++) {
                w += 34 + 32 + 33 + 32;
                r += 34 + 32 + 33 + 32 + 2;  // a packing row per sum
            }
        for (int i = 0; i < 8; i++) {
            w += 32;  // h ^ v[i]
            r += 32;
            if (blk + 1 == blocks && i == 0) *digest_at = w;
            w += 32;  // ^ v[i + 8]: the new state word, a digest word in the last block
            r += 32;
        }
    }
    r += 2;  // lo, hi
    *witnesses = w;
    *rows = r;
}

int main() {
    size_t shapes = 0, items = 0;
    Blake2sShape s;
    const size_t bad_lens[] = {BH_MAX_INPUT_LEN + 1, (size_t)1 << 40, ~(size_t)0 - 63, ~(size_t)0 / 8 + 1, ~(size_t)0};
    for (size_t len : bad_lens)
        if (blake2s_shape(len, &s)) fail("input_len accepted", len, 0);

    for (size_t len = 0; len <= 201; len++) {
        const size_t n = len == 201 ? (size_t)BH_MAX_INPUT_LEN : len;
        size_t w, r, at, dg;
        walk(n, &w, &r, &at, &dg);
        if (!blake2s_shape(n, &s)) fail("shape refused", n, 0);
        const size_t blocks = n ? (n + 63) / 64 : 1;
        if (s.input_len != n || s.blocks != blocks || s.num_instance != 3) fail("block or instance count", n, 0);
        if (s.num_witness != w || s.num_witness != 8 * n + 21472 * blocks) fail("witness count", n, 0);
        if (s.num_constraints != r || s.num_constraints != 8 * n + 21792 * blocks + 2) fail("row count", n, 0);
        if (s.b2s_at != at || s.digest_at != dg) fail("offsets", n, 0);
        if (s.num_witness >= ((size_t)1 << 31)) fail("chunk indices leave 32 bits", n, 0);
        shapes++;
    }
    if (!blake2s_shape(32, &s) || s.num_witness != 21728 || s.num_constraints != 22050) fail("the reference's 32-byte case", 32, 0);

    // bh_b2s_source is the inverse of sv_b2s_slot
    {
        std::vector<int> seen(SV_BLOCK_WITNESSES, 0);
        for (uint32_t k = 0; k < SV_BLOCK_WORDS; k++) {
            const SvSlot slot = sv_b2s_slot(k);
            for (uint32_t b = 0; b < slot.bits; b++) {
                const BhSource src = bh_b2s_source(slot.at + b);
                if (src.word != k || src.bit != b) fail("bh_b2s_source", k, b);
                seen[slot.at + b]++;
            }
        }
        for (size_t e = 0; e < SV_BLOCK_WITNESSES; e++)
            if (seen[e] != 1) fail("a witness of a block without exactly one source", e, 0);
    }

    const size_t lens[] = {0, 1, 32, 64, 65, 129};
    for (size_t len : lens)
        for (size_t count : {(size_t)1, (size_t)3}) {
            if (!blake2s_shape(len, &s)) fail("shape refused", len, 0);
            const size_t total = count * len;
            // exactly `total` bytes on the heap (malloc aligns to 16): ASan sees any byte read past them
            uint8_t* in = (uint8_t*)malloc(total ? total : 1);
            if (!in) fail("malloc", len, 0);
            for (size_t i = 0; i < total; i++) in[i] = len == 32 && count == 1 ? 1 : (uint8_t)next_u32();
            const uint32_t* words = reinterpret_cast<const uint32_t*>(in);
            for (size_t item = 0; item < count; item++) {
                const size_t at = item * len, end = at + len;
                std::vector<uint8_t> bits(s.num_witness, 0xFF);
                for (size_t e = 0; e < 8 * len; e++) bits[e] = (in[at + (e >> 3)] >> (e & 7)) & 1u;
                uint32_t h[8];
                sv_b2s_init(h);
                std::vector<uint64_t> rec(SV_BLOCK_WORDS);
                for (size_t blk = 0; blk < s.blocks; blk++) {
                    uint32_t m[16];
                    for (size_t j = 0; j < 16; j++) {
                        m[j] = bh_message_word(words, total, at + 64 * blk + 4 * j, end);
                        uint32_t want = 0;
                        for (size_t k = 0; k < 4; k++) {
                            const size_t o = at + 64 * blk + 4 * j + k;
                            if (o < end) want |= (uint32_t)in[o] << (8 * k);
                        }
                        if (m[j] != want) fail("bh_message_word", len, item);
                    }
                    const bool last = blk + 1 == s.blocks;
                    sv_b2s_compress_record(h, m, last ? (uint64_t)len : (uint64_t)64 * (blk + 1), last, rec.data());
                    uint8_t* bw = &bits[s.b2s_at + SV_BLOCK_WITNESSES * blk];
                    for (uint32_t e = 0; e < SV_BLOCK_WITNESSES; e++) {  // storage order, as the kernel writes
                        const BhSource src = bh_b2s_source(e);
                        bw[e] = (uint8_t)((rec[src.word] >> src.bit) & 1u);
                    }
                    for (uint32_t k = 0; k < SV_BLOCK_WORDS; k++) {  // slot order, as schnorr_witness.hip writes
                        const SvSlot slot = sv_b2s_slot(k);
                        for (uint32_t b = 0; b < slot.bits; b++)
                            if (bw[slot.at + b] != ((rec[k] >> b) & 1u)) fail("a witness differs from its slot's bit", len, item);
                    }
                }
                for (size_t e = 0; e < s.num_witness; e++)
                    if (bits[e] > 1) fail("a witness was not written", len, item);
                uint8_t want[32];
                Blake2s::digest(in + at, len, want);
                for (size_t i = 0; i < 8; i++)
                    for (size_t j = 0; j < 32; j++)
                        if (bits[s.digest_at + 64 * i + j] != ((want[4 * i + j / 8] >> (j % 8)) & 1u)) fail("digest bits", len, item);
                if (len == 32 && count == 1) {  // the reference's [1u8; 32]
                    static const uint8_t known[4] = {0x5d, 0xa8, 0xbc, 0xf5};
                    if (memcmp(want, known, 4) != 0) fail("the digest of [1u8; 32]", len, item);
                }
                items++;
            }
            free(in);
        }
    printf("ok %zu %zu\n", shapes, items);
    return 0;
}

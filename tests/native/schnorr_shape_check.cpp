// schnorr_shape_check.cpp — csrc/host/schnorr_shape.h under -fsanitize=address,undefined (tests/test_schnorr_circuit_host.py): the
// offset arithmetic of the Schnorr verification circuit and the Blake2s schedule that csrc/schnorr_witness.hip writes witnesses
// by.  Stand-alone: no GPU, no library.  Checks for a grid of (msg_len, salted) that the witness groups tile the vector without
// gap or overlap, that the recorded words of a block tile its 21472 witnesses in order, that the recording compression arrives at
// the digest of a plain Blake2s written here, that every recorded word fits the width of its slot, and that the last recorded
// words of a block are its new state.  Prints "ok <shapes> <blocks>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "host/schnorr_shape.h"

using namespace swm;

static void fail(const char* what, size_t msg_len, int salted) {
    fprintf(stderr, "schnorr_shape_check: %s (msg_len %zu, salted %d)\n", what, msg_len, salted);
    exit(1);
}

// ---- a plain BLAKE2s-256 (RFC 7693), unkeyed, with its own tables
static const uint32_t IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
static const uint8_t SIGMA[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
static void plain_g(uint32_t* v, int a, int b, int c, int d, uint32_t x, uint32_t y) {
    v[a] = v[a] + v[b] + x; v[d] = rotr(v[d] ^ v[a], 16); v[c] = v[c] + v[d]; v[b] = rotr(v[b] ^ v[c], 12);
    v[a] = v[a] + v[b] + y; v[d] = rotr(v[d] ^ v[a], 8);  v[c] = v[c] + v[d]; v[b] = rotr(v[b] ^ v[c], 7);
}
static void plain_compress(uint32_t* h, const uint32_t* m, uint64_t t, bool last) {
    uint32_t v[16];
    for (int i = 0; i < 8; i++) { v[i] = h[i]; v[i + 8] = IV[i]; }
    v[12] ^= (uint32_t)t;
    v[13] ^= (uint32_t)(t >> 32);
    if (last) v[14] = ~v[14];
    for (int r = 0; r < 10; r++) {
        const uint8_t* s = SIGMA[r];
        plain_g(v, 0, 4, 8, 12, m[s[0]], m[s[1]]);   plain_g(v, 1, 5, 9, 13, m[s[2]], m[s[3]]);
        plain_g(v, 2, 6, 10, 14, m[s[4]], m[s[5]]);  plain_g(v, 3, 7, 11, 15, m[s[6]], m[s[7]]);
        plain_g(v, 0, 5, 10, 15, m[s[8]], m[s[9]]);  plain_g(v, 1, 6, 11, 12, m[s[10]], m[s[11]]);
        plain_g(v, 2, 7, 8, 13, m[s[12]], m[s[13]]); plain_g(v, 3, 4, 9, 14, m[s[14]], m[s[15]]);
    }
    for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
}

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint32_t next_u32() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 32);
}

int main() {
    size_t shapes = 0, blocks_run = 0;
    SchnorrShape s;
    const size_t bad_lens[] = {SV_MAX_MSG_LEN + 1, (size_t)1 << 40, ~(size_t)0};
    for (size_t len : bad_lens)
        for (int salted = 0; salted < 2; salted++)
            if (schnorr_shape(len, salted != 0, &s)) fail("msg_len accepted", len, salted);

    // the slots of a block: in order, no gap, no overlap, widths 34 / 33 / 32
    {
        size_t at = 0;
        for (uint32_t k = 0; k < SV_BLOCK_WORDS; k++) {
            const SvSlot slot = sv_b2s_slot(k);
            if (slot.at != at) fail("slot offset", k, 0);
            const uint32_t want = k >= 640 ? 32u : (k & 3u) == 0 ? 34u : (k & 3u) == 2 ? 33u : 32u;
            if (slot.bits != want) fail("slot width", k, 0);
            at += slot.bits;
        }
        if (at != SV_BLOCK_WITNESSES || SV_BLOCK_WITNESSES != 21472 || SV_BLOCK_ROWS != 21792) fail("block size", 0, 0);
    }

    const size_t lens[] = {0, 1, 23, 24, 31, 32, 33, 63, 64, 65, 95, 96, 97, 200, 1000, SV_MAX_MSG_LEN};
    for (size_t len : lens)
        for (int salted = 0; salted < 2; salted++) {
            if (!schnorr_shape(len, salted != 0, &s)) fail("shape refused", len, salted);
            const size_t hash_len = (salted ? 160 : 128) + len, blocks = (hash_len + 63) / 64;
            if (s.hash_len != hash_len || s.blocks != blocks || blocks < 2) fail("block count", len, salted);
            if (s.sig_at != 4 + 8 * len || s.fix_at != s.sig_at + 512 || s.dbl_at != s.fix_at + 1530 || s.sel_at != s.dbl_at + 1275 ||
                s.add_at != s.sel_at + 512 || s.sum_at != s.add_at + 1785 || s.dec_at != s.sum_at + 7 || s.b2s_at != s.dec_at + 1024)
                fail("group offsets", len, salted);
            if (s.num_instance != 1 || s.num_witness != 6649 + 8 * len + 21472 * blocks) fail("witness count", len, salted);
            if (s.num_constraints != 6672 + 8 * len + 21792 * blocks) fail("row count", len, salted);
            if (s.num_witness >= ((size_t)1 << 32)) fail("offsets leave 32 bits", len, salted);
            shapes++;
            if (len > 1000) continue;

            // a random input of hash_len bytes through the recording compression and through the plain one
            std::vector<uint8_t> in(64 * blocks, 0);
            for (size_t i = 0; i < hash_len; i++) in[i] = (uint8_t)next_u32();
            uint32_t h[8], hp[8];
            sv_b2s_init(h);
            for (int i = 0; i < 8; i++) hp[i] = IV[i];
            hp[0] ^= 0x01010020u;
            std::vector<uint64_t> rec(SV_BLOCK_WORDS);
            for (size_t b = 0; b < blocks; b++) {
                uint32_t m[16];
                for (int k = 0; k < 16; k++) {
                    const uint8_t* p = &in[64 * b + 4 * k];
                    m[k] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
                }
                const bool last = b + 1 == blocks;
                const uint64_t t = last ? hash_len : 64 * (b + 1);
                uint32_t before[8];
                memcpy(before, h, sizeof(before));
                sv_b2s_compress_record(h, m, t, last, rec.data());
                plain_compress(hp, m, t, last);
                if (memcmp(h, hp, sizeof(h)) != 0) fail("digest state differs from the plain Blake2s", len, salted);
                for (uint32_t k = 0; k < SV_BLOCK_WORDS; k++)
                    if (rec[k] >> sv_b2s_slot(k).bits) fail("a recorded word is wider than its slot", len, salted);
                // the feed-forward's second xor is the new state
                for (int i = 0; i < 8; i++)
                    if (rec[640 + 2 * i + 1] != h[i]) fail("feed-forward", len, salted);
                blocks_run++;
            }
        }
    printf("ok %zu %zu\n", shapes, blocks_run);
    return 0;
}

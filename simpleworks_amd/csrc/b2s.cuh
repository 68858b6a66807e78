// b2s.cuh — BLAKE2s-256 (RFC 7693), unkeyed, on plain 32-bit words: the compression function shared by schnorr.hip (the
// challenge hash behind the signature kernels) and blake2s.hip (the random oracle, batched).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ff.cuh"

namespace swm {

// ---------------------------------------------------------------------------------------------- BLAKE2s-256 (RFC 7693), unkeyed
struct B2s {
    static constexpr uint32_t IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
    static constexpr uint8_t SIGMA[10][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
};
SWM_HD uint32_t b2s_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
// one compression; `t` = bytes hashed so far including this block.  The rounds are unrolled so that every index into m is a constant.
SWM_HD void b2s_compress(uint32_t (&h)[8], const uint32_t (&m)[16], uint64_t t, bool last) {
    uint32_t v[16];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        v[i] = h[i];
        v[i + 8] = B2s::IV[i];
    }
    v[12] ^= (uint32_t)t;
    v[13] ^= (uint32_t)(t >> 32);
    if (last) v[14] = ~v[14];
#define SWM_B2S_G(a, b, c, d, x, y)       \
    v[a] = v[a] + v[b] + (x);             \
    v[d] = b2s_rotr(v[d] ^ v[a], 16);     \
    v[c] = v[c] + v[d];                   \
    v[b] = b2s_rotr(v[b] ^ v[c], 12);     \
    v[a] = v[a] + v[b] + (y);             \
    v[d] = b2s_rotr(v[d] ^ v[a], 8);      \
    v[c] = v[c] + v[d];                   \
    v[b] = b2s_rotr(v[b] ^ v[c], 7);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        SWM_B2S_G(0, 4, 8, 12, m[B2s::SIGMA[r][0]], m[B2s::SIGMA[r][1]])
        SWM_B2S_G(1, 5, 9, 13, m[B2s::SIGMA[r][2]], m[B2s::SIGMA[r][3]])
        SWM_B2S_G(2, 6, 10, 14, m[B2s::SIGMA[r][4]], m[B2s::SIGMA[r][5]])
        SWM_B2S_G(3, 7, 11, 15, m[B2s::SIGMA[r][6]], m[B2s::SIGMA[r][7]])
        SWM_B2S_G(0, 5, 10, 15, m[B2s::SIGMA[r][8]], m[B2s::SIGMA[r][9]])
        SWM_B2S_G(1, 6, 11, 12, m[B2s::SIGMA[r][10]], m[B2s::SIGMA[r][11]])
        SWM_B2S_G(2, 7, 8, 13, m[B2s::SIGMA[r][12]], m[B2s::SIGMA[r][13]])
        SWM_B2S_G(3, 4, 9, 14, m[B2s::SIGMA[r][14]], m[B2s::SIGMA[r][15]])
    }
#undef SWM_B2S_G
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
}

// h of an unkeyed BLAKE2s-256 before the first block: digest length 32, no key, fanout = depth = 1
SWM_HD void b2s_init(uint32_t (&h)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = B2s::IV[i];
    h[0] ^= 0x01010000u ^ 32u;
}

// 64-byte blocks of a message of `len` bytes: the empty message is one block of zeros
SWM_HD size_t b2s_blocks(size_t len) { return len ? (len + 63) / 64 : 1; }

}  // namespace swm

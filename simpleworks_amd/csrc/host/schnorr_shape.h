// schnorr_shape.h — the SHAPE of the Schnorr verification circuit (simpleworks_amd/workloads.py, build_schnorr_verification):
// how many variables and rows a message length and the presence of a salt give, where each group of witnesses starts, and the
// Blake2s schedule — which word recorded during a compression lands at which witness offset, with how many bits.  Plain C++, no
// GPU headers, no library state: shared by host_abi.inc (swm_schnorr_circuit_shape), by schnorr_witness.hip (which lays the
// witness vector out by these offsets and runs sv_b2s_compress_record on one lane) and by tests/native/schnorr_shape_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SWM_SHAPE_HD __host__ __device__ inline
#else
#define SWM_SHAPE_HD inline
#endif
#if defined(__clang__)
#define SWM_SHAPE_UNROLL _Pragma("unroll")
#else
#define SWM_SHAPE_UNROLL
#endif

namespace swm {

// Witness layout of one signature (the order in which build_schnorr_verification calls new_witness_variable):
//   key   x, y, xx, yy                                          4
//   msg   8 bits per message byte                               8 msg_len
//   sig   256 bits of the response s, 256 of the challenge e    512
//   fix   s G: steps 1 .. 255, t, b t, m1, m2, X3, Y3 each      255 x 6
//   dbl   P_{i+1} = 2 P_i, i = 0 .. 254: xy, xx, yy, x', y'     255 x 5
//   sel   Q_i = e_i P_i, i = 0 .. 255: qx, qy                   256 x 2
//   add   acc_i = acc_{i-1} + Q_i, i = 1 .. 255                 255 x 7   (x1y2, y1x2, y1y2, x1x2, their product, x3, y3)
//   sum   R' = s G + acc_255                                    7
//   dec   bits of Y.x, Y.y, R'.x, R'.y                          4 x 256
//   b2s   per 64-byte block: 80 G of 262, then 16 words of 32   21472 per block
static constexpr size_t SV_MAX_MSG_LEN = 65536;
static constexpr size_t SV_SCALAR_BITS = 256;
static constexpr size_t SV_FIX_STEP = 6, SV_DBL_STEP = 5, SV_SEL_STEP = 2, SV_ADD_STEP = 7;
static constexpr size_t SV_KEY_AT = 0, SV_KEY_WITNESSES = 4;
static constexpr size_t SV_MSG_AT = SV_KEY_AT + SV_KEY_WITNESSES;
static constexpr size_t SV_G_WORDS = 8;                                           // recorded words per G: sum, xor, sum, xor, twice
static constexpr size_t SV_G_WITNESSES = 34 + 32 + 33 + 32 + 34 + 32 + 33 + 32;  // 262
static constexpr size_t SV_G_ROWS = SV_G_WITNESSES + 4;                           // a packing row per sum
static constexpr size_t SV_BLOCK_G = 80;
static constexpr size_t SV_BLOCK_WORDS = SV_BLOCK_G * SV_G_WORDS + 16;            // 656: + two xors per word of the feed-forward
static constexpr size_t SV_BLOCK_WITNESSES = SV_BLOCK_G * SV_G_WITNESSES + 16 * 32;  // 21472
static constexpr size_t SV_BLOCK_ROWS = SV_BLOCK_G * SV_G_ROWS + 16 * 32;            // 21792
static constexpr size_t SV_DEC_ROWS = 256 + 1 + 3;  // booleanity, the packing row, `0 * 0 = bit` for bits 253 .. 255

struct SchnorrShape {
    size_t msg_len = 0;
    bool salted = false;
    size_t num_instance = 0, num_witness = 0, num_constraints = 0;
    size_t sig_at = 0, fix_at = 0, dbl_at = 0, sel_at = 0, add_at = 0, sum_at = 0, dec_at = 0, b2s_at = 0;
    size_t hash_len = 0, blocks = 0;  // bytes that enter Blake2s; 64-byte blocks (>= 2)
};

// false: msg_len > SV_MAX_MSG_LEN
inline bool schnorr_shape(size_t msg_len, bool salted, SchnorrShape* out) {
    if (msg_len > SV_MAX_MSG_LEN) return false;
    SchnorrShape s;
    s.msg_len = msg_len;
    s.salted = salted;
    s.num_instance = 1;
    s.sig_at = SV_MSG_AT + 8 * msg_len;
    s.fix_at = s.sig_at + 2 * SV_SCALAR_BITS;
    s.dbl_at = s.fix_at + (SV_SCALAR_BITS - 1) * SV_FIX_STEP;
    s.sel_at = s.dbl_at + (SV_SCALAR_BITS - 1) * SV_DBL_STEP;
    s.add_at = s.sel_at + SV_SCALAR_BITS * SV_SEL_STEP;
    s.sum_at = s.add_at + (SV_SCALAR_BITS - 1) * SV_ADD_STEP;
    s.dec_at = s.sum_at + SV_ADD_STEP;
    s.b2s_at = s.dec_at + 4 * 256;
    s.hash_len = (salted ? 160 : 128) + msg_len;
    s.blocks = (s.hash_len + 63) / 64;
    s.num_witness = s.b2s_at + SV_BLOCK_WITNESSES * s.blocks;
    // the on-curve rows (3); a booleanity row per message and signature bit; a row per witness of the curve arithmetic; the
    // decompositions; the hash; eight comparison rows
    s.num_constraints = 3 + 8 * msg_len + 2 * SV_SCALAR_BITS + (s.dec_at - s.fix_at) + 4 * SV_DEC_ROWS + SV_BLOCK_ROWS * s.blocks + 8;
    *out = s;
    return true;
}

// Recorded word k (0 .. SV_BLOCK_WORDS - 1) of a block: its first witness relative to the block's, and its width in bits.
// A G records sum (34 bits: three operands), xor, sum (33), xor, and the same again; the feed-forward records h ^ v[i] and
// that ^ v[i + 8] for i = 0 .. 7.
struct SvSlot {
    uint32_t at, bits;
};
SWM_SHAPE_HD SvSlot sv_b2s_slot(uint32_t k) {
    SvSlot s;
    if (k >= SV_BLOCK_G * SV_G_WORDS) {
        s.at = (uint32_t)(SV_BLOCK_G * SV_G_WITNESSES) + 32u * (k - (uint32_t)(SV_BLOCK_G * SV_G_WORDS));
        s.bits = 32;
        return s;
    }
    const uint32_t g = k >> 3, j = k & 7u, half = j >> 2, q = j & 3u;  // within a half: 34 | 32 | 33 | 32 at 0, 34, 66, 99
    s.at = g * (uint32_t)SV_G_WITNESSES + half * 131u + (q == 0 ? 0u : q == 1 ? 34u : q == 2 ? 66u : 99u);
    s.bits = q == 0 ? 34u : q == 2 ? 33u : 32u;
    return s;
}

// BLAKE2s (RFC 7693) constants, as single values so that host and device read them alike
SWM_SHAPE_HD uint32_t sv_b2s_iv(int i) {
    return i == 0 ? 0x6A09E667u : i == 1 ? 0xBB67AE85u : i == 2 ? 0x3C6EF372u : i == 3 ? 0xA54FF53Au : i == 4 ? 0x510E527Fu
         : i == 5 ? 0x9B05688Cu : i == 6 ? 0x1F83D9ABu : 0x5BE0CD19u;
}
// the message schedule, one nibble per entry: row r is sigma_r[0] in the lowest nibble
SWM_SHAPE_HD uint64_t sv_b2s_sigma(int r) {
    return r == 0 ? 0xFEDCBA9876543210ull : r == 1 ? 0x357B20C16DF984AEull : r == 2 ? 0x491763EADF250C8Bull : r == 3 ? 0x8F04A562EBCD1397ull
         : r == 4 ? 0xD386CB1EFA427509ull : r == 5 ? 0x91EF57D438B0A6C2ull : r == 6 ? 0xB8293670A4DEF15Cull : r == 7 ? 0xA2684F05931CE7BDull
         : r == 8 ? 0x5A417D2C803B9EF6ull : 0x0DC3E9BF5167482Aull;
}
SWM_SHAPE_HD uint32_t sv_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// One compression that records every intermediate the circuit holds as witnesses: rec[k] is recorded word k of sv_b2s_slot —
// a sum with its carries (up to 34 bits), or an xor before its rotation.  `t` = bytes hashed so far including this block.
SWM_SHAPE_HD void sv_b2s_compress_record(uint32_t* h, const uint32_t* m, uint64_t t, bool last, uint64_t* rec) {
    uint32_t v[16];
    for (int i = 0; i < 8; i++) {
        v[i] = h[i];
        v[i + 8] = sv_b2s_iv(i);
    }
    v[12] ^= (uint32_t)t;
    v[13] ^= (uint32_t)(t >> 32);
    if (last) v[14] = ~v[14];
    size_t k = 0;
    for (int r = 0; r < 10; r++) {
        const uint64_t sigma = sv_b2s_sigma(r);
        SWM_SHAPE_UNROLL
        for (int g = 0; g < 8; g++) {
            const int a = g & 3, b = 4 + ((g + (g >> 2)) & 3), c = 8 + ((g + 2 * (g >> 2)) & 3), d = 12 + ((g + 3 * (g >> 2)) & 3);
            const uint32_t x = m[(sigma >> (8 * g)) & 15u], y = m[(sigma >> (8 * g + 4)) & 15u];
            uint64_t s;
            uint32_t w;
            s = (uint64_t)v[a] + v[b] + x;  rec[k++] = s;  v[a] = (uint32_t)s;
            w = v[d] ^ v[a];                rec[k++] = w;  v[d] = sv_rotr(w, 16);
            s = (uint64_t)v[c] + v[d];      rec[k++] = s;  v[c] = (uint32_t)s;
            w = v[b] ^ v[c];                rec[k++] = w;  v[b] = sv_rotr(w, 12);
            s = (uint64_t)v[a] + v[b] + y;  rec[k++] = s;  v[a] = (uint32_t)s;
            w = v[d] ^ v[a];                rec[k++] = w;  v[d] = sv_rotr(w, 8);
            s = (uint64_t)v[c] + v[d];      rec[k++] = s;  v[c] = (uint32_t)s;
            w = v[b] ^ v[c];                rec[k++] = w;  v[b] = sv_rotr(w, 7);
        }
    }
    for (int i = 0; i < 8; i++) {
        const uint32_t w = h[i] ^ v[i];
        rec[k++] = w;
        h[i] = w ^ v[i + 8];
        rec[k++] = h[i];
    }
}

// h of an unkeyed BLAKE2s-256 before the first block
SWM_SHAPE_HD void sv_b2s_init(uint32_t* h) {
    for (int i = 0; i < 8; i++) h[i] = sv_b2s_iv(i);
    h[0] ^= 0x01010020u;
}

}  // namespace swm

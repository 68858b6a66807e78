// schnorr.hip — the reference's native Schnorr scheme on ed-on-BLS12-377, batched: keygen, sign and verify with one lane per item.
//
// What the reference does there (src/schnorr_signature/schnorr.rs, SimpleSchnorr = Schnorr<EdwardsProjective>, one call per item):
//   :57-62     setup    salt = None, generator = prime_subgroup_generator()
//   :64-80     keygen   x = ScalarField::rand, pk = x G
//   :82-124    sign     k = ScalarField::rand, R = k G, e = Blake2s([salt] || to_bytes![pk] || to_bytes![R] || message),
//                       s = k - from_le_bytes_mod_order(e) x; the signature is (s, e)
//   :126-160   verify   R' = s G + from_le_bytes_mod_order(e) pk; accept iff Blake2s([salt] || pk || R' || message) == e
// to_bytes! of an affine point is x || y, 32 little-endian bytes each in standard form [U].
//
// On the GPU.  The curve is pedersen.hip's (ed.cuh over ff.cuh's Fr); the two scalar multiplications are ed_mul.cuh's, shared with
// elgamal.hip.  s G comes from a table of the generator's window
// multiples, 32 windows of 8 bits (768 KB, resident in L2): one mixed addition per non-zero byte of s.  e Y is a signed
// 4-bit-digit ladder over a per-signature table of 1 Y .. 8 Y in cached form: e + 0x0777..7 read nibble by nibble gives the 63
// digits nibble - 7 in [-7, 8], so there is no carry chain; 4 doublings and at most one addition per digit.  That table is 1 KB
// per lane and indexed at run time, so it lives in a global buffer laid out [entry][word][signature]: lanes that pick the same
// entry read neighbouring words.  One inversion per item (frinv.cuh), then the hash, streamed block by block from the five
// 32-byte pieces and the message without assembling the input anywhere.
// The scalar field (order l, 251 bits) needs no Montgomery form: a canonical test, a reduction of 256 bits by at most six
// conditional subtractions (2^256 / l < 55), and for signing one 256 x 256 product reduced bit by bit.
// The addition law is complete (ed.cuh): identity, doublings, keys of order 2 and 4 and e = 0 take the common path.
#include <hip/hip_runtime.h>

#include "b2s.cuh"
#include "context.h"
#include "ed_mul.cuh"
#include "schnorr.h"
#include "swmarlin.h"

namespace swm {

// ---------------------------------------------------------------------------------------------- the scalar field, beyond ed_mul.cuh's canonical test
// from_le_bytes_mod_order of 32 bytes: a < 2^256 < 55 l, so the quotient has six bits
SWM_HD void sc_reduce(uint32_t (&a)[8]) {
    sc_cond_sub<5>(a);
    sc_cond_sub<4>(a);
    sc_cond_sub<3>(a);
    sc_cond_sub<2>(a);
    sc_cond_sub<1>(a);
    sc_cond_sub<0>(a);
}
// k - x e mod l (k, x, e < l): schoolbook product, then one shift-and-subtract step per bit.  Once per signature, beside
// the ~2 000 field products of k G.
SWM_HD void sc_mulsub(const uint32_t (&k)[8], const uint32_t (&x)[8], const uint32_t (&e)[8], uint32_t (&out)[8]) {
    uint32_t p[16];
#pragma unroll
    for (int i = 0; i < 16; i++) p[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            c += (uint64_t)x[i] * e[j] + p[i + j];
            p[i + j] = (uint32_t)c;
            c >>= 32;
        }
        p[i + 8] = (uint32_t)c;
    }
    uint32_t r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int w = 15; w >= 0; w--) {
        uint32_t word = p[w];
#pragma unroll 1
        for (int b = 0; b < 32; b++) {  // r = 2 r + bit < 2 l, then back below l
#pragma unroll
            for (int i = 7; i > 0; i--) r[i] = (r[i] << 1) | (r[i - 1] >> 31);
            r[0] = (r[0] << 1) | (word >> 31);
            word <<= 1;
            sc_cond_sub<0>(r);
        }
    }
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t t = (uint64_t)k[i] - r[i] - borrow;
        out[i] = (uint32_t)t;
        borrow = (uint32_t)(t >> 63);
    }
    const uint32_t mask = 0u - borrow;
    uint32_t carry = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t t = (uint64_t)out[i] + (EdScalar::L[i] & mask) + carry;
        out[i] = (uint32_t)t;
        carry = (uint32_t)(t >> 32);
    }
}

// what a kernel needs of a swm_schnorr
struct SchnorrDev {
    const EdRow* table;  // [32 windows][256]: row (w, v) = v 2^(8 w) G
    Fr k2d, d;
    uint32_t salt[8];
    uint32_t has_salt;
};

// Blake2s([salt] || pk.x || pk.y || R.x || R.y || message) -> h.  The input is a run of 32-byte pieces: five that sit in
// registers (the salt one skipped when there is none), then the message.  Block b holds pieces 2 b and 2 b + 1; a word of a
// register piece is picked by a select on the piece number, a word of the message is read from memory, zero past its end.
SWM_HD void schnorr_hash(const SchnorrDev& P, const uint32_t (&px)[8], const uint32_t (&py)[8], const uint32_t (&rx)[8],
                         const uint32_t (&ry)[8], const uint8_t* msg, size_t len, uint32_t (&h)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = B2s::IV[i];
    h[0] ^= 0x01010000u ^ 32u;  // digest length 32, no key, fanout = depth = 1
    const size_t skip = P.has_salt ? 0 : 1;
    const size_t total = (5 - skip) * 32 + len;
    const size_t nblocks = (total + 63) / 64;  // >= 2
#pragma unroll 1
    for (size_t b = 0; b < nblocks; b++) {
        uint32_t m[16];
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const size_t q = 2 * b + half + skip;
            if (q < 5) {
#pragma unroll
                for (int j = 0; j < 8; j++)
                    m[8 * half + j] = q == 0 ? P.salt[j] : q == 1 ? px[j] : q == 2 ? py[j] : q == 3 ? rx[j] : ry[j];
            } else {
                const size_t off = (q - 5) * 32;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    uint32_t w = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const size_t o = off + 4 * j + k;
                        if (o < len) w |= (uint32_t)msg[o] << (8 * k);
                    }
                    m[8 * half + j] = w;
                }
            }
        }
        const bool last = b + 1 == nblocks;
        b2s_compress(h, m, last ? (uint64_t)total : (uint64_t)64 * (b + 1), last);
    }
}

// s G + e Y (schnorr.rs:140-143), e < l: the ladder, then the table walk.  `tab` is this lane's column of the table buffer.
SWM_HD EdExt schnorr_commitment(const SchnorrDev& P, const EdExt& Y, const uint32_t (&s)[8], const uint32_t (&e)[8], uint32_t* tab,
                                size_t stride) {
    EdExt acc = ed_ladder_mul(Y, e, P.k2d, tab, stride);
    ed_fixed_mul(acc, P.table, s);
    return acc;
}

// ---------------------------------------------------------------------------------------------- kernels: one lane per item
// A refused input lowers *bad (refuse, ed_mul.cuh); the host then returns without copying anything out.

__global__ void __launch_bounds__(256) schnorr_keygen_kernel(SchnorrDev P, const uint8_t* __restrict__ secrets, size_t count,
                                                             uint8_t* __restrict__ out, unsigned* __restrict__ bad) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint32_t x[8], px[8], py[8];
    load_words(secrets + 32 * i, x);
    if (!sc_is_canonical(x)) return refuse(bad, i);
    EdExt acc = ed_identity();
    ed_fixed_mul(acc, P.table, x);
    ed_affine(acc, px, py);
    store_words(out + 64 * i, px);
    store_words(out + 64 * i + 32, py);
}

__global__ void __launch_bounds__(256) schnorr_sign_kernel(SchnorrDev P, const uint8_t* __restrict__ secrets, const uint8_t* __restrict__ pks,
                                                           const uint8_t* __restrict__ nonces, const uint8_t* __restrict__ msgs, size_t msg_len,
                                                           size_t count, uint8_t* __restrict__ out, unsigned* __restrict__ bad) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint32_t x[8], k[8], px[8], py[8], rx[8], ry[8], h[8], e[8], s[8];
    load_words(secrets + 32 * i, x);
    load_words(nonces + 32 * i, k);
    load_words(pks + 64 * i, px);
    load_words(pks + 64 * i + 32, py);
    EdExt Y;
    if (!sc_is_canonical(x) || !sc_is_canonical(k) || !ed_point_from_words(P.d, px, py, &Y)) return refuse(bad, i);
    EdExt acc = ed_identity();
    ed_fixed_mul(acc, P.table, k);
    ed_affine(acc, rx, ry);
    schnorr_hash(P, px, py, rx, ry, msgs + i * msg_len, msg_len, h);
#pragma unroll
    for (int j = 0; j < 8; j++) e[j] = h[j];
    sc_reduce(e);
    sc_mulsub(k, x, e, s);
    store_words(out + 64 * i, s);
    store_words(out + 64 * i + 32, h);
}

// items [base, base + n); lane j of the launch owns column j of `tab`.  COMMIT: the claimed commitment as affine bytes, a bad
// input refuses the call; otherwise one result byte, and a bad input is a signature that does not verify.
template <bool COMMIT>
__global__ void __launch_bounds__(256) schnorr_verify_kernel(SchnorrDev P, const uint8_t* __restrict__ pks, const uint8_t* __restrict__ sigs,
                                                             const uint8_t* __restrict__ msgs, size_t msg_len, size_t base, size_t n,
                                                             uint32_t* __restrict__ tab, size_t stride, uint8_t* __restrict__ out,
                                                             unsigned* __restrict__ bad) {
    const size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const size_t i = base + j;
    uint32_t px[8], py[8], s[8], c[8], e[8], rx[8], ry[8];
    load_words(pks + 64 * i, px);
    load_words(pks + 64 * i + 32, py);
    load_words(sigs + 64 * i, s);
    load_words(sigs + 64 * i + 32, c);
    EdExt Y;
    if (!sc_is_canonical(s) || !ed_point_from_words(P.d, px, py, &Y)) {
        if (COMMIT)
            refuse(bad, i);
        else
            out[i] = 0;
        return;
    }
#pragma unroll
    for (int w = 0; w < 8; w++) e[w] = c[w];
    sc_reduce(e);
    const EdExt acc = schnorr_commitment(P, Y, s, e, tab + j, stride);
    ed_affine(acc, rx, ry);
    if (COMMIT) {
        store_words(out + 64 * i, rx);
        store_words(out + 64 * i + 32, ry);
    } else {
        uint32_t h[8], diff = 0;
        schnorr_hash(P, px, py, rx, ry, msgs + i * msg_len, msg_len, h);
#pragma unroll
        for (int w = 0; w < 8; w++) diff |= h[w] ^ c[w];
        out[i] = diff == 0;
    }
}

}  // namespace swm

using namespace swm;

namespace {

constexpr size_t SCH_CHUNK = ED_LADDER_CHUNK;  // signatures per verify launch

SchnorrDev dev_params(const swm_schnorr* p) {
    SchnorrDev d;
    d.table = reinterpret_cast<const EdRow*>(p->d_table);
    d.k2d = fp_from_u64<Fr>(2 * ED_D);
    d.d = fp_from_u64<Fr>(ED_D);
    for (int i = 0; i < 8; i++) d.salt[i] = p->salt[i];
    d.has_salt = p->has_salt ? 1u : 0u;
    return d;
}

enum SchnorrOp { OP_KEYGEN, OP_SIGN, OP_VERIFY, OP_COMMIT };

// Stages the inputs (each array starts at a multiple of 32 count bytes: word-aligned), runs the kernel of `op`, and copies the
// result out only when no input was refused.
int schnorr_run(swm_ctx* ctx, const swm_schnorr* p, SchnorrOp op, const uint8_t* secrets, const uint8_t* pks, const uint8_t* nonces,
                const uint8_t* sigs, const uint8_t* msgs, size_t msg_len, size_t count, uint8_t* out, const char* what) {
    const size_t out_item = op == OP_VERIFY ? 1 : 64;
    const size_t n_sk = secrets ? 32 * count : 0, n_pk = pks ? 64 * count : 0, n_k = nonces ? 32 * count : 0, n_sig = sigs ? 64 * count : 0;
    const size_t n_msg = msgs ? msg_len * count : 0;
    uint8_t *d_in = nullptr, *d_res = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", n_sk + n_pk + n_k + n_sig + n_msg + 32, (void**)&d_in));
    SWM_TRY(scratch(ctx, "stage.b", 256 + out_item * count, (void**)&d_res));
    uint8_t *d_sk = d_in, *d_pk = d_sk + n_sk, *d_k = d_pk + n_pk, *d_sig = d_k + n_k, *d_msg = d_sig + n_sig;
    unsigned* d_bad = reinterpret_cast<unsigned*>(d_res);
    uint8_t* d_out = d_res + 256;
    if (n_sk) SWM_HIP(ctx, hipMemcpyAsync(d_sk, secrets, n_sk, hipMemcpyHostToDevice, ctx->stream));
    if (n_pk) SWM_HIP(ctx, hipMemcpyAsync(d_pk, pks, n_pk, hipMemcpyHostToDevice, ctx->stream));
    if (n_k) SWM_HIP(ctx, hipMemcpyAsync(d_k, nonces, n_k, hipMemcpyHostToDevice, ctx->stream));
    if (n_sig) SWM_HIP(ctx, hipMemcpyAsync(d_sig, sigs, n_sig, hipMemcpyHostToDevice, ctx->stream));
    if (n_msg) SWM_HIP(ctx, hipMemcpyAsync(d_msg, msgs, n_msg, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemsetAsync(d_bad, 0xff, sizeof(unsigned), ctx->stream));
    const SchnorrDev P = dev_params(p);
    const dim3 block(256);
    if (op == OP_KEYGEN) {
        SWM_LAUNCH(ctx, "schnorr_keygen", schnorr_keygen_kernel, dim3((unsigned)((count + 255) / 256)), block, 0, P, d_sk, count, d_out, d_bad);
    } else if (op == OP_SIGN) {
        SWM_LAUNCH(ctx, "schnorr_sign", schnorr_sign_kernel, dim3((unsigned)((count + 255) / 256)), block, 0, P, d_sk, d_pk, d_k, d_msg, msg_len,
                   count, d_out, d_bad);
    } else {
        const size_t lanes = count < SCH_CHUNK ? count : SCH_CHUNK;
        const size_t stride = (lanes + 63) & ~(size_t)63;
        uint32_t* d_tab = nullptr;
        SWM_TRY(scratch(ctx, "schnorr.tab", ED_LADDER_TABLE_WORDS * sizeof(uint32_t) * stride, (void**)&d_tab));
        for (size_t base = 0; base < count; base += SCH_CHUNK) {
            const size_t n = count - base < SCH_CHUNK ? count - base : SCH_CHUNK;
            const dim3 grid((unsigned)((n + 255) / 256));
            if (op == OP_VERIFY)
                SWM_LAUNCH(ctx, "schnorr_verify", schnorr_verify_kernel<false>, grid, block, 0, P, d_pk, d_sig, d_msg, msg_len, base, n, d_tab,
                           stride, d_out, d_bad);
            else
                SWM_LAUNCH(ctx, "schnorr_commitments", schnorr_verify_kernel<true>, grid, block, 0, P, d_pk, d_sig, d_msg, msg_len, base, n,
                           d_tab, stride, d_out, d_bad);
        }
    }
    unsigned bad = 0;
    SWM_HIP(ctx, hipMemcpyAsync(&bad, d_bad, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bad != 0xffffffffu)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: item %u%s holds a scalar >= the group order or a point off ed-on-BLS12-377", what, bad,
                       bad == 0xfffffffeu ? " (or a later one)" : "");
    SWM_HIP(ctx, hipMemcpyAsync(out, d_out, out_item * count, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWM_OK;
}

}  // namespace

extern "C" {

int swm_schnorr_create(swm_ctx* ctx, const uint8_t generator_xy[64], const uint8_t* salt32_or_null, swm_schnorr** out) {
    if (!ctx || !generator_xy || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "schnorr_create: bad arguments");
    SWM_ON_DEVICE(ctx);
    swm_schnorr* p = new swm_schnorr;
    if (salt32_or_null) {
        words_from_bytes(salt32_or_null, p->salt);
        p->has_salt = true;
    }
    const SchnorrDev P = dev_params(p);
    uint32_t gx[8], gy[8];
    words_from_bytes(generator_xy, gx);
    words_from_bytes(generator_xy + 32, gy);
    EdExt base;
    if (!ed_point_from_words(P.d, gx, gy, &base)) {
        delete p;
        return set_err(ctx, SWM_ERR_INVALID_ARG, "schnorr_create: the generator is not a point of ed-on-BLS12-377");
    }
    const int rc = ed_window_table_upload(ctx, base, P.k2d, &p->d_table, "schnorr_create");
    if (rc != SWM_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return SWM_OK;
}

void swm_schnorr_destroy(swm_ctx* ctx, swm_schnorr* p) {
    if (!p) return;
    DeviceGuard guard(ctx);
    if (ctx) drain_streams(ctx);
    if (p->d_table) (void)hipFree(p->d_table);
    delete p;
}

int swm_schnorr_keygen(swm_ctx* ctx, const swm_schnorr* p, const uint8_t* secret_keys, size_t count, uint8_t* public_keys_xy) {
    if (!ctx || !p || (count && (!secret_keys || !public_keys_xy))) return set_err(ctx, SWM_ERR_INVALID_ARG, "schnorr_keygen: bad arguments");
    SWM_ON_DEVICE(ctx);
    if (!count) return SWM_OK;
    return schnorr_run(ctx, p, OP_KEYGEN, secret_keys, nullptr, nullptr, nullptr, nullptr, 0, count, public_keys_xy, "schnorr_keygen");
}

int swm_schnorr_sign(swm_ctx* ctx, const swm_schnorr* p, const uint8_t* secret_keys, const uint8_t* public_keys_xy, const uint8_t* nonces,
                     const uint8_t* messages, size_t msg_len, size_t count, uint8_t* signatures) {
    if (!ctx || !p || (count && (!secret_keys || !public_keys_xy || !nonces || !signatures || (msg_len && !messages))))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "schnorr_sign: bad arguments");
    SWM_ON_DEVICE(ctx);
    if (!count) return SWM_OK;
    return schnorr_run(ctx, p, OP_SIGN, secret_keys, public_keys_xy, nonces, nullptr, msg_len ? messages : nullptr, msg_len, count, signatures,
                       "schnorr_sign");
}

int swm_schnorr_verify(swm_ctx* ctx, const swm_schnorr* p, const uint8_t* public_keys_xy, const uint8_t* messages, size_t msg_len,
                       const uint8_t* signatures, size_t count, uint8_t* ok) {
    if (!ctx || !p || (count && (!public_keys_xy || !signatures || !ok || (msg_len && !messages))))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "schnorr_verify: bad arguments");
    SWM_ON_DEVICE(ctx);
    if (!count) return SWM_OK;
    return schnorr_run(ctx, p, OP_VERIFY, nullptr, public_keys_xy, nullptr, signatures, msg_len ? messages : nullptr, msg_len, count, ok,
                       "schnorr_verify");
}

int swm_schnorr_commitments(swm_ctx* ctx, const swm_schnorr* p, const uint8_t* public_keys_xy, const uint8_t* signatures, size_t count,
                            uint8_t* commitments_xy) {
    if (!ctx || !p || (count && (!public_keys_xy || !signatures || !commitments_xy)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "schnorr_commitments: bad arguments");
    SWM_ON_DEVICE(ctx);
    if (!count) return SWM_OK;
    return schnorr_run(ctx, p, OP_COMMIT, nullptr, public_keys_xy, nullptr, signatures, nullptr, 0, count, commitments_xy, "schnorr_commitments");
}

}  // extern "C"

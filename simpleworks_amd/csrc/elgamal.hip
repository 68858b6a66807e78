// elgamal.hip — ElGamal encryption on ed-on-BLS12-377, batched: keygen, encrypt and decrypt with one lane per item.
//
// What the reference exercises (tests/encrypt.rs:11-28, ElGamal<EdwardsProjective> of ark-crypto-primitives 0.3,
// encryption/elgamal/mod.rs [U], one call per item):
//   setup    generator = C::rand(rng)                        a random point of the prime subgroup, not the Schnorr generator
//   keygen   sk = ScalarField::rand, pk = sk G
//   encrypt  s = r pk, c1 = r G, c2 = m + s                  the ciphertext is (c1, c2), both affine
//   decrypt  s = sk c1, m = c2 + (-s)
// to_bytes! of an affine point is x || y, 32 little-endian bytes each in standard form [U].
//
// On the GPU.  The scalar multiplications are ed_mul.cuh's, shared with schnorr.hip: sk G and r G walk the table of the
// generator's window multiples; r pk_i and sk_i c1_i, whose point differs per item, run the signed-digit ladder over a per-item
// table in the global scratch buffer.  Encrypting MANY messages to ONE recipient is the case every real user has: the recipient's
// key is then tabulated once (swm_elgamal_key), r G and r PK become two table walks fused in one loop over the bytes of r, and
// the 252-doubling ladder, its table and its scratch buffer disappear.  An encryption yields two points: both go to affine form
// with one inversion (ed_affine2).
// The addition law is complete (ed.cuh): the identity, points of order 2 and 4, on-curve points outside the prime subgroup,
// r = 0 and sk = 0 take the common path.  pk.mul(r) of arkworks is the integer multiple with r < l, and so is the ladder's, so
// results agree on every on-curve point.
#include <hip/hip_runtime.h>

#include "context.h"
#include <string.h>

#include "ed_mul.cuh"
#include "elgamal.h"
#include "swmarlin.h"

namespace swm {

// what a kernel needs of the curve, and of a swm_elgamal when it has one
struct ElGamalDev {
    const EdRow* table;  // [32 windows][256]: row (w, v) = v 2^(8 w) G
    Fr k2d, d;
};

// x || y at `xy` -> the point (Z = 1), or false when it is refused
SWM_HD bool elgamal_load_point(const ElGamalDev& P, const uint8_t* xy, EdExt* out) {
    uint32_t xs[8], ys[8];
    load_words(xy, xs);
    load_words(xy + 32, ys);
    return ed_point_from_words(P.d, xs, ys, out);
}
SWM_HD void elgamal_store_ciphertext(const EdExt& c1, const EdExt& c2, uint8_t* out) {
    uint32_t c1x[8], c1y[8], c2x[8], c2y[8];
#if defined(SWM_ELGAMAL_TWO_INVERSIONS)  // the A/B build of DESIGN §3.5b: not what the library ships
    ed_affine(c1, c1x, c1y);
    ed_affine(c2, c2x, c2y);
#else
    ed_affine2(c1, c2, c1x, c1y, c2x, c2y);
#endif
    store_words(out, c1x);
    store_words(out + 32, c1y);
    store_words(out + 64, c2x);
    store_words(out + 96, c2y);
}

// ---------------------------------------------------------------------------------------------- the lane functions
// (c1, c2) = (r G, m + r pk) for a per-item pk: ladder, one unified addition, table walk.  false: refused.
SWM_HD bool elgamal_encrypt_lane(const ElGamalDev& P, const uint8_t* pk_xy, const uint8_t* m_xy, const uint8_t* r32, uint32_t* tab,
                                 size_t stride, uint8_t* out128) {
    uint32_t r[8];
    load_words(r32, r);
    EdExt pk, m;
    if (!sc_is_canonical(r) || !elgamal_load_point(P, pk_xy, &pk) || !elgamal_load_point(P, m_xy, &m)) return false;
    EdExt c2 = ed_ladder_mul(pk, r, P.k2d, tab, stride);
    ed_add_cached(c2, ed_to_cached(m, P.k2d));
    EdExt c1 = ed_identity();
    ed_fixed_mul(c1, P.table, r);
    elgamal_store_ciphertext(c1, c2, out128);
    return true;
}

// the same under a tabulated key: byte w of r picks row (w, byte) of both tables; c2 starts at m
SWM_HD bool elgamal_encrypt_to_lane(const ElGamalDev& P, const EdRow* key_table, const uint8_t* m_xy, const uint8_t* r32, uint8_t* out128) {
    uint32_t t[8];
    load_words(r32, t);
    EdExt c2;
    if (!sc_is_canonical(t) || !elgamal_load_point(P, m_xy, &c2)) return false;
    EdExt c1 = ed_identity();
#pragma unroll 1
    for (unsigned w = 0; w < ED_WINDOWS; w++) {
        const unsigned v = t[0] & 255u;
#pragma unroll
        for (int i = 0; i < 7; i++) t[i] = (t[i] >> 8) | (t[i + 1] << 24);
        t[7] >>= 8;
        if (v) {
            ed_madd(c1, P.table[(w << 8) + v]);
            ed_madd(c2, key_table[(w << 8) + v]);
        }
    }
    elgamal_store_ciphertext(c1, c2, out128);
    return true;
}

// m = c2 - sk c1: the ladder, its result negated (X and T change sign), one unified addition
SWM_HD bool elgamal_decrypt_lane(const ElGamalDev& P, const uint8_t* sk32, const uint8_t* ct128, uint32_t* tab, size_t stride,
                                 uint8_t* out64) {
    uint32_t sk[8], mx[8], my[8];
    load_words(sk32, sk);
    EdExt c1, c2;
    if (!sc_is_canonical(sk) || !elgamal_load_point(P, ct128, &c1) || !elgamal_load_point(P, ct128 + 64, &c2)) return false;
    EdExt s = ed_ladder_mul(c1, sk, P.k2d, tab, stride);
    s.x = fp_neg(s.x);
    s.t = fp_neg(s.t);
    ed_add_cached(s, ed_to_cached(c2, P.k2d));
    ed_affine(s, mx, my);
    store_words(out64, mx);
    store_words(out64 + 32, my);
    return true;
}

// ---------------------------------------------------------------------------------------------- kernels: one lane per item
// A refused input lowers *bad (refuse, ed_mul.cuh); the host then returns without copying anything out.
__global__ void __launch_bounds__(256) elgamal_keygen_kernel(ElGamalDev P, const uint8_t* __restrict__ secrets, size_t count,
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

// items [base, base + n); lane j of the launch owns column j of `tab`
__global__ void __launch_bounds__(256) elgamal_encrypt_kernel(ElGamalDev P, const uint8_t* __restrict__ pks, const uint8_t* __restrict__ msgs,
                                                              const uint8_t* __restrict__ rs, size_t base, size_t n,
                                                              uint32_t* __restrict__ tab, size_t stride, uint8_t* __restrict__ out,
                                                              unsigned* __restrict__ bad) {
    const size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const size_t i = base + j;
    if (!elgamal_encrypt_lane(P, pks + 64 * i, msgs + 64 * i, rs + 32 * i, tab + j, stride, out + 128 * i)) refuse(bad, i);
}

__global__ void __launch_bounds__(256) elgamal_encrypt_to_kernel(ElGamalDev P, const EdRow* __restrict__ key_table,
                                                                 const uint8_t* __restrict__ msgs, const uint8_t* __restrict__ rs,
                                                                 size_t count, uint8_t* __restrict__ out, unsigned* __restrict__ bad) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= count) return;
    if (!elgamal_encrypt_to_lane(P, key_table, msgs + 64 * i, rs + 32 * i, out + 128 * i)) refuse(bad, i);
}

__global__ void __launch_bounds__(256) elgamal_decrypt_kernel(ElGamalDev P, const uint8_t* __restrict__ sks, const uint8_t* __restrict__ cts,
                                                              size_t base, size_t n, uint32_t* __restrict__ tab, size_t stride,
                                                              uint8_t* __restrict__ out, unsigned* __restrict__ bad) {
    const size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const size_t i = base + j;
    if (!elgamal_decrypt_lane(P, sks + 32 * i, cts + 128 * i, tab + j, stride, out + 64 * i)) refuse(bad, i);
}

}  // namespace swm

using namespace swm;

namespace {

ElGamalDev dev_params(const swm_elgamal* p) {
    ElGamalDev d;
    d.table = p ? reinterpret_cast<const EdRow*>(p->d_table) : nullptr;
    d.k2d = fp_from_u64<Fr>(2 * ED_D);
    d.d = fp_from_u64<Fr>(ED_D);
    return d;
}

enum ElGamalOp { OP_KEYGEN, OP_ENCRYPT, OP_ENCRYPT_TO, OP_DECRYPT };

// Stages the inputs (each array starts at a multiple of 32 count bytes: word-aligned), runs the kernel of `op`, and copies the
// result out only when no input was refused.  The ladder's kernels run in launches of at most ED_LADDER_CHUNK items, as Schnorr's
// verification does, over the same table buffer.
int elgamal_run(swm_ctx* ctx, const swm_elgamal* p, const swm_elgamal_key* key, ElGamalOp op, const uint8_t* scalars, const uint8_t* pks,
                const uint8_t* msgs, const uint8_t* cts, size_t count, uint8_t* out, const char* what) {
    const size_t out_item = op == OP_ENCRYPT || op == OP_ENCRYPT_TO ? 128 : 64;
    const size_t n_sc = 32 * count, n_pk = pks ? 64 * count : 0, n_m = msgs ? 64 * count : 0, n_ct = cts ? 128 * count : 0;
    uint8_t *d_in = nullptr, *d_res = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", n_sc + n_pk + n_m + n_ct + 32, (void**)&d_in));
    SWM_TRY(scratch(ctx, "stage.b", 256 + out_item * count, (void**)&d_res));
    uint8_t *d_sc = d_in, *d_pk = d_sc + n_sc, *d_m = d_pk + n_pk, *d_ct = d_m + n_m;
    unsigned* d_bad = reinterpret_cast<unsigned*>(d_res);
    uint8_t* d_out = d_res + 256;
    SWM_HIP(ctx, hipMemcpyAsync(d_sc, scalars, n_sc, hipMemcpyHostToDevice, ctx->stream));
    if (n_pk) SWM_HIP(ctx, hipMemcpyAsync(d_pk, pks, n_pk, hipMemcpyHostToDevice, ctx->stream));
    if (n_m) SWM_HIP(ctx, hipMemcpyAsync(d_m, msgs, n_m, hipMemcpyHostToDevice, ctx->stream));
    if (n_ct) SWM_HIP(ctx, hipMemcpyAsync(d_ct, cts, n_ct, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemsetAsync(d_bad, 0xff, sizeof(unsigned), ctx->stream));
    const ElGamalDev P = dev_params(p);
    const dim3 block(256);
    if (op == OP_KEYGEN) {
        SWM_LAUNCH(ctx, "elgamal_keygen", elgamal_keygen_kernel, dim3((unsigned)((count + 255) / 256)), block, 0, P, d_sc, count, d_out, d_bad);
    } else if (op == OP_ENCRYPT_TO) {
        SWM_LAUNCH(ctx, "elgamal_encrypt_to", elgamal_encrypt_to_kernel, dim3((unsigned)((count + 255) / 256)), block, 0, P,
                   reinterpret_cast<const EdRow*>(key->d_table), d_m, d_sc, count, d_out, d_bad);
    } else {
        const size_t lanes = count < ED_LADDER_CHUNK ? count : ED_LADDER_CHUNK;
        const size_t stride = (lanes + 63) & ~(size_t)63;
        uint32_t* d_tab = nullptr;
        SWM_TRY(scratch(ctx, "schnorr.tab", ED_LADDER_TABLE_WORDS * sizeof(uint32_t) * stride, (void**)&d_tab));
        for (size_t base = 0; base < count; base += ED_LADDER_CHUNK) {
            const size_t n = count - base < ED_LADDER_CHUNK ? count - base : ED_LADDER_CHUNK;
            const dim3 grid((unsigned)((n + 255) / 256));
            if (op == OP_ENCRYPT)
                SWM_LAUNCH(ctx, "elgamal_encrypt", elgamal_encrypt_kernel, grid, block, 0, P, d_pk, d_m, d_sc, base, n, d_tab, stride, d_out,
                           d_bad);
            else
                SWM_LAUNCH(ctx, "elgamal_decrypt", elgamal_decrypt_kernel, grid, block, 0, P, d_sc, d_ct, base, n, d_tab, stride, d_out, d_bad);
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

// the resident table of the point `xy`, or SWM_ERR_INVALID_ARG when it is not on the curve
int table_of(swm_ctx* ctx, const uint8_t xy[64], void** d_table, const char* what) {
    const ElGamalDev P = dev_params(nullptr);
    uint32_t xs[8], ys[8];
    words_from_bytes(xy, xs);
    words_from_bytes(xy + 32, ys);
    EdExt base;
    if (!ed_point_from_words(P.d, xs, ys, &base)) return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: not a point of ed-on-BLS12-377", what);
    return ed_window_table_upload(ctx, base, P.k2d, d_table, what);
}

template <class T> int create(swm_ctx* ctx, const uint8_t xy[64], T** out, const char* what) {
    if (!ctx || !xy || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what);
    SWM_ON_DEVICE(ctx);
    T* p = new T;
    const int rc = table_of(ctx, xy, &p->d_table, what);
    if (rc != SWM_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return SWM_OK;
}

template <class T> void destroy(swm_ctx* ctx, T* p) {
    if (!p) return;
    DeviceGuard guard(ctx);
    if (ctx) drain_streams(ctx);
    if (p->d_table) (void)hipFree(p->d_table);
    delete p;
}

}  // namespace

extern "C" {

int swm_elgamal_create(swm_ctx* ctx, const uint8_t generator_xy[64], swm_elgamal** out) { return create(ctx, generator_xy, out, "elgamal_create"); }

void swm_elgamal_destroy(swm_ctx* ctx, swm_elgamal* p) { destroy(ctx, p); }

int swm_elgamal_key_create(swm_ctx* ctx, const uint8_t public_key_xy[64], swm_elgamal_key** out) {
    SWM_TRY(create(ctx, public_key_xy, out, "elgamal_key_create"));
    memcpy((*out)->xy, public_key_xy, 64);  // canonical and on the curve: table_of accepted it
    return SWM_OK;
}

void swm_elgamal_key_destroy(swm_ctx* ctx, swm_elgamal_key* key) { destroy(ctx, key); }

int swm_elgamal_keygen(swm_ctx* ctx, const swm_elgamal* p, const uint8_t* secret_keys, size_t count, uint8_t* public_keys_xy) {
    if (!ctx || !p || (count && (!secret_keys || !public_keys_xy))) return set_err(ctx, SWM_ERR_INVALID_ARG, "elgamal_keygen: bad arguments");
    SWM_ON_DEVICE(ctx);
    if (!count) return SWM_OK;
    return elgamal_run(ctx, p, nullptr, OP_KEYGEN, secret_keys, nullptr, nullptr, nullptr, count, public_keys_xy, "elgamal_keygen");
}

int swm_elgamal_encrypt(swm_ctx* ctx, const swm_elgamal* p, const uint8_t* public_keys_xy, const uint8_t* messages_xy, const uint8_t* randomness,
                        size_t count, uint8_t* ciphertexts) {
    if (!ctx || !p || (count && (!public_keys_xy || !messages_xy || !randomness || !ciphertexts)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "elgamal_encrypt: bad arguments");
    SWM_ON_DEVICE(ctx);
    if (!count) return SWM_OK;
    return elgamal_run(ctx, p, nullptr, OP_ENCRYPT, randomness, public_keys_xy, messages_xy, nullptr, count, ciphertexts, "elgamal_encrypt");
}

int swm_elgamal_encrypt_to(swm_ctx* ctx, const swm_elgamal* p, const swm_elgamal_key* key, const uint8_t* messages_xy, const uint8_t* randomness,
                           size_t count, uint8_t* ciphertexts) {
    if (!ctx || !p || !key || (count && (!messages_xy || !randomness || !ciphertexts)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "elgamal_encrypt_to: bad arguments");
    SWM_ON_DEVICE(ctx);
    if (!count) return SWM_OK;
    return elgamal_run(ctx, p, key, OP_ENCRYPT_TO, randomness, nullptr, messages_xy, nullptr, count, ciphertexts, "elgamal_encrypt_to");
}

int swm_elgamal_decrypt(swm_ctx* ctx, const uint8_t* secret_keys, const uint8_t* ciphertexts, size_t count, uint8_t* messages_xy) {
    if (!ctx || (count && (!secret_keys || !ciphertexts || !messages_xy))) return set_err(ctx, SWM_ERR_INVALID_ARG, "elgamal_decrypt: bad arguments");
    SWM_ON_DEVICE(ctx);
    if (!count) return SWM_OK;
    return elgamal_run(ctx, nullptr, nullptr, OP_DECRYPT, secret_keys, nullptr, nullptr, ciphertexts, count, messages_xy, "elgamal_decrypt");
}

}  // extern "C"

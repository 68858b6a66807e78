// ed_mul.cuh — scalar multiplication on ed-on-BLS12-377 one lane per item: what schnorr.hip and elgamal.hip share.
//   * the scalar field's canonical test (order l, 251 bits);
//   * points and scalars in and out of the wire form (x || y, 32 little-endian bytes each in standard form);
//   * s G from a table of the base's window multiples, 32 windows of 8 bits (768 KB, resident in L2): one mixed addition per
//     non-zero byte of s (ed_fixed_mul), and the host function that fills such a table for any on-curve base;
//   * e Y for a per-item point: a signed 4-bit-digit ladder over a per-item table of 1 Y .. 8 Y in cached form.  e + 0x0777..7
//     read nibble by nibble gives the 63 digits nibble - 7 in [-7, 8], so there is no carry chain; 4 doublings and at most one
//     addition per digit.  That table is 1 KB per lane and indexed at run time, so it lives in a global buffer laid out
//     [entry][word][item]: lanes that pick the same entry read neighbouring words;
//   * one inversion per item (frinv.cuh) for one affine point, or for two that share it.
// The addition law is complete (ed.cuh): the identity, doublings, points of order 2 and 4, points outside the prime subgroup and
// the scalar 0 take the common path.  The lane functions are host and device: on a CPU they run as written (fp_inv for the inverse).
#pragma once
#include <vector>

#include "context.h"
#include "ed.cuh"
#include "ff.cuh"
#include "frinv.cuh"

namespace swm {

// ---------------------------------------------------------------------------------------------- the scalar field
struct EdScalar {  // l = 2111115437357092606062206234695386632838870926408408195193685246394721360383, little-endian words
    static constexpr uint32_t L[8] = {0xc33fd9ffu, 0xb95aee9au, 0xc43c8afeu, 0x5293a3afu, 0x970dec00u, 0x982d1347u, 0xa68b2955u, 0x04aad957u};
};
// word i of l 2^k, k <= 5 (l < 2^251)
SWM_HD constexpr uint32_t sc_l_shifted(int i, int k) {
    return k == 0 ? EdScalar::L[i] : (EdScalar::L[i] << k) | (i ? EdScalar::L[i - 1] >> (32 - k) : 0u);
}
// a -= l 2^K when that does not go negative; returns whether it subtracted
template <int K> SWM_HD bool sc_cond_sub(uint32_t (&a)[8]) {
    uint32_t d[8], borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t t = (uint64_t)a[i] - sc_l_shifted(i, K) - borrow;
        d[i] = (uint32_t)t;
        borrow = (uint32_t)(t >> 63);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) a[i] = borrow ? a[i] : d[i];
    return borrow == 0;
}
SWM_HD bool sc_is_canonical(const uint32_t (&a)[8]) {
    uint32_t t[8];
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = a[i];
    return !sc_cond_sub<0>(t);
}

// ---------------------------------------------------------------------------------------------- points in and out
SWM_HD void load_words(const uint8_t* p, uint32_t (&w)[8]) {  // p is 4-byte aligned (the staging layouts of the callers)
    const uint32_t* s = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = s[i];
}
SWM_HD void store_words(uint8_t* p, const uint32_t (&w)[8]) {
    uint32_t* d = reinterpret_cast<uint32_t*>(p);
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = w[i];
}
SWM_HD bool fr_from_words(const uint32_t (&w)[8], Fr* out) {  // canonical (< r) or refused
    Fr s, r;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        s.v[i] = w[i];
        r.v[i] = FrParams::P[i];
    }
    if (fp_cmp_std(s, r) >= 0) return false;
    *out = fp_from_std(s);
    return true;
}
// x || y (standard form) -> the point, or false when a coordinate is >= r or -x^2 + y^2 != 1 + d x^2 y^2
SWM_HD bool ed_point_from_words(const Fr& d, const uint32_t (&xs)[8], const uint32_t (&ys)[8], EdExt* out) {
    Fr x, y;
    if (!fr_from_words(xs, &x) || !fr_from_words(ys, &y)) return false;
    Fr x2 = fp_sqr(x), y2 = fp_sqr(y);
    if (!fp_eq(fp_sub(y2, x2), fp_add(fp_one<Fr>(), fp_mul(d, fp_mul(x2, y2))))) return false;
    out->x = x;
    out->y = y;
    out->t = fp_mul(x, y);
    out->z = fp_one<Fr>();
    return true;
}
SWM_HD Fr ed_inv(const Fr& z) {  // z != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return fr_inv_single(z);
#else
    return fp_inv(z);  // (host: the lane functions of this file also run on a CPU, which is how they were first checked)
#endif
}
SWM_HD void ed_affine_words(const EdExt& p, const Fr& zi, uint32_t (&xs)[8], uint32_t (&ys)[8]) {
    const Fr x = fp_to_std(fp_mul(p.x, zi)), y = fp_to_std(fp_mul(p.y, zi));
#pragma unroll
    for (int i = 0; i < 8; i++) {
        xs[i] = x.v[i];
        ys[i] = y.v[i];
    }
}
SWM_HD void ed_affine(const EdExt& p, uint32_t (&xs)[8], uint32_t (&ys)[8]) {
    ed_affine_words(p, ed_inv(p.z), xs, ys);  // Z != 0: the law is complete
}
// two points, one inversion: 1 / (Z1 Z2), then Z2 / (Z1 Z2) = 1 / Z1 and Z1 / (Z1 Z2) = 1 / Z2
SWM_HD void ed_affine2(const EdExt& p, const EdExt& q, uint32_t (&pxs)[8], uint32_t (&pys)[8], uint32_t (&qxs)[8], uint32_t (&qys)[8]) {
    const Fr zi = ed_inv(fp_mul(p.z, q.z));
    ed_affine_words(p, fp_mul(zi, q.z), pxs, pys);
    ed_affine_words(q, fp_mul(zi, p.z), qxs, qys);
}

// ---------------------------------------------------------------------------------------------- a tabulated base
constexpr unsigned ED_WINDOWS = 32, ED_ROWS = 256;

// acc += s G: byte w of s picks row (w, byte) of G's table
SWM_HD void ed_fixed_mul(EdExt& acc, const EdRow* table, const uint32_t (&s)[8]) {
    uint32_t t[8];
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = s[i];
#pragma unroll 1
    for (unsigned w = 0; w < ED_WINDOWS; w++) {
        const unsigned v = t[0] & 255u;
#pragma unroll
        for (int i = 0; i < 7; i++) t[i] = (t[i] >> 8) | (t[i + 1] << 24);
        t[7] >>= 8;
        if (v) ed_madd(acc, table[(w << 8) + v]);
    }
}

// the table of an on-curve base (host): row (w, v) = v 2^(8 w) base, for any point of the curve
inline std::vector<EdRow> ed_window_table(EdExt base, const Fr& k2d) {
    std::vector<EdRow> rows((size_t)ED_WINDOWS * ED_ROWS);
    for (unsigned w = 0; w < ED_WINDOWS; w++) {  // base = 2^(8 w) G
        EdExt acc = ed_identity();
        for (unsigned v = 0; v < ED_ROWS; v++) {  // acc = v base
            const Fr zi = fp_inv(acc.z);
            const Fr x = fp_mul(acc.x, zi), y = fp_mul(acc.y, zi);
            EdRow& r = rows[(size_t)w * ED_ROWS + v];
            r.ymx = fp_sub(y, x);
            r.ypx = fp_add(y, x);
            r.kt = fp_mul(k2d, fp_mul(x, y));
            acc = ed_add(acc, base, k2d);
        }
        base = acc;  // 256 base
    }
    return rows;
}
// ... built and made resident: *d_table owns a device allocation on success (hipFree), and is NULL otherwise
inline int ed_window_table_upload(swm_ctx* ctx, const EdExt& base, const Fr& k2d, void** d_table, const char* what) {
    const std::vector<EdRow> rows = ed_window_table(base, k2d);
    *d_table = nullptr;
    hipError_t e = hipMalloc(d_table, rows.size() * sizeof(EdRow));
    if (e == hipSuccess) e = hipMemcpyAsync(*d_table, rows.data(), rows.size() * sizeof(EdRow), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // `rows` goes out of scope
    if (e != hipSuccess) {
        if (*d_table) (void)hipFree(*d_table);
        *d_table = nullptr;
        (void)hipGetLastError();
        return set_err(ctx, e == hipErrorOutOfMemory ? SWM_ERR_OOM : SWM_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    }
    return SWM_OK;
}

// ---------------------------------------------------------------------------------------------- a per-item point
constexpr size_t ED_LADDER_CHUNK = (size_t)1 << 18;  // items per launch of a kernel that runs the ladder: bounds the table buffer at 256 MB
constexpr size_t ED_LADDER_TABLE_WORDS = 8 * 32;     // per item

// the per-item table: entry k (k + 1 times Y, cached form) is 32 words, word j at tab[(32 k + j) stride]
SWM_HD void cached_store(uint32_t* tab, size_t stride, unsigned k, const EdCached& c) {
    uint32_t* p = tab + (size_t)32 * k * stride;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        p[(size_t)i * stride] = c.ymx.v[i];
        p[(size_t)(8 + i) * stride] = c.ypx.v[i];
        p[(size_t)(16 + i) * stride] = c.kt.v[i];
        p[(size_t)(24 + i) * stride] = c.z2.v[i];
    }
}
SWM_HD EdCached cached_load(const uint32_t* tab, size_t stride, unsigned k) {
    const uint32_t* p = tab + (size_t)32 * k * stride;
    EdCached c;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c.ymx.v[i] = p[(size_t)i * stride];
        c.ypx.v[i] = p[(size_t)(8 + i) * stride];
        c.kt.v[i] = p[(size_t)(16 + i) * stride];
        c.z2.v[i] = p[(size_t)(24 + i) * stride];
    }
    return c;
}

// e Y, e < l: the integer multiple, for any on-curve Y.  `tab` is this lane's column of the table buffer.
SWM_HD EdExt ed_ladder_mul(const EdExt& Y, const uint32_t (&e)[8], const Fr& k2d, uint32_t* tab, size_t stride) {
    const EdCached c1 = ed_to_cached(Y, k2d);
    cached_store(tab, stride, 0, c1);
    EdExt run = Y;
#pragma unroll 1
    for (unsigned k = 1; k < 8; k++) {
        ed_add_cached(run, c1);
        cached_store(tab, stride, k, ed_to_cached(run, k2d));
    }
    // e + 0x0777..7 < 2^251 + 2^251: 63 nibbles, nibble i - 7 = digit i in [-7, 8], sum of digit i 16^i = e
    uint32_t d[8], carry = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t t = (uint64_t)e[i] + (i == 7 ? 0x07777777u : 0x77777777u) + carry;
        d[i] = (uint32_t)t;
        carry = (uint32_t)(t >> 32);
    }
#pragma unroll
    for (int i = 7; i > 0; i--) d[i] = (d[i] << 4) | (d[i - 1] >> 28);  // nibble 63 is zero: start at nibble 62
    d[0] <<= 4;
    EdExt acc = ed_identity();
#pragma unroll 1
    for (int i = 0; i < 63; i++) {
        if (i) {
#pragma unroll 1
            for (int j = 0; j < 4; j++) ed_dbl(acc);
        }
        const int dg = (int)(d[7] >> 28) - 7;
#pragma unroll
        for (int k = 7; k > 0; k--) d[k] = (d[k] << 4) | (d[k - 1] >> 28);
        d[0] <<= 4;
        if (dg) {
            EdCached c = cached_load(tab, stride, (unsigned)(dg < 0 ? -dg : dg) - 1u);
            if (dg < 0) c = ed_cached_neg(c);
            ed_add_cached(acc, c);
        }
    }
    return acc;
}

// ---------------------------------------------------------------------------------------------- refusing a call
#if defined(__HIPCC__)
// A refused input lowers *bad to the smallest refused index (0xffffffff: none); the host then returns without copying anything out.
__device__ __forceinline__ void refuse(unsigned* bad, size_t i) { atomicMin(bad, (unsigned)(i < 0xfffffffeu ? i : 0xfffffffeu)); }
#endif

inline void words_from_bytes(const uint8_t* b, uint32_t (&w)[8]) {
    for (int i = 0; i < 8; i++) w[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
}

}  // namespace swm

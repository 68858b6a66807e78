// ed.cuh — ed-on-BLS12-377 (-x^2 + y^2 = 1 + 3021 x^2 y^2 over BLS12-377 Fr) in extended coordinates: what pedersen.hip and
// schnorr.hip share.  a = -1 is a square and d = 3021 a non-square in Fr, so the unified law below is complete: the identity,
// doublings and the points of order 2 and 4 take the same formulas as everything else, and no caller special-cases them.
#pragma once
#include "ff.cuh"

namespace swm {

struct EdExt {
    Fr x, y, t, z;
};
struct EdRow {  // an affine point as the mixed addition wants it; the identity is (1, 1, 0)
    Fr ymx, ypx, kt;
};
static constexpr uint64_t ED_D = 3021;

SWM_HD EdExt ed_identity() {
    EdExt p;
    p.x = fp_zero<Fr>();
    p.y = fp_one<Fr>();
    p.t = fp_zero<Fr>();
    p.z = fp_one<Fr>();
    return p;
}
// add-2008-hwcd-3 (a = -1), 8 multiplications + one by 2d
SWM_HD EdExt ed_add(const EdExt& p, const EdExt& q, const Fr& k2d) {
    Fr a = fp_mul(fp_sub(p.y, p.x), fp_sub(q.y, q.x));
    Fr b = fp_mul(fp_add(p.y, p.x), fp_add(q.y, q.x));
    Fr c = fp_mul(fp_mul(p.t, k2d), q.t);
    Fr d = fp_dbl(fp_mul(p.z, q.z));
    Fr e = fp_sub(b, a), f = fp_sub(d, c), g = fp_add(d, c), h = fp_add(b, a);
    EdExt r;
    r.x = fp_mul(e, f);
    r.y = fp_mul(g, h);
    r.t = fp_mul(e, h);
    r.z = fp_mul(f, g);
    return r;
}
// madd-2008-hwcd-3 against a tabulated affine point: 7 multiplications
SWM_HD void ed_madd(EdExt& p, const EdRow& q) {
    Fr a = fp_mul(fp_sub(p.y, p.x), q.ymx);
    Fr b = fp_mul(fp_add(p.y, p.x), q.ypx);
    Fr c = fp_mul(p.t, q.kt);
    Fr d = fp_dbl(p.z);
    Fr e = fp_sub(b, a), f = fp_sub(d, c), g = fp_add(d, c), h = fp_add(b, a);
    p.x = fp_mul(e, f);
    p.y = fp_mul(g, h);
    p.t = fp_mul(e, h);
    p.z = fp_mul(f, g);
}

__device__ __forceinline__ EdExt ed_shfl_xor(const EdExt& p, int mask) {
    EdExt r;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(&p);
    uint32_t* d = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(EdExt) / 4); i++) d[i] = (uint32_t)__shfl_xor((int)s[i], mask, 64);
    return r;
}

// dbl-2008-hwcd (a = -1): 4 squares + 4 multiplications.  With A = X^2, B = Y^2, C = 2 Z^2: E = (X + Y)^2 - A - B,
// G = B - A, F = G - C, H = -A - B.  Z3 = F G != 0 on the curve (y^2 - x^2 = 1 + d x^2 y^2 != 0, and F / Z^2 is the
// other denominator of the unified law), so this too holds for every point.
SWM_HD void ed_dbl(EdExt& p) {
    Fr a = fp_sqr(p.x), b = fp_sqr(p.y);
    Fr c = fp_dbl(fp_sqr(p.z));
    Fr s = fp_add(a, b);
    Fr e = fp_sub(fp_sqr(fp_add(p.x, p.y)), s);
    Fr g = fp_sub(b, a), f = fp_sub(g, c), h = fp_neg(s);
    p.x = fp_mul(e, f);
    p.y = fp_mul(g, h);
    p.t = fp_mul(e, h);
    p.z = fp_mul(f, g);
}

// A projective point as the addition wants its second operand ("cached"): what add-2008-hwcd-3 derives from (X2 : Y2 : T2 : Z2)
// before its four final products.  8 multiplications per addition, none spent on the operand.
struct EdCached {
    Fr ymx, ypx, kt, z2;  // Y - X, Y + X, 2 d T, 2 Z
};
SWM_HD EdCached ed_to_cached(const EdExt& p, const Fr& k2d) {
    EdCached c;
    c.ymx = fp_sub(p.y, p.x);
    c.ypx = fp_add(p.y, p.x);
    c.kt = fp_mul(p.t, k2d);
    c.z2 = fp_dbl(p.z);
    return c;
}
SWM_HD void ed_add_cached(EdExt& p, const EdCached& q) {
    Fr a = fp_mul(fp_sub(p.y, p.x), q.ymx);
    Fr b = fp_mul(fp_add(p.y, p.x), q.ypx);
    Fr c = fp_mul(p.t, q.kt);
    Fr d = fp_mul(p.z, q.z2);
    Fr e = fp_sub(b, a), f = fp_sub(d, c), g = fp_add(d, c), h = fp_add(b, a);
    p.x = fp_mul(e, f);
    p.y = fp_mul(g, h);
    p.t = fp_mul(e, h);
    p.z = fp_mul(f, g);
}
// -(x, y) = (-x, y): Y - X and Y + X change places, T changes sign
SWM_HD EdCached ed_cached_neg(const EdCached& q) {
    EdCached r;
    r.ymx = q.ypx;
    r.ypx = q.ymx;
    r.kt = fp_neg(q.kt);
    r.z2 = q.z2;
    return r;
}

}  // namespace swm

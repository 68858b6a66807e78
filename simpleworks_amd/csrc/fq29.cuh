// fq29.cuh — BLS12-377 Fq in 13 x 29-bit limbs with LAZY carries: the table rows and the accumulators of msm_accumulate_te.
//
// Why a second limb form: fq28.cuh needs fourteen limbs only because its limbs have 28 bits — Fq has 377 bits and
// 13 x 29 = 377.  A product here is 13 x 13 partial products plus 14 reduction steps x 12 limbs of p = 337 v_mad_u64_u32
// against 378 (404 instructions against 447), and every limb-wise addition, load and select is 13 long instead of 14.
// What it costs: a column of thirteen products of 29-bit limbs leaves less room in the 64-bit accumulator than fourteen of
// 28-bit ones, so two of the eight operands of the mixed addition's second round are carry-normalised first (below).
// The domain no longer ends at the accumulation: a job whose bucket stage works one lane per chain (msm_bucket_reduce<256, FormTE29>,
// msm_bucket_reduce_low) gets its partial sums as they stand in the accumulator — unpacked, no product spent on them — and adds them
// by the general addition at the end of this file (te29_slot_add); the workgroup results leave through te29_store_384 in the
// canonical radix-2^384 form the host fold and the wire formats always saw.  Only the quad bucket stage of small jobs (FormTEQuad)
// still adds in the 28-bit domain: for those jobs the accumulation's epilogue converts (te29_to_slot).
//
// Representation.  value = sum l[i] 2^(29 i); Montgomery radix 2^406 = 2^(29 x 14): FOURTEEN reduction steps for thirteen
// limbs, so that a product of two operands of several p comes back below p (1 + 2^-23) — with thirteen steps (radix 2^377,
// barely above p) lazy operands would not be absorbed.  p = 1 mod 2^46, so p_0 = 1 in this radix too and m_k is a negation.
// Forms:
//   C  canonical:   limbs < 2^29, value < p                                — table rows, constants
//   N  normalised:  limbs < 2^29, value < p (1 + 2^-23)                    — what fq29_mul returns for operands < 8p:
//        (a b + m p) / 2^406 with m < 2^406: < 64 p^2 / 2^406 + p, and p / 2^406 < 2^-29
//   L  lazy:        limbs < 2^32, value < 8p                               — what fq29_mul accepts, PROVIDED the column sums of
//        the particular pair of operands stay below 2^64 - 2^29.  Unlike fq28_mul there is no blanket limb bound that two
//        lazy operands may both reach: 13 x 2^29 x max|p_j| is 0.20 x 2^64 already, and two spread subtractions
//        (limbs up to 3 x 2^29) multiply to 1.83 x 2^64.  The bound of every product is therefore stated where it is formed,
//        and tools/check_te29.py evaluates each with every limb at its documented maximum (and emulates every limb
//        operation on random and extremal chains).
// Subtraction a - b is a + SPREADk - b, where SPREADk are the limbs of k p with 2^29 borrowed into every limb below the top
// one; b must be N or C for SPREAD2 (top limb of b <= p_12 + 1 < top limb of 2p), normalised and below 3p for SPREAD4.
#pragma once
#include "ff.cuh"
#include "g1.cuh"

namespace swm {

struct Fq29 {
    uint32_t l[13];
};
static constexpr uint32_t M29Q = (1u << 29) - 1;

struct Fq29Consts {
    static constexpr uint32_t P[13] = SWM_FQ29_P;
    static constexpr uint32_t ONE[13] = SWM_FQ29_ONE;
    static constexpr uint32_t TWO[13] = SWM_FQ29_TWO;
    static constexpr uint32_t INVD[13] = SWM_FQ29_TE_INVD;
    static constexpr uint32_t TO392[13] = SWM_FQ29_TO392;
    static constexpr uint32_t K2D[13] = SWM_FQ29_TE_2D;
    static constexpr uint32_t TO384[13] = SWM_FQ29_TO384;
    static constexpr uint32_t SPREAD2[13] = SWM_FQ29_SPREAD2;
    static constexpr uint32_t SPREAD4[13] = SWM_FQ29_SPREAD4;
};

__device__ __forceinline__ Fq29 fq29_const(const uint32_t (&c)[13]) {
    Fq29 r;
#pragma unroll
    for (int i = 0; i < 13; i++) r.l[i] = c[i];
    return r;
}
// 12 x 32-bit words (value < 2^377) -> 13 x 29-bit limbs
__device__ __forceinline__ Fq29 fq29_unpack(const Fq& a) {
    Fq29 r;
#pragma unroll
    for (int i = 0; i < 13; i++) {
        const int bit = 29 * i, w = bit >> 5, off = bit & 31;
        uint32_t v = a.v[w] >> off;
        if (off > 3 && w + 1 < 12) v |= a.v[w + 1] << (32 - off);
        r.l[i] = v & M29Q;
    }
    return r;
}
// limbs < 2^29 (value < 2^377) -> 12 words
__device__ __forceinline__ Fq fq29_pack(const Fq29& a) {
    Fq r;
#pragma unroll
    for (int w = 0; w < 12; w++) {
        const int bit = 32 * w, i = bit / 29, off = bit - 29 * i;
        uint32_t v = a.l[i] >> off;
        if (i + 1 < 13) v |= a.l[i + 1] << (29 - off);
        if (29 - off + 29 < 32 && i + 2 < 13) v |= a.l[i + 2] << (58 - off);
        r.v[w] = v;
    }
    return r;
}
// carry propagation: limbs < 2^32 in, limbs < 2^29 out (the top limb takes what is left)
__device__ __forceinline__ Fq29 fq29_normalize(const Fq29& a) {
    Fq29 r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const uint32_t t = a.l[i] + c;
        r.l[i] = t & M29Q;
        c = t >> 29;
    }
    r.l[12] = a.l[12] + c;
    return r;
}
__device__ __forceinline__ Fq29 fq29_add(const Fq29& a, const Fq29& b) {  // lazy: limbs add, no carry
    Fq29 r;
#pragma unroll
    for (int i = 0; i < 13; i++) r.l[i] = a.l[i] + b.l[i];
    return r;
}
// a - b + k p  (b: limbs < 2^29 below the top one, top limb below the spread's)
#define FQ29_SUB(a, b, SPREAD) fq29_sub_impl((a), (b), Fq29Consts::SPREAD)
__device__ __forceinline__ Fq29 fq29_sub_impl(const Fq29& a, const Fq29& b, const uint32_t (&sp)[13]) {
    Fq29 r;
#pragma unroll
    for (int i = 0; i < 13; i++) r.l[i] = a.l[i] + sp[i] - b.l[i];
    return r;
}

// Montgomery product a b 2^-406 mod p (result N for operands below 8p).  Columns 0 .. 13 each fix one m_k; the m_i p_j terms
// reach column 25, one past the a_i b_j ones; columns 14 .. 25 leave the result limbs 0 .. 11 and the accumulator the twelfth.
__device__ __forceinline__ Fq29 fq29_mul(const Fq29& a, const Fq29& b) {
    Fq29 r;
    uint32_t m[14];
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 14; k++) {
#pragma unroll
        for (int i = (k > 12 ? k - 12 : 0); i <= (k < 12 ? k : 12); i++) acc += (uint64_t)a.l[i] * b.l[k - i];
#pragma unroll
        for (int i = (k > 12 ? k - 12 : 0); i < k; i++) acc += (uint64_t)m[i] * Fq29Consts::P[k - i];
        // p = 1 mod 2^29: m_k = -acc mod 2^29 and acc + m_k * p_0 clears the low limb
        m[k] = (0u - (uint32_t)acc) & M29Q;
        acc = (acc + m[k]) >> 29;
    }
#pragma unroll
    for (int k = 14; k < 26; k++) {
#pragma unroll
        for (int i = k - 12; i < 13; i++) acc += (uint64_t)a.l[i] * b.l[k - i];
#pragma unroll
        for (int i = k - 12; i < 14; i++) acc += (uint64_t)m[i] * Fq29Consts::P[k - i];
        r.l[k - 14] = (uint32_t)acc & M29Q;
        acc >>= 29;
    }
    r.l[12] = (uint32_t)acc;
    return r;
}
// The same product as one asm statement (text generated by tools/gen_mul28_asm.py fq29; the carry rule and the reasons are
// those of fq28_mul_asm): 337 + 14 x 3 + 12 x 2 + 1 = 404 instructions, the same limbs as fq29_mul bit for bit
// (tools/ubench/te28_bench.hip compares them on the GPU; tools/check_te29.py emulates the carry rule, whose
// acc + 2^29 - 1 is part of every column bound below).
#include "fq29_mul_asm.inc"
__device__ __forceinline__ Fq29 fq29_mul_asm(const Fq29& a, const Fq29& b) {
    Fq29 r;
    uint32_t m0, m1, m2, m3, m4, m5, m6, m7, m8, m9, m10, m11, m12, m13;
    constexpr const uint32_t (&P)[13] = Fq29Consts::P;
    asm(SWM_FQ29_MUL_ASM_TEXT
        : "=&v"(r.l[0]), "=&v"(r.l[1]), "=&v"(r.l[2]), "=&v"(r.l[3]), "=&v"(r.l[4]), "=&v"(r.l[5]), "=&v"(r.l[6]), "=&v"(r.l[7]),
          "=&v"(r.l[8]), "=&v"(r.l[9]), "=&v"(r.l[10]), "=&v"(r.l[11]), "=&v"(r.l[12]),
          "=&v"(m0), "=&v"(m1), "=&v"(m2), "=&v"(m3), "=&v"(m4), "=&v"(m5), "=&v"(m6), "=&v"(m7), "=&v"(m8), "=&v"(m9),
          "=&v"(m10), "=&v"(m11), "=&v"(m12), "=&v"(m13)
        : "v"(a.l[0]), "v"(a.l[1]), "v"(a.l[2]), "v"(a.l[3]), "v"(a.l[4]), "v"(a.l[5]), "v"(a.l[6]), "v"(a.l[7]), "v"(a.l[8]),
          "v"(a.l[9]), "v"(a.l[10]), "v"(a.l[11]), "v"(a.l[12]),
          "v"(b.l[0]), "v"(b.l[1]), "v"(b.l[2]), "v"(b.l[3]), "v"(b.l[4]), "v"(b.l[5]), "v"(b.l[6]), "v"(b.l[7]), "v"(b.l[8]),
          "v"(b.l[9]), "v"(b.l[10]), "v"(b.l[11]), "v"(b.l[12]),
          "s"(P[1]), "s"(P[2]), "s"(P[3]), "s"(P[4]), "s"(P[5]), "s"(P[6]), "s"(P[7]), "s"(P[8]), "s"(P[9]), "s"(P[10]),
          "s"(P[11]), "s"(P[12]), "s"(M29Q), "s"((uint64_t)M29Q)
        : "v0", "v1", "vcc");
    return r;
}
struct Mul29Fenced {  // the C form behind scheduling fences (see MulFenced)
    static __device__ __forceinline__ Fq29 mul(const Fq29& a, const Fq29& b) {
        __builtin_amdgcn_sched_barrier(0);
        Fq29 r = fq29_mul(a, b);
        __builtin_amdgcn_sched_barrier(0);
        return r;
    }
};
struct Mul29Asm {
    static __device__ __forceinline__ Fq29 mul(const Fq29& a, const Fq29& b) { return fq29_mul_asm(a, b); }
};

// ------------------------------------------------------------------------------------------------ twisted Edwards points in the 29-bit domain
// Coordinates are field elements times 2^406.  An accumulator at rest has normalised limbs (below 2^29; the top limb holds what
// the value leaves) and X < 3p, Y < 2p, T and Z: N.  After an addition all four are N; the first point of a segment
// (te29_from_row) has X in (p, 3p), Y below 2p and Z the constant.  That form is what te29_madd_row and te29_to_slot accept
// (a Z1 of 2p with every limb full would take F G to 1.05 x 2^64).
struct T29 {
    Fq29 x, y, t, z;
};
// one coordinate of a table row (G1TE: thirteen limbs in a 64-byte sector): three 16-byte loads and a 4-byte one
__device__ __forceinline__ Fq29 te29_load_coord(const uint32_t* __restrict__ p) {
    const uint4 v0 = *reinterpret_cast<const uint4*>(p), v1 = *reinterpret_cast<const uint4*>(p + 4),
                v2 = *reinterpret_cast<const uint4*>(p + 8);
    Fq29 r;
    r.l[0] = v0.x, r.l[1] = v0.y, r.l[2] = v0.z, r.l[3] = v0.w;
    r.l[4] = v1.x, r.l[5] = v1.y, r.l[6] = v1.z, r.l[7] = v1.w;
    r.l[8] = v2.x, r.l[9] = v2.y, r.l[10] = v2.z, r.l[11] = v2.w;
    r.l[12] = p[12];
    return r;
}
// E, H, F, G of the unified addition from its first-round results (A, B, C: N) and D = 2 Z1 (Z1: N), shared by the one-lane and
// the quad form so that both give the same limbs.  Bounds (limbs below the top one | value):
//   E = B + 2p - A     < 2^29 + SPREAD2_i <= 3 2^29 - 2 | < 3p (1 + 2^-23)     raw
//   H = A + B          normalised                        | < 2p (1 + 2^-23)
//   D - C + 2p         < 2^30 + SPREAD2_i <= 2^31 - 4   | < 4p (1 + 2^-23)     F when the point is added, G when subtracted
//   D + C              < 3 2^29                          | < 3p (1 + 2^-23)     G when added, F when subtracted
//   F                  normalised;   G raw
// Which are normalised, and why these two: the four products of the second round are the edges of the cycle E - F - G - H - E,
// and a product of two raw operands overflows its columns (E F, F G: up to 1.8 - 2.2 x 2^64; G H, E H: 1.1 - 1.3 x 2^64,
// tools/check_te29.py prints them), so every edge needs a normalised end: two of the four, {F, H} or {E, G}.  With F and H
// normalised the worst column of the four products is 0.95 x 2^64 (F G of a subtracted point: D + C normalised against
// D - C + 2p raw, every limb at its maximum); {E, G} costs the same instructions and bounds no better.  One normalisation is 36 plain instructions.
__device__ __forceinline__ void te29_efgh(Fq29& E, Fq29& F, Fq29& G, Fq29& H, const Fq29& A, const Fq29& B, const Fq29& C, const Fq29& Z1,
                                          bool neg) {
    Fq29 f, h;
#pragma unroll
    for (int i = 0; i < 13; i++) {
        const uint32_t sp = Fq29Consts::SPREAD2[i];
        E.l[i] = B.l[i] + sp - A.l[i];
        h.l[i] = A.l[i] + B.l[i];
        const uint32_t D = Z1.l[i] + Z1.l[i];
        const uint32_t dm = D + sp - C.l[i], dp = D + C.l[i];
        f.l[i] = neg ? dp : dm;
        G.l[i] = neg ? dm : dp;
    }
    F = fq29_normalize(f);
    H = fq29_normalize(h);
}
// acc += +-P for the table row (m2, s2, k2) = (y2 - x2, y2 + x2, 2 d x2 y2) of P, as te28_madd_row: seven products, a negative
// digit loads the first two coordinates from each other's address.  First round (rows: C):
//   Y1 - X1 + 4p: limbs < 2^29 + SPREAD4_i, value < 6p   (SPREAD4 and not SPREAD2: X1 may be te29_from_row's, in (p, 3p))
//   Y1 + X1:      limbs < 2^30,             value < 5p
//   T1:           N
// each against a canonical row coordinate: columns at most 0.63 x 2^64.  Second round: te29_efgh.  All operands below 8p -> N.
template <class M = Mul29Asm>
__device__ __forceinline__ void te29_madd_row(T29& a, const G1TE* __restrict__ rp, bool neg) {
    const uint32_t* pa = neg ? rp->ypx : rp->ymx;
    const uint32_t* pb = neg ? rp->ymx : rp->ypx;
    Fq29 d, s;
#pragma unroll
    for (int i = 0; i < 13; i++) {
        d.l[i] = a.y.l[i] + Fq29Consts::SPREAD4[i] - a.x.l[i];
        s.l[i] = a.y.l[i] + a.x.l[i];
    }
    // all three coordinates of the row are requested before the first product (te28_madd_row, SWM_TE_EARLY_LOADS)
    const Fq29 ra = te29_load_coord(pa), rb = te29_load_coord(pb), rk = te29_load_coord(rp->kt);
    __builtin_amdgcn_sched_barrier(0);
    const Fq29 A = M::mul(d, ra);
    const Fq29 B = M::mul(s, rb);
    const Fq29 C = M::mul(a.t, rk);
    Fq29 E, F, G, H;
    te29_efgh(E, F, G, H, A, B, C, a.z, neg);
    a.x = M::mul(E, F);
    a.y = M::mul(G, H);
    a.t = M::mul(E, H);
    a.z = M::mul(F, G);
}
// the point a row stands for, as an accumulator: (X : Y : T : Z) = (2x : 2y : 2xy : 2), one product (by 1/d).
//   X = +-(s2 - m2) + 2p normalised: in (p, 3p);  Y = s2 + m2 normalised: < 2p;  T: N (operand k2 or 2p - k2: limbs < 2^30, < 2p);  Z: C
__device__ __forceinline__ T29 te29_from_row(const Fq29& m2, const Fq29& s2, const Fq29& k2, bool neg) {
    T29 r;
    Fq29 d, ks;
#pragma unroll
    for (int i = 0; i < 13; i++) {
        d.l[i] = Fq29Consts::SPREAD2[i] + (neg ? m2.l[i] - s2.l[i] : s2.l[i] - m2.l[i]);
        ks.l[i] = neg ? Fq29Consts::SPREAD2[i] - k2.l[i] : k2.l[i];
    }
    r.x = fq29_normalize(d);
    r.y = fq29_normalize(fq29_add(s2, m2));
    r.t = fq29_mul(ks, fq29_const(Fq29Consts::INVD));
    r.z = fq29_const(Fq29Consts::TWO);
    return r;
}
// One accumulator coordinate -> the slot the bucket stage reads (fq28_unpack): the product by the constant 2^392 mod p takes
// x 2^406 to x 2^392, the 28-bit domain.  The operand is an accumulator coordinate at rest (normalised limbs, < 3p), the
// constant canonical: column at most 0.33 x 2^64, result N of THIS form: limbs < 2^29, value < p (1 + 2^-23) < 2^377.  As a
// 12-word integer that is an N value of the 28-bit domain: below 2p, and its fourteenth 28-bit limb (bits 364 ..) is below
// 2^13 < 2^15.
template <class M = Mul29Asm>
__device__ __forceinline__ Fq te29_to_slot(const Fq29& c) {
    return fq29_pack(M::mul(c, fq29_const(Fq29Consts::TO392)));
}

// The mixed addition by a quad (te28_quad_madd_row): the accumulator one coordinate per lane (X, Y, T, Z on lanes 0 .. 3), two
// rounds of one product per lane.  Every lane forms E, F, G, H itself (te29_efgh): same formulas and limbs as te29_madd_row.
template <int SRC>
__device__ __forceinline__ Fq29 te29_quad_get(const Fq29& v) {  // every lane of the quad: the value held by its lane SRC
    Fq29 r;
#pragma unroll
    for (int i = 0; i < 13; i++) r.l[i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.l[i], SRC * 0x55, 0xf, 0xf, true);
    return r;
}
template <class M = Mul29Asm>
__device__ __forceinline__ void te29_quad_madd_row(Fq29& own, const G1TE* __restrict__ rp, bool neg, unsigned q) {
    const uint32_t* pr = q == 2 ? rp->kt : ((q == 0) != neg ? rp->ymx : rp->ypx);
    const Fq29 v = te29_load_coord(pr);
    Fq29 u;  // lane 0: Y1 - X1 + 4p, lane 1: Y1 + X1, lane 2: T1, lane 3: Z1 (its product is not used)
#pragma unroll
    for (int i = 0; i < 13; i++) {
        const uint32_t other = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)own.l[i], 0xB1, 0xf, 0xf, true);  // quad_perm [1, 0, 3, 2]
        u.l[i] = q == 0 ? other + Fq29Consts::SPREAD4[i] - own.l[i] : (q == 1 ? own.l[i] + other : own.l[i]);
    }
    Fq29 p1 = M::mul(u, v);
#pragma unroll
    for (int i = 0; i < 13; i++) p1.l[i] = q == 3 ? own.l[i] : p1.l[i];  // lane 3 passes Z1 on
    const Fq29 A = te29_quad_get<0>(p1), B = te29_quad_get<1>(p1), C = te29_quad_get<2>(p1), Z1 = te29_quad_get<3>(p1);
    Fq29 E, F, G, H, l, r;  // lane 0: E F, lane 1: G H, lane 2: E H, lane 3: F G
    te29_efgh(E, F, G, H, A, B, C, Z1, neg);
#pragma unroll
    for (int i = 0; i < 13; i++) {
        l.l[i] = q == 1 ? G.l[i] : (q == 3 ? F.l[i] : E.l[i]);
        r.l[i] = q == 0 ? F.l[i] : (q == 3 ? G.l[i] : H.l[i]);
    }
    own = M::mul(l, r);
}
// the first point of a segment (te29_from_row), one coordinate per lane
template <class M = Mul29Asm>
__device__ __forceinline__ Fq29 te29_quad_from_row(const G1TE* __restrict__ rp, bool neg, unsigned q) {
    const Fq29 a = te29_load_coord(q == 2 ? rp->kt : rp->ymx), s2 = te29_load_coord(rp->ypx);  // a: m2, or k2 on lane 2
    Fq29 d, ks;
#pragma unroll
    for (int i = 0; i < 13; i++) {
        d.l[i] = q == 0 ? Fq29Consts::SPREAD2[i] + (neg ? a.l[i] - s2.l[i] : s2.l[i] - a.l[i]) : s2.l[i] + a.l[i];
        ks.l[i] = neg ? Fq29Consts::SPREAD2[i] - a.l[i] : a.l[i];
    }
    d = fq29_normalize(d);  // lane 0: +-2x in (p, 3p), lane 1: 2y
    const Fq29 t = M::mul(ks, fq29_const(Fq29Consts::INVD));  // lane 2: 2 d x y / d
    Fq29 r;
#pragma unroll
    for (int i = 0; i < 13; i++) r.l[i] = q < 2 ? d.l[i] : (q == 2 ? t.l[i] : Fq29Consts::TWO[i]);
    return r;
}

// ------------------------------------------------------------------------------------------------ the general addition (bucket stage)
// A point at rest in MEMORY (a partial sum in HBM, an LDS slot of the bucket stage): X | Y | T | Z, thirteen limbs each, unpacked —
// 4 x 13 x 4 B = 208 B, thirteen 128-bit words, the stride of the bucket stage's padded 28-bit slot (msm_points.cuh RedSlot), so the
// LDS budget and the bank layout of its 128-bit accesses are those of the 28-bit form; nothing is packed or unpacked on the way.
// A coordinate is 52 bytes and starts on a 16-byte boundary only every fourth time, so the one-lane forms move a point as two
// runs of whole 128-bit words: words 0 .. 27 (X, Y and the first two limbs of T) and words 28 .. 51 (the rest of T, and Z).
// Accepted forms of an operand:  all four coordinates N (what an addition leaves);  X normalised below 3p, Y normalised below 2p,
// T: N, Z: C (what te29_from_row leaves for a one-entry segment);  the identity (0 : 1 : 0 : 1), Y = Z = the constant ONE.
struct alignas(16) TE29Pt {
    uint32_t w[52];
};
static_assert(sizeof(TE29Pt) == 208, "point stride");
__device__ __forceinline__ void te29_pt_load_xy(const TE29Pt* p, Fq29& x, Fq29& y, uint32_t (&t01)[2]) {
    uint32_t w[28];
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const uint4 v = reinterpret_cast<const uint4*>(p->w)[k];
        w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
    }
#pragma unroll
    for (int i = 0; i < 13; i++) x.l[i] = w[i], y.l[i] = w[13 + i];
    t01[0] = w[26], t01[1] = w[27];
}
__device__ __forceinline__ void te29_pt_load_tz(const TE29Pt* p, const uint32_t (&t01)[2], Fq29& t, Fq29& z) {
    uint32_t w[24];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const uint4 v = reinterpret_cast<const uint4*>(p->w)[7 + k];
        w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
    }
    t.l[0] = t01[0], t.l[1] = t01[1];
#pragma unroll
    for (int i = 2; i < 13; i++) t.l[i] = w[i - 2];
#pragma unroll
    for (int i = 0; i < 13; i++) z.l[i] = w[11 + i];
}
__device__ __forceinline__ void te29_pt_store_xy(TE29Pt* p, const Fq29& x, const Fq29& y, uint32_t t0, uint32_t t1) {
    uint32_t w[28];
#pragma unroll
    for (int i = 0; i < 13; i++) w[i] = x.l[i], w[13 + i] = y.l[i];
    w[26] = t0, w[27] = t1;
#pragma unroll
    for (int k = 0; k < 7; k++) reinterpret_cast<uint4*>(p->w)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
__device__ __forceinline__ void te29_pt_store_tz(TE29Pt* p, const Fq29& t, const Fq29& z) {
    uint32_t w[24];
#pragma unroll
    for (int i = 2; i < 13; i++) w[i - 2] = t.l[i];
#pragma unroll
    for (int i = 0; i < 13; i++) w[11 + i] = z.l[i];
#pragma unroll
    for (int k = 0; k < 6; k++) reinterpret_cast<uint4*>(p->w)[7 + k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
// an accumulator at rest (msm_accumulate_te's, after any number of additions) as it is: the limbs are normalised already
__device__ __forceinline__ void te29_pt_store(TE29Pt* p, const T29& a) {
    te29_pt_store_xy(p, a.x, a.y, a.t.l[0], a.t.l[1]);
    te29_pt_store_tz(p, a.t, a.z);
}
__device__ __forceinline__ T29 te29_pt_load(const TE29Pt* p) {
    T29 r;
    uint32_t t01[2];
    te29_pt_load_xy(p, r.x, r.y, t01);
    te29_pt_load_tz(p, t01, r.t, r.z);
    return r;
}
__device__ __forceinline__ void te29_store_identity(TE29Pt* p) {
    T29 r;
#pragma unroll
    for (int i = 0; i < 13; i++) r.x.l[i] = r.t.l[i] = 0, r.y.l[i] = r.z.l[i] = Fq29Consts::ONE[i];
    te29_pt_store(p, r);
}
// one coordinate per lane of a quad: plain 32-bit accesses (a coordinate is not a run of whole 128-bit words)
__device__ __forceinline__ Fq29 te29_pt_load_coord(const TE29Pt* p, unsigned c) {
    Fq29 r;
#pragma unroll
    for (int i = 0; i < 13; i++) r.l[i] = p->w[13 * c + i];
    return r;
}
__device__ __forceinline__ void te29_pt_store_coord(TE29Pt* p, unsigned c, const Fq29& v) {
#pragma unroll
    for (int i = 0; i < 13; i++) p->w[13 * c + i] = v.l[i];
}
__device__ __forceinline__ void te29_quad_store_identity(TE29Pt* p, unsigned q) {
    Fq29 v;
#pragma unroll
    for (int i = 0; i < 13; i++) v.l[i] = (q & 1u) ? Fq29Consts::ONE[i] : 0u;
    te29_pt_store_coord(p, q, v);
}
// First round of the general addition: A = (Y1 - X1)(Y2 - X2), B = (Y1 + X1)(Y2 + X2), C = 2d T1 T2 and Z1 Z2 (te29_efgh doubles it).
// Bounds (limbs below the top one | value; tools/check_te29.py `tail` prints the columns):
//   Y - X + 4p   raw: < 2^29 + SPREAD4_i <= 3 2^29 - 2 | < 6p      (SPREAD4: X may be te29_from_row's, below 3p)
//   Y + X        raw: < 2^30                           | < 5p
// Two raw differences multiply to 1.45 x 2^64 in the worst column and two raw sums to 1.05 x 2^64, so the FIRST operand's difference and
// sum are carry-normalised (top limb then <= that of 6p resp. 5p): A at most 0.76 x 2^64, B 0.64 x 2^64.  T and Z are N: T1 T2,
// Z1 Z2 and (T1 T2) 2d (the constant: C) at most 0.30 x 2^64.  All operands below 8p -> A, B, C and Z1 Z2: N, what te29_efgh takes with
// D = 2 Z1 Z2 in the place of 2 Z1: its second-round products are bounded where it stands (a point that is ADDED: F G at most 0.85 x 2^64).
// The same evaluation at build time (check_te29.py's column_bound: every a_i, b_i and m_i at its maximum, the carry rule's 2^29 - 1
// included).
constexpr bool te29_columns_fit(const uint32_t (&amax)[13], const uint32_t (&bmax)[13]) {
    unsigned __int128 carry = 0;
    for (int k = 0; k < 26; k++) {
        unsigned __int128 acc = carry;
        for (int i = (k > 12 ? k - 12 : 0); i <= (k < 12 ? k : 12); i++) acc += (uint64_t)amax[i] * bmax[k - i];
        for (int i = (k > 12 ? k - 12 : 0); i < (k < 14 ? k : 14); i++) acc += (uint64_t)M29Q * Fq29Consts::P[k - i];
        if (k < 14) acc += M29Q;
        if (acc >= ((unsigned __int128)1 << 64) - (1u << 29)) return false;
        carry = acc >> 29;
    }
    return true;
}
// The operand maxima are the tool's own: te29_bounds_gen.inc is written by `python tools/check_te29.py header` from its
// tail_operands() and held to it by tests/test_te29_tail_bounds.py, so the build asserts what the tool prints.
struct Te29Bound {
    const char* name;
    uint32_t a[13], b[13];
};
#include "te29_bounds_gen.inc"
constexpr Te29Bound TE29_TAIL_BOUNDS[] = {SWM_TE29_TAIL_BOUNDS};
constexpr bool te29_slot_add_bounds_ok() {
    for (const Te29Bound& r : TE29_TAIL_BOUNDS)
        if (!te29_columns_fit(r.a, r.b)) return false;
    return sizeof(TE29_TAIL_BOUNDS) / sizeof(TE29_TAIL_BOUNDS[0]) == 10;  // nine products and the store's
}
static_assert(te29_slot_add_bounds_ok(), "te29_slot_add: a column of one of its nine products can reach 2^64 - 2^29");
template <class M>
__device__ __forceinline__ void te29_add_ab(Fq29& A, Fq29& B, const Fq29& ax, const Fq29& ay, const Fq29& qx, const Fq29& qy) {
    A = M::mul(fq29_normalize(FQ29_SUB(ay, ax, SPREAD4)), FQ29_SUB(qy, qx, SPREAD4));
    B = M::mul(fq29_normalize(fq29_add(ay, ax)), fq29_add(qy, qx));
}
// *dst = *pa + *pq: the unified 9-product law of te28_slot_add on points at rest, streamed as that one is — every load precedes the
// first store, so dst may be pa or pq, and pa == pq is doubling.  The result has all four coordinates N.  Against the 28-bit step:
// nine products of 404 instead of 447 instructions, no unpacking of eight coordinates or packing of four, four carry
// normalisations (two here, two in te29_efgh) of 36 instructions each.
template <class M = Mul29Asm>
__device__ __forceinline__ void te29_slot_add(TE29Pt* dst, const TE29Pt* pa, const TE29Pt* pq) {
    Fq29 A, B, C, ZZ;
    {
        uint32_t at01[2], qt01[2];
        {
            Fq29 ax, ay, qx, qy;
            te29_pt_load_xy(pa, ax, ay, at01);
            te29_pt_load_xy(pq, qx, qy, qt01);
            te29_add_ab<M>(A, B, ax, ay, qx, qy);
        }
        Fq29 at, az, qt, qz;
        te29_pt_load_tz(pa, at01, at, az);
        te29_pt_load_tz(pq, qt01, qt, qz);
        C = M::mul(M::mul(at, qt), fq29_const(Fq29Consts::K2D));
        ZZ = M::mul(az, qz);
    }
    Fq29 E, F, G, H;
    te29_efgh(E, F, G, H, A, B, C, ZZ, false);
    const Fq29 T3 = M::mul(E, H);
    te29_pt_store_xy(dst, M::mul(E, F), M::mul(G, H), T3.l[0], T3.l[1]);
    te29_pt_store_tz(dst, T3, M::mul(F, G));
}
// te29_slot_add for steps in which a lane reads ANOTHER lane's slot that the same step rewrites (te28_slot_add_sync: the in-place
// suffix scan of msm_bucket_reduce_low): every load of the workgroup precedes the barrier, every store follows it.  Same limbs.
template <class M = Mul29Asm>
__device__ __forceinline__ void te29_slot_add_sync(TE29Pt* dst, const TE29Pt* pa, const TE29Pt* pq, bool act, bool barrier = true) {
    Fq29 E, F, G, H;
#pragma unroll
    for (int i = 0; i < 13; i++) E.l[i] = F.l[i] = G.l[i] = H.l[i] = 0;
    if (act) {
        Fq29 A, B, C, ZZ;
        uint32_t at01[2], qt01[2];
        {
            Fq29 ax, ay, qx, qy;
            te29_pt_load_xy(pa, ax, ay, at01);
            te29_pt_load_xy(pq, qx, qy, qt01);
            te29_add_ab<M>(A, B, ax, ay, qx, qy);
        }
        Fq29 at, az, qt, qz;
        te29_pt_load_tz(pa, at01, at, az);
        te29_pt_load_tz(pq, qt01, qt, qz);
        C = M::mul(M::mul(at, qt), fq29_const(Fq29Consts::K2D));
        ZZ = M::mul(az, qz);
        te29_efgh(E, F, G, H, A, B, C, ZZ, false);
    }
    if (barrier) __syncthreads();  // (uniform over the workgroup; false for steps in which every lane works on slots of its own)
    if (act) {
        const Fq29 T3 = M::mul(E, H);
        te29_pt_store_xy(dst, M::mul(E, F), M::mul(G, H), T3.l[0], T3.l[1]);
        te29_pt_store_tz(dst, T3, M::mul(F, G));
    }
}
// The same addition by a quad of lanes (te28_quad_add): three rounds of one product per lane — (A, B, T1 T2, Z1 Z2), then 2d (T1 T2)
// on lane 2, then (X3, Y3, T3, Z3) — every lane storing one coordinate.  Every lane normalises its first operand: on lanes 2 and 3
// that is a coordinate with normalised limbs already, which the carry chain leaves as it is.  Same formulas, same limbs as
// te29_slot_add.  All lanes of the quad are handed the same pointers; one wave, lock step: the loads precede the stores.
template <class M = Mul29Asm>
__device__ __forceinline__ void te29_quad_add(TE29Pt* dst, const TE29Pt* pa, const TE29Pt* pq, unsigned q) {
    const unsigned ia = q < 2 ? 1u : q;  // lanes 0, 1: Y and X; lane 2: T; lane 3: Z
    const Fq29 a1 = te29_pt_load_coord(pa, ia), b1 = te29_pt_load_coord(pa, 0), a2 = te29_pt_load_coord(pq, ia), b2 = te29_pt_load_coord(pq, 0);
    Fq29 u, v;
#pragma unroll
    for (int i = 0; i < 13; i++) {
        const uint32_t sp = Fq29Consts::SPREAD4[i];
        const uint32_t t1 = q == 0 ? sp - b1.l[i] : (q == 1 ? b1.l[i] : 0u), t2 = q == 0 ? sp - b2.l[i] : (q == 1 ? b2.l[i] : 0u);
        u.l[i] = a1.l[i] + t1;
        v.l[i] = a2.l[i] + t2;
    }
    Fq29 p1 = M::mul(fq29_normalize(u), v);
    const Fq29 p2 = M::mul(p1, fq29_const(Fq29Consts::K2D));  // only lane 2 keeps it: C = 2d T1 T2
#pragma unroll
    for (int i = 0; i < 13; i++) p1.l[i] = q == 2 ? p2.l[i] : p1.l[i];
    const Fq29 A = te29_quad_get<0>(p1), B = te29_quad_get<1>(p1), C = te29_quad_get<2>(p1), ZZ = te29_quad_get<3>(p1);
    Fq29 E, F, G, H, l, r;  // lane 0: E F, lane 1: G H, lane 2: E H, lane 3: F G
    te29_efgh(E, F, G, H, A, B, C, ZZ, false);
#pragma unroll
    for (int i = 0; i < 13; i++) {
        l.l[i] = q == 1 ? G.l[i] : (q == 3 ? F.l[i] : E.l[i]);
        r.l[i] = q == 0 ? F.l[i] : (q == 3 ? G.l[i] : H.l[i]);
    }
    te29_pt_store_coord(dst, q, M::mul(l, r));  // X3, Y3, T3, Z3
}
// value below p (1 + 2^-23) with normalised limbs -> below p
__device__ __forceinline__ Fq29 fq29_canonical(const Fq29& a) {
    Fq29 d;
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 13; i++) {
        const uint32_t t = a.l[i] - Fq29Consts::P[i] - borrow;  // |a_i - p_i - borrow| < 2^30: bit 31 is the sign
        d.l[i] = t & M29Q;
        borrow = t >> 31;
    }
    Fq29 r;
#pragma unroll
    for (int i = 0; i < 13; i++) r.l[i] = borrow ? a.l[i] : d.l[i];
    return r;
}
// 29-bit domain (x 2^406) -> radix 2^384, canonical, packed: what te28_store_384 gives for the same point (the host folds in that
// form).  One product per coordinate by 2^384 mod p; operand: a coordinate at rest (below 3p, normalised limbs), column at most
// 0.33 x 2^64, result N.
__device__ __forceinline__ void te29_store_384(G1XYZZ& m, const TE29Pt& slot) {
    const T29 p = te29_pt_load(&slot);
    const Fq29 k = fq29_const(Fq29Consts::TO384);
    m.x = fq29_pack(fq29_canonical(fq29_mul(p.x, k)));
    m.y = fq29_pack(fq29_canonical(fq29_mul(p.y, k)));
    m.zz = fq29_pack(fq29_canonical(fq29_mul(p.t, k)));
    m.zzz = fq29_pack(fq29_canonical(fq29_mul(p.z, k)));
}

}  // namespace swm

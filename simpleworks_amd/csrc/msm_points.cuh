// msm_points.cuh — the device routines and slot types of the MSM's point stages that more than one unit needs: the mixed addition
// of msm_accumulate (Acc28, madd28), the streamed forms of the 28-bit general addition, and the slots and point forms of the bucket
// stage.  Included by msm_stages.hip (the kernels) and msm_selftest.hip (the same routines, one call per element), by nothing else.
#pragma once
#include "fq28.cuh"
#include "fq29.cuh"
#include "g1.cuh"

namespace swm {

// ---------------------------------------------------------------------------------------------- accumulation
// The inner loop of msm_accumulate (msm_stages.hip) runs in the 28-bit lazy-carry representation of fq28.cuh (bases28 = the same points with both
// coordinates pre-multiplied by 2^8, i.e. in Montgomery radix 2^392).  Bounds, per EFD madd-2008-s step
// (N: normalised limbs, value < 2p;  X1: normalised, < 18p;  Y1: normalised, < 6p;  ZZ1, ZZZ1: N):
//   U2 = x2 ZZ1, S2 = y2 ZZZ1                              N          (y2 may be 4p - y2: limbs < 2^30, value < 4p)
//   P  = U2 + 32p - X1                                     limbs < 2^30, value in (14p, 34p)
//   R  = S2 +  8p - Y1                                     limbs < 2^30, value in ( 2p, 10p)
//   PP = P^2, PPP = P PP, Q = X1 PP, RR = R^2              N          (products of two lazy values: 14 * 2^60 < 2^64)
//   X3 = normalise(RR + 16p - PPP - 2Q)                    normalised, value in (10p, 18p)
//   V  = Q + 32p - X3                                      limbs < 2^30, value in (14p, 24p)
//   Y3 = (R V + (8p - Y1) PPP) 2^-392, ONE reduction        N          (fq28_mul2: limbs 1.5 2^29 x 1.5 2^29 + 2^29 x 2^28)
//   ZZ3 = ZZ1 PP, ZZZ3 = ZZZ1 PPP                          N
// P = 0 mod p (doubling or cancellation: the point equals +-accumulator) is detected on PP, which is an N value; the
// segment is then recomputed with the fully reducing 32-bit-limb adder (cold path).
struct Acc28 {
    Fq28 x, y, zz, zzz;
};
__device__ __forceinline__ bool madd28(Acc28& a, const Fq28& x2, const Fq28& y2) {
    Fq28 u2 = fq28_mul(x2, a.zz);
    Fq28 s2 = fq28_mul(y2, a.zzz);
    Fq28 p = FQ28_SUB(u2, a.x, SPREAD32);
    Fq28 r = FQ28_SUB(s2, a.y, SPREAD8);
    Fq28 pp = fq28_mul(p, p);
    if (fq28_is_zero_mod_p(pp)) return false;
    Fq28 ppp = fq28_mul(p, pp);
    Fq28 q = fq28_mul(a.x, pp);
    Fq28 rr = fq28_mul(r, r);
    Fq28 x3;
#pragma unroll
    for (int i = 0; i < 14; i++) x3.l[i] = rr.l[i] + Fq28Consts::SPREAD16_3[i] - ppp.l[i] - q.l[i] - q.l[i];
    x3 = fq28_normalize(x3);
    Fq28 v = FQ28_SUB(q, x3, SPREAD32);
    Fq28 ny;  // 8p - Y1 > 0, limbs < 2^29
#pragma unroll
    for (int i = 0; i < 14; i++) ny.l[i] = Fq28Consts::SPREAD8[i] - a.y.l[i];
    a.y = fq28_mul2(r, v, ny, ppp);  // R V - Y1 PPP with one reduction
    a.x = x3;
    a.zz = fq28_mul(a.zz, pp);
    a.zzz = fq28_mul(a.zzz, ppp);
    return true;
}

// ---------------------------------------------------------------------------------------------- bucket stage
// Register budget of the bucket stage: a general addition keeps two points (2 x 56 VGPRs) plus ~8 temporaries
// (112 VGPRs) live; a third live point spills to scratch, i.e. to HBM-backed private memory with nothing to hide the
// latency at one wave per SIMD (measured: 5x slower).  So each lane parks the point it is not currently adding in LDS
// (packed 192-B slots) and at most two points are ever in registers.
// (the unfenced multiplier with a 512-register budget — amdgpu_waves_per_eu(1, 1) — was measured in r02: the bucket stage
// takes the same 0.85 ms either way)
__device__ __forceinline__ void p28_add_ool(P28& a, const P28& q) { p28_add<MulFenced>(a, q); }

// Streamed form of the general addition for the bucket stage:  *dst = *pa + *pq  (dst may be pa), operands in memory
// (LDS slots or HBM, packed 192-B points of the 28-bit domain).  Coordinates are loaded when they are needed and results
// stored as soon as they exist, so that about eight field elements are live at the peak instead of two whole points plus
// temporaries: the kernel then fits the 168-VGPR footprint of an msm_accumulate wave.  That matters more than the
// instruction count: with 248 VGPRs a bucket-stage wave could only be placed on a SIMD that holds at most ONE
// accumulation wave, i.e. never while an accumulation grid was in flight — the r02 timeline showed all 12.6 ms of
// bucket stage per 2^20 proof running with no accumulation beside it.  Same formulas and bounds as p28_add_fast.
// *dst = 2 * *pa, streamed (EFD dbl-2008-s-1, a = 0; the identity stays the identity: zz, zzz are only multiplied)
__device__ __forceinline__ void p28_slot_dbl(G1XYZZ* dst, const G1XYZZ* pa) {
    typedef MulFenced M;
    Fq28 y = fq28_unpack(pa->y);
    Fq28 u = fq28_add(y, y);                    // limbs < 2^29, value < 12p
    Fq28 v = M::sqr(u);
    if (fq28_is_zero_mod_p(v)) {                // y = 0 mod p, a point of order two: its double is the identity, zz EXACTLY 0 (p28_dbl)
        p28_store(*dst, p28_identity());
        return;
    }
    Fq28 w = M::mul(u, v);
    Fq28 ny;                                    // 8p - Y1 > 0 (Y1 < 6p), limbs < 2^29
#pragma unroll
    for (int i = 0; i < 14; i++) ny.l[i] = Fq28Consts::SPREAD8[i] - y.l[i];
    Fq28 zz3 = M::mul(v, fq28_unpack(pa->zz));
    Fq28 zzz3 = M::mul(w, fq28_unpack(pa->zzz));
    Fq28 x = fq28_unpack(pa->x);
    Fq28 sv = M::mul(x, v);
    Fq28 xx = M::sqr(x);
    dst->zz = fq28_pack(zz3);
    dst->zzz = fq28_pack(zzz3);
    Fq28 m = fq28_add(fq28_add(xx, xx), xx);   // limbs < 3 * 2^28, value < 6p
    Fq28 mm = M::sqr(m);
    Fq28 x3;
#pragma unroll
    for (int i = 0; i < 14; i++) x3.l[i] = mm.l[i] + Fq28Consts::SPREAD16_3[i] - sv.l[i] - sv.l[i];
    x3 = fq28_normalize(x3);                   // (12p, 18p)
    dst->x = fq28_pack(x3);
    dst->y = fq28_pack(M::mul2(m, FQ28_SUB(sv, x3, SPREAD32), ny, w));  // M (S - X3) - W Y1, one reduction
}
__device__ __forceinline__ bool fq28_all_zero(const Fq28& a) {
    uint32_t z = 0;
#pragma unroll
    for (int i = 0; i < 14; i++) z |= a.l[i];
    return z == 0;
}
__device__ __forceinline__ void p28_slot_add(G1XYZZ* dst, const G1XYZZ* pa, const G1XYZZ* pq) {
    typedef MulFenced M;
    Fq28 azz = fq28_unpack(pa->zz), qzz = fq28_unpack(pq->zz);
    if (fq28_all_zero(qzz)) {  // q is the identity
        if (dst != pa) *dst = *pa;
        return;
    }
    if (fq28_all_zero(azz)) {  // a is the identity
        *dst = *pq;
        return;
    }
    Fq28 u1 = M::mul(fq28_unpack(pa->x), qzz);
    Fq28 p = M::mul(fq28_unpack(pq->x), azz);  // U2
    p = FQ28_SUB(p, u1, SPREAD4);               // P = U2 - U1, limbs < 2^30, value in (2p, 6p)
    Fq28 t = M::mul(azz, qzz);
    Fq28 pp = M::sqr(p);
    if (fq28_is_zero_mod_p(pp)) {  // q = +-a: doubling or cancellation, decided on (S2 - S1)^2 (cold)
        Fq28 c1 = M::mul(fq28_unpack(pa->y), fq28_unpack(pq->zzz)), c2 = M::mul(fq28_unpack(pq->y), fq28_unpack(pa->zzz));
        if (fq28_is_zero_mod_p(M::sqr(FQ28_SUB(c2, c1, SPREAD4)))) p28_slot_dbl(dst, pa);
        else p28_store(*dst, p28_identity());
        return;
    }
    // the x / zz side is finished first (its inputs die early): of a only y and zzz are still to be read, and those slots
    // are written last
    dst->zz = fq28_pack(M::mul(t, pp));
    Fq28 ppp = M::mul(p, pp);
    Fq28 qq = M::mul(u1, pp);
    Fq28 azzz = fq28_unpack(pa->zzz), qzzz = fq28_unpack(pq->zzz);
    Fq28 s1 = M::mul(fq28_unpack(pa->y), qzzz);
    Fq28 r = M::mul(fq28_unpack(pq->y), azzz);  // S2
    r = FQ28_SUB(r, s1, SPREAD4);                // R = S2 - S1
    Fq28 t2 = M::mul(azzz, qzzz);
    dst->zzz = fq28_pack(M::mul(t2, ppp));
    Fq28 rr = M::sqr(r);
    Fq28 x3;
#pragma unroll
    for (int i = 0; i < 14; i++) x3.l[i] = rr.l[i] + Fq28Consts::SPREAD16_3[i] - ppp.l[i] - qq.l[i] - qq.l[i];
    x3 = fq28_normalize(x3);  // (10p, 18p)
    dst->x = fq28_pack(x3);
    Fq28 ns1;  // 4p - S1 > 0 (S1 < 2p), limbs < 2^29
#pragma unroll
    for (int i = 0; i < 14; i++) ns1.l[i] = Fq28Consts::SPREAD4[i] - s1.l[i];
    dst->y = fq28_pack(M::mul2(r, FQ28_SUB(qq, x3, SPREAD32), ns1, ppp));  // R (Q - X3) - S1 PPP, one reduction
}

// The two point forms of the bucket stage: XYZZ on the Weierstrass curve (per-window schedule, XYZZ tables) and extended
// twisted Edwards (TE tables).  Each kernel of msm_stages.hip is instantiated once per form; a launch handles jobs of one form.
// LANES: hardware lanes that share one chain of the bucket stage (msm_bucket_reduce); `q` = the lane's index among them.
// One LDS slot of the bucket stage: a packed point PLUS 16 bytes (r06).  At 192 bytes the slots of consecutive lanes lie 48 dwords
// = 16 banks apart, so the 128-bit reads and writes of a wave fall on 8 of the 32 banks: 87 % of the kernel's LDS cycles were bank
// conflicts (SQ_LDS_BANK_CONFLICT 51.1 M of SQ_LDS_IDX_ACTIVE 58.7 M per launch) and the four lone waves of a workgroup queued up
// behind one another's operand loads — the "26 % of wave-cycles parked" of profiles/r05_pmc_sq_msm_bucket_reduce_and_sort.json.
// At 208 bytes (52 dwords: 20 banks) the 128-bit accesses of 8 consecutive lanes cover all 32 banks.  (3 x 256 + 1) x 208 B =
// 159 952 B: just inside the 160 KB of a CU.
struct alignas(16) RedSlot {
    G1XYZZ p;
    uint32_t pad[4];
};
static_assert(sizeof(RedSlot) == 208, "slot stride");
// ... and the slot of the QUAD forms, where a lane reads ONE coordinate (48 bytes) of its chain's slot: there the plain 192 bytes
// are the conflict-free stride (the sixteen 128-bit accesses of four chains fall on every 4-bank group exactly twice; 208 bytes
// puts four of them on one group)
struct alignas(16) PlainSlot {
    G1XYZZ p;
};
// ... and of the 29-bit twisted Edwards form: the unpacked point IS 208 bytes (fq29.cuh TE29Pt), same stride, same banks.
struct alignas(16) Red29Slot {
    TE29Pt p;
};
static_assert(sizeof(Red29Slot) == sizeof(RedSlot), "slot stride");
// Pt: a point at rest (partial sum, LDS slot); quad_add: the four-lane step of a QUAD_TREE form; slot_add_sync: msm_bucket_reduce_low's.
// A job's partial sums are G1XYZZ slots of the 28-bit domain for the XYZZ and the quad forms, raw TE29Pt for FormTE29 (MsmShape::raw).
struct FormXYZZ {
    using Slot = RedSlot;
    using Pt = G1XYZZ;
    static constexpr int LANES = 1;
    static constexpr bool QUAD_TREE = false;
    static __device__ __forceinline__ void slot_add(G1XYZZ* dst, const G1XYZZ* pa, const G1XYZZ* pq, unsigned = 0) { p28_slot_add(dst, pa, pq); }
    static __device__ __forceinline__ void slot_dbl(G1XYZZ* dst, const G1XYZZ* pa, unsigned = 0) { p28_slot_dbl(dst, pa); }
    static __device__ __forceinline__ void copy(G1XYZZ* dst, const G1XYZZ* src, unsigned = 0) { *dst = *src; }
    static __device__ __forceinline__ void store_identity(G1XYZZ& m, unsigned = 0) { p28_store(m, p28_identity()); }
    static __device__ __forceinline__ void store_384(G1XYZZ& m, const G1XYZZ& slot) { p28_store_384(m, p28_load(slot)); }
};
// The one-lane twisted Edwards stage: thirteen 29-bit limbs, slots and partial sums unpacked (fq29.cuh, "the general addition").
struct FormTE29 {
    using Slot = Red29Slot;
    using Pt = TE29Pt;
    static constexpr int LANES = 1;
    static constexpr bool QUAD_TREE = true;
    static __device__ __forceinline__ void slot_add(TE29Pt* dst, const TE29Pt* pa, const TE29Pt* pq, unsigned = 0) { te29_slot_add(dst, pa, pq); }
    static __device__ __forceinline__ void slot_add_sync(TE29Pt* dst, const TE29Pt* pa, const TE29Pt* pq, bool act, bool barrier) {
        te29_slot_add_sync(dst, pa, pq, act, barrier);
    }
    static __device__ __forceinline__ void quad_add(TE29Pt* dst, const TE29Pt* pa, const TE29Pt* pq, unsigned q) { te29_quad_add(dst, pa, pq, q); }
    static __device__ __forceinline__ void slot_dbl(TE29Pt* dst, const TE29Pt* pa, unsigned = 0) { te29_slot_add(dst, pa, pa); }
    static __device__ __forceinline__ void copy(TE29Pt* dst, const TE29Pt* src, unsigned = 0) { *dst = *src; }
    static __device__ __forceinline__ void store_identity(TE29Pt& m, unsigned = 0) { te29_store_identity(&m); }
    static __device__ __forceinline__ void store_384(G1XYZZ& m, const TE29Pt& slot) { te29_store_384(m, slot); }
};
// Twisted Edwards with every chain worked by a quad of lanes (te28_quad_add: three products per lane and step instead of
// nine): the bucket stage of SMALL MSMs, where the chain's latency is all there is.
struct FormTEQuad {
    using Slot = PlainSlot;
    using Pt = G1XYZZ;
    static constexpr int LANES = 4;
    static constexpr bool QUAD_TREE = false;
    static __device__ __forceinline__ void slot_add(G1XYZZ* dst, const G1XYZZ* pa, const G1XYZZ* pq, unsigned q) { te28_quad_add(dst, pa, pq, q); }
    static __device__ __forceinline__ void slot_dbl(G1XYZZ* dst, const G1XYZZ* pa, unsigned q) { te28_quad_add(dst, pa, pa, q); }
    static __device__ __forceinline__ void copy(G1XYZZ* dst, const G1XYZZ* src, unsigned q) { te28_quad_copy(dst, src, q); }
    static __device__ __forceinline__ void store_identity(G1XYZZ& m, unsigned q) { te28_quad_store_identity(&m, q); }
    static __device__ __forceinline__ void store_384(G1XYZZ& m, const G1XYZZ& slot) { te28_store_384(m, slot); }
};

// What msm_big_bucket_sum runs ahead of a QUAD stage: that job's partial sums are 28-bit slots, folded one lane per sum.
struct FormTEFold28 {
    using Pt = G1XYZZ;
    static __device__ __forceinline__ void slot_add(G1XYZZ* dst, const G1XYZZ* pa, const G1XYZZ* pq) { te28_slot_add(dst, pa, pq); }
    static __device__ __forceinline__ void store_identity(G1XYZZ& m) { te28_store_identity(m); }
};

}  // namespace swm

// Micro-benchmark + bit-exactness check of the twisted Edwards mixed addition of msm_accumulate_te (fq28.cuh):
//   r03  packed 144-byte rows, compiler-scheduled multiplier (fq28_mul behind scheduling fences), sign on the accumulator
//   r04  192-byte limb rows, the one-statement asm multiplier (fq28_mul_asm), sign by load address
//   te29 the same rows and law on thirteen 29-bit limbs (fq29.cuh): 337 multiply-adds per product instead of 378, two
//        normalisations per addition; its rows are the r04 rows times 2^14 (radix 2^406), its accumulators leave through
//        te29_to_slot, so that they must equal r04's mod p (compared on the host after reduction below p)
// Every lane runs a chain of CHAIN additions against rows gathered from a small (L2-resident) table, i.e. the loop of the
// accumulation kernel without its HBM gathers: what is measured is instruction issue.  The final accumulators of both
// variants must be identical limb for limb (same products, same limbs) — printed as "identical: yes".
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I simpleworks_amd/csrc -I include tools/ubench/te28_bench.hip -o tools/ubench/te28_bench
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "fq28.cuh"
#include "fq29.cuh"
using namespace swm;
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

struct alignas(16) RowPacked {  // the r03 row
    Fq ymx, ypx, kt;
};
// r03's addition, verbatim in structure: sign taken on the accumulator side, rows unpacked before each product
template <class M>
__device__ __forceinline__ void madd_r03(T28& a, const RowPacked* __restrict__ rp, bool neg) {
    Fq28 a1, b1;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        const uint32_t d = a.y.l[i] + Fq28Consts::SPREAD4[i] - a.x.l[i], s = a.y.l[i] + a.x.l[i];
        a1.l[i] = neg ? s : d;
        b1.l[i] = neg ? d : s;
    }
    Fq28 A = M::mul(a1, fq28_unpack(rp->ymx));
    Fq28 B = M::mul(b1, fq28_unpack(rp->ypx));
    Fq28 C = M::mul(a.t, fq28_unpack(rp->kt));
    Fq28 E, H, F, G;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        const uint32_t sp = Fq28Consts::SPREAD4[i];
        E.l[i] = neg ? A.l[i] + sp - B.l[i] : B.l[i] + sp - A.l[i];
        H.l[i] = A.l[i] + B.l[i];
        const uint32_t D = a.z.l[i] + a.z.l[i];
        const uint32_t dm = D + sp - C.l[i], dp = D + C.l[i];
        F.l[i] = neg ? dp : dm;
        G.l[i] = neg ? dm : dp;
    }
    a.x = M::mul(E, F);
    a.y = M::mul(G, H);
    a.t = M::mul(E, H);
    a.z = M::mul(F, G);
#pragma unroll
    for (int i = 0; i < 14; i++) {
        asm volatile("" : "+v"(a.x.l[i]));
        asm volatile("" : "+v"(a.y.l[i]));
        asm volatile("" : "+v"(a.t.l[i]));
        asm volatile("" : "+v"(a.z.l[i]));
    }
}

__device__ __forceinline__ void store_acc(G1XYZZ& o, const T28& acc) {
    o.x = fq28_pack(acc.x);
    o.y = fq28_pack(acc.y);
    o.zz = fq28_pack(acc.t);
    o.zzz = fq28_pack(acc.z);
}
template <int WAVES>
__global__ void __launch_bounds__(256, WAVES) k_r03(const RowPacked* __restrict__ rows, const uint32_t* __restrict__ idx, uint32_t chain,
                                                    G1XYZZ* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t* my = idx + (size_t)t * chain;
    const RowPacked r0 = rows[my[0] & 0x7fffffffu];
    T28 acc = te28_from_row(fq28_unpack(r0.ymx), fq28_unpack(r0.ypx), fq28_unpack(r0.kt), (my[0] >> 31) != 0);
    for (uint32_t k = 1; k < chain; k++) madd_r03<MulFenced>(acc, rows + (my[k] & 0x7fffffffu), (my[k] >> 31) != 0);
    store_acc(out[t], acc);
}
template <int WAVES, class M>
__global__ void __launch_bounds__(256, WAVES) k_r04(const G1TE* __restrict__ rows, const uint32_t* __restrict__ idx, uint32_t chain,
                                                    G1XYZZ* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t* my = idx + (size_t)t * chain;
    const G1TE* r0 = rows + (my[0] & 0x7fffffffu);
    T28 acc = te28_from_row(te28_load_coord(r0->ymx), te28_load_coord(r0->ypx), te28_load_coord(r0->kt), (my[0] >> 31) != 0);
    for (uint32_t k = 1; k < chain; k++) te28_madd_row<M>(acc, rows + (my[k] & 0x7fffffffu), (my[k] >> 31) != 0);
    store_acc(out[t], acc);
}
template <int WAVES, class M>
__global__ void __launch_bounds__(256, WAVES) k_te29(const G1TE* __restrict__ rows, const uint32_t* __restrict__ idx, uint32_t chain,
                                                     G1XYZZ* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t* my = idx + (size_t)t * chain;
    const G1TE* r0 = rows + (my[0] & 0x7fffffffu);
    T29 acc = te29_from_row(te29_load_coord(r0->ymx), te29_load_coord(r0->ypx), te29_load_coord(r0->kt), (my[0] >> 31) != 0);
    for (uint32_t k = 1; k < chain; k++) te29_madd_row<M>(acc, rows + (my[k] & 0x7fffffffu), (my[k] >> 31) != 0);
    out[t].x = te29_to_slot<M>(acc.x);
    out[t].y = te29_to_slot<M>(acc.y);
    out[t].zz = te29_to_slot<M>(acc.t);
    out[t].zzz = te29_to_slot<M>(acc.z);
}
// one product, both 29-bit multipliers: a as wide as a spread subtraction leaves it (limbs < 3 2^29), b normalised
__global__ void k_mul29_check(const uint32_t* __restrict__ in, uint32_t* __restrict__ bad) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    Fq29 a, b;
#pragma unroll
    for (int i = 0; i < 13; i++) {
        a.l[i] = in[(size_t)t * 26 + i];
        b.l[i] = in[(size_t)t * 26 + 13 + i];
    }
    const Fq29 r0 = fq29_mul(a, b), r1 = fq29_mul_asm(a, b), s0 = fq29_mul(b, b), s1 = fq29_mul_asm(b, b);
    uint32_t x = 0;
#pragma unroll
    for (int i = 0; i < 13; i++) x |= (r0.l[i] ^ r1.l[i]) | (s0.l[i] ^ s1.l[i]);
    if (x) atomicAdd(bad, 1u);
}
// one product, both multipliers, on random lazy operands (limbs < 2^30): the limbs must agree
__global__ void k_mul_check(const uint32_t* __restrict__ in, uint32_t* __restrict__ bad) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    Fq28 a, b;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        a.l[i] = in[(size_t)t * 28 + i];
        b.l[i] = in[(size_t)t * 28 + 14 + i];
    }
    const Fq28 r0 = fq28_mul(a, b), r1 = fq28_mul_asm(a, b), s0 = fq28_mul(a, a), s1 = fq28_mul_asm(a, a);
    uint32_t x = 0;
#pragma unroll
    for (int i = 0; i < 14; i++) x |= (r0.l[i] ^ r1.l[i]) | (s0.l[i] ^ s1.l[i]);
    if (x) atomicAdd(bad, 1u);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
// a random value below p as 14 limbs (top limb below p's: 0x1ae3) and packed into twelve words
static void rand_coord(uint32_t limbs[14], uint32_t words[12]) {
    for (int i = 0; i < 13; i++) limbs[i] = rnd() & 0xfffffffu;
    limbs[13] = rnd() % 0x1ae3u;
    memset(words, 0, 48);
    for (int i = 0; i < 14; i++) {
        const int bit = 28 * i, w = bit >> 5, off = bit & 31;
        words[w] |= limbs[i] << off;
        if (off > 4 && w + 1 < 12) words[w + 1] |= limbs[i] >> (32 - off);
    }
}

// host arithmetic on 12-word integers below 2p, for the 29-bit rows and the comparison of the two domains
static void p_words(uint32_t w[12]) {
    memset(w, 0, 48);
    for (int i = 0; i < 14; i++) {
        const int bit = 28 * i, k = bit >> 5, off = bit & 31;
        w[k] |= Fq28Consts::P[i] << off;
        if (off > 4 && k + 1 < 12) w[k + 1] |= Fq28Consts::P[i] >> (32 - off);
    }
}
static void reduce_once(uint32_t v[12]) {  // v < 2p -> v mod p
    uint32_t p[12], d[12];
    p_words(p);
    uint64_t borrow = 0;
    for (int i = 0; i < 12; i++) {
        const uint64_t t = (uint64_t)v[i] - p[i] - borrow;
        d[i] = (uint32_t)t;
        borrow = (t >> 32) & 1;
    }
    if (!borrow) memcpy(v, d, 48);
}
static void times_2_14(uint32_t v[12]) {  // v < p -> v 2^14 mod p
    for (int k = 0; k < 14; k++) {
        for (int i = 11; i > 0; i--) v[i] = (v[i] << 1) | (v[i - 1] >> 31);
        v[0] <<= 1;
        reduce_once(v);
    }
}
static void row29_coord(uint32_t sector[16], const uint32_t words28[12]) {  // the r04 coordinate x 2^14 as thirteen 29-bit limbs
    uint32_t v[12];
    memcpy(v, words28, 48);
    times_2_14(v);
    memset(sector, 0, 64);
    for (int i = 0; i < 13; i++) {
        const int bit = 29 * i, w = bit >> 5, off = bit & 31;
        uint32_t x = v[w] >> off;
        if (off > 3 && w + 1 < 12) x |= v[w + 1] << (32 - off);
        sector[i] = x & 0x1fffffffu;
    }
}
static bool same_mod_p(std::vector<G1XYZZ>& a, std::vector<G1XYZZ>& b) {
    for (auto* v : {&a, &b})
        for (auto& pt : *v) {
            reduce_once(pt.x.v);
            reduce_once(pt.y.v);
            reduce_once(pt.zz.v);
            reduce_once(pt.zzz.v);
        }
    return memcmp(a.data(), b.data(), a.size() * sizeof(G1XYZZ)) == 0;
}

template <class F>
static int time_kernel(const char* name, F launch, uint32_t lanes, uint32_t chain) {
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int i = 0; i < 3; i++) launch();
    CHECK(hipDeviceSynchronize());
    const int reps = 10;
    CHECK(hipEventRecord(e0));
    for (int i = 0; i < reps; i++) launch();
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    ms /= reps;
    printf("{\"variant\": \"%s\", \"lanes\": %u, \"chain\": %u, \"ms\": %.4f, \"mixed_adds_per_s\": %.4g}\n", name, lanes, chain, ms,
           (double)lanes * (chain - 1) / (ms * 1e-3));
    return 0;
}

int main() {
    const uint32_t nrows = 1u << 14, chain = 48;
    const uint32_t lanes = 256 * 256 * 12;  // twelve workgroups per CU: whole waves of work at 3 and at 4 waves per SIMD
    std::vector<RowPacked> hp(nrows);
    std::vector<G1TE> hu(nrows);
    memset(hu.data(), 0, nrows * sizeof(G1TE));
    for (uint32_t r = 0; r < nrows; r++) {
        rand_coord(hu[r].ymx, hp[r].ymx.v);
        rand_coord(hu[r].ypx, hp[r].ypx.v);
        rand_coord(hu[r].kt, hp[r].kt.v);
    }
    std::vector<G1TE> hn(nrows);
    for (uint32_t r = 0; r < nrows; r++) {
        row29_coord(hn[r].ymx, hp[r].ymx.v);
        row29_coord(hn[r].ypx, hp[r].ypx.v);
        row29_coord(hn[r].kt, hp[r].kt.v);
    }
    std::vector<uint32_t> hidx((size_t)lanes * chain);
    for (auto& v : hidx) v = (rnd() % nrows) | ((rnd() & 1u) << 31);
    RowPacked* dp;
    G1TE *du, *dn;
    uint32_t *didx, *dbad, *dmul;
    G1XYZZ *o3, *o4, *o4f, *o29;
    CHECK(hipMalloc(&dn, nrows * sizeof(G1TE)));
    CHECK(hipMalloc(&o29, (size_t)lanes * sizeof(G1XYZZ)));
    CHECK(hipMemcpy(dn, hn.data(), nrows * sizeof(G1TE), hipMemcpyHostToDevice));
    CHECK(hipMalloc(&dp, nrows * sizeof(RowPacked)));
    CHECK(hipMalloc(&du, nrows * sizeof(G1TE)));
    CHECK(hipMalloc(&didx, hidx.size() * 4));
    CHECK(hipMalloc(&o3, (size_t)lanes * sizeof(G1XYZZ)));
    CHECK(hipMalloc(&o4, (size_t)lanes * sizeof(G1XYZZ)));
    CHECK(hipMalloc(&o4f, (size_t)lanes * sizeof(G1XYZZ)));
    CHECK(hipMalloc(&dbad, 4));
    CHECK(hipMemcpy(dp, hp.data(), nrows * sizeof(RowPacked), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(du, hu.data(), nrows * sizeof(G1TE), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(didx, hidx.data(), hidx.size() * 4, hipMemcpyHostToDevice));
    // the multiplier alone on lazy operands
    {
        const uint32_t n = 1u << 16;
        std::vector<uint32_t> hm((size_t)n * 28);
        for (size_t i = 0; i < hm.size(); i++) hm[i] = (i % 14 == 13) ? (rnd() & 0x3ffffu) : (rnd() & 0x3fffffffu);  // limbs < 2^30, value < 128 p
        CHECK(hipMalloc(&dmul, hm.size() * 4));
        CHECK(hipMemcpy(dmul, hm.data(), hm.size() * 4, hipMemcpyHostToDevice));
        CHECK(hipMemset(dbad, 0, 4));
        k_mul_check<<<n / 256, 256>>>(dmul, dbad);
        uint32_t bad = 1;
        CHECK(hipMemcpy(&bad, dbad, 4, hipMemcpyDeviceToHost));
        printf("{\"check\": \"fq28_mul_asm == fq28_mul on %u lazy operand pairs (and squares)\", \"mismatches\": %u}\n", n, bad);
        if (bad) return 2;
    }
    {
        const uint32_t n = 1u << 16;
        std::vector<uint32_t> hm((size_t)n * 26);
        for (size_t i = 0; i < hm.size(); i++) hm[i] = (i % 26 < 13) ? rnd() % 0x60000000u : (rnd() & 0x1fffffffu);
        uint32_t* dm29;
        CHECK(hipMalloc(&dm29, hm.size() * 4));
        CHECK(hipMemcpy(dm29, hm.data(), hm.size() * 4, hipMemcpyHostToDevice));
        CHECK(hipMemset(dbad, 0, 4));
        k_mul29_check<<<n / 256, 256>>>(dm29, dbad);
        uint32_t bad = 1;
        CHECK(hipMemcpy(&bad, dbad, 4, hipMemcpyDeviceToHost));
        printf("{\"check\": \"fq29_mul_asm == fq29_mul on %u operand pairs (and squares)\", \"mismatches\": %u}\n", n, bad);
        if (bad) return 2;
    }
    const dim3 grid(lanes / 256), block(256);
    if (time_kernel("r03 packed rows, compiler multiplier, 3 waves", [&] { k_r03<3><<<grid, block>>>(dp, didx, chain, o3); }, lanes, chain)) return 1;
    if (time_kernel("r04 limb rows, compiler multiplier, 3 waves", [&] { k_r04<3, MulFenced><<<grid, block>>>(du, didx, chain, o4f); }, lanes, chain)) return 1;
    if (time_kernel("r04 limb rows, asm multiplier, 3 waves", [&] { k_r04<3, MulAsm><<<grid, block>>>(du, didx, chain, o4); }, lanes, chain)) return 1;
    std::vector<G1XYZZ> h3(lanes), h4(lanes), h4f(lanes);
    CHECK(hipMemcpy(h3.data(), o3, (size_t)lanes * sizeof(G1XYZZ), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h4.data(), o4, (size_t)lanes * sizeof(G1XYZZ), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h4f.data(), o4f, (size_t)lanes * sizeof(G1XYZZ), hipMemcpyDeviceToHost));
    const bool same = memcmp(h3.data(), h4.data(), (size_t)lanes * sizeof(G1XYZZ)) == 0 &&
                      memcmp(h3.data(), h4f.data(), (size_t)lanes * sizeof(G1XYZZ)) == 0;
    if (time_kernel("r04 limb rows, asm multiplier, 4 waves", [&] { k_r04<4, MulAsm><<<grid, block>>>(du, didx, chain, o4); }, lanes, chain)) return 1;
    CHECK(hipMemcpy(h4.data(), o4, (size_t)lanes * sizeof(G1XYZZ), hipMemcpyDeviceToHost));
    const bool same4 = memcmp(h3.data(), h4.data(), (size_t)lanes * sizeof(G1XYZZ)) == 0;
    printf("{\"identical\": \"%s\", \"lanes_compared\": %u}\n", same && same4 ? "yes" : "NO", lanes);
    if (!(same && same4)) return 3;
    // old form against new, alternating, so that the spread of repeated runs shows beside the difference
    for (int rep = 0; rep < 5; rep++) {
        if (time_kernel("r04 limb rows, asm multiplier, 3 waves", [&] { k_r04<3, MulAsm><<<grid, block>>>(du, didx, chain, o4); }, lanes, chain)) return 1;
        if (time_kernel("te29 rows, asm multiplier, 3 waves", [&] { k_te29<3, Mul29Asm><<<grid, block>>>(dn, didx, chain, o29); }, lanes, chain)) return 1;
    }
    std::vector<G1XYZZ> h29(lanes);
    CHECK(hipMemcpy(h29.data(), o29, (size_t)lanes * sizeof(G1XYZZ), hipMemcpyDeviceToHost));
    const bool eq3 = same_mod_p(h29, h4);
    if (time_kernel("te29 rows, compiler multiplier, 3 waves", [&] { k_te29<3, Mul29Fenced><<<grid, block>>>(dn, didx, chain, o29); }, lanes, chain)) return 1;
    CHECK(hipMemcpy(h29.data(), o29, (size_t)lanes * sizeof(G1XYZZ), hipMemcpyDeviceToHost));
    const bool eqf = same_mod_p(h29, h4);
    if (time_kernel("te29 rows, asm multiplier, 4 waves", [&] { k_te29<4, Mul29Asm><<<grid, block>>>(dn, didx, chain, o29); }, lanes, chain)) return 1;
    CHECK(hipMemcpy(h29.data(), o29, (size_t)lanes * sizeof(G1XYZZ), hipMemcpyDeviceToHost));
    const bool eq4 = same_mod_p(h29, h4);
    printf("{\"te29 equals r04 mod p\": \"%s\", \"lanes_compared\": %u}\n", eq3 && eqf && eq4 ? "yes" : "NO", lanes);
    return eq3 && eqf && eq4 ? 0 : 4;
}

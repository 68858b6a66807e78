// merkle_stage.cuh — ONE Pedersen hash with the witnesses of its conditional additions, as merkle_witness.hip (the membership
// circuit, a path's stages in sequence) and pedersen_payment_witness.hip (one stage per workgroup) share it.  One lane per 4-bit
// window, WAVES waves of 64 lanes: two for the 128 windows of a two-to-one hash, three for the 144 windows of a 72-byte leaf.
// Every witness of a hash is a pointwise function of the affine prefix sums P_k = sum_{i <= k} bit_i G_i:
//   1. lane w looks its window's point up in the resident table of swm_pedersen (one mixed addition from the identity);
//   2. an exclusive scan of the window points with the unified addition: shuffles inside a wave, LDS across the wave boundaries;
//   3. from its prefix each lane walks its four bits with mixed additions against the rows 1 << j: the running sums;
//   4. ONE inversion normalises all of them: products of four Z per lane, a prefix and a suffix product scan over the lanes, the
//      inverse of the total on one lane (frinv.cuh), three multiplications back to each lane's product and six to its four Z;
//   5. the six witnesses of step k — t = X Y, b t, m1, m2, X3, Y3 — from P_{k-1}, P_k and the generator's (cx, cy), which the
//      table row 1 << j gives as ((y + x) -+ (y - x)) / 2.
// The law is complete (ed.cuh): identity windows, zero bits and repeated points take the same path and no Z is zero.
#pragma once
#include <hip/hip_runtime.h>

#include "ed.cuh"
#include "ff.cuh"
#include "frinv.cuh"
#include "host/merkle_shape.h"

namespace swm {

template <unsigned WAVES>
struct MwStage {
    static constexpr unsigned LANES = 64 * WAVES;
    EdExt wave_total[WAVES - 1];      // the sum of wave w's window points, w < WAVES - 1
    Fr cross_pre[WAVES - 1];          // wave w's Z product, for the waves above it
    Fr cross_suf[WAVES - 1];          // wave w + 1's Z product, for the waves below it
    Fr inv;                           // the inverse of the product of all Z
    Fr last_x[LANES], last_y[LANES];  // each lane's last affine running sum (the next lane's P_{k-1})
    uint32_t cur[8];                  // the digest, canonical
};

__device__ __forceinline__ Fr fr_shfl_up(const Fr& a, unsigned d) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)__shfl_up((int)a.v[i], d, 64);
    return r;
}
__device__ __forceinline__ Fr fr_shfl_down(const Fr& a, unsigned d) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)__shfl_down((int)a.v[i], d, 64);
    return r;
}
__device__ __forceinline__ EdExt ed_shfl_up(const EdExt& p, unsigned d) {
    EdExt r;
    r.x = fr_shfl_up(p.x, d);
    r.y = fr_shfl_up(p.y, d);
    r.t = fr_shfl_up(p.t, d);
    r.z = fr_shfl_up(p.z, d);
    return r;
}

// One Pedersen hash of `nbits` bits (4 per lane; `nib` is zero on the lanes past the input) with the witnesses of its
// conditional additions: step k = 1 .. nbits - 1 at out[6 (k - 1) .. + 6).  Leaves the digest, canonical, in sh.cur (the caller
// synchronises before reading it).  Called by all 64 WAVES lanes; the lanes past the input carry the sum along, so the last lane
// always holds the hash.
template <unsigned WAVES>
__device__ __noinline__ void mw_hash_stage(const EdRow* __restrict__ table, unsigned nib, unsigned nbits, Fr* __restrict__ out,
                                           const Fr k2d, const Fr half, MwStage<WAVES>& sh) {
    constexpr unsigned LANES = 64 * WAVES;
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const EdRow* rows = table + ((size_t)tid << 4);  // only read where nib has a bit: never past the windows the input fills
    // 1. + 2.
    EdExt acc = ed_identity();
    if (nib) ed_madd(acc, rows[nib]);
#pragma unroll 1
    for (unsigned d = 1; d < 64; d <<= 1) {
        const EdExt o = ed_shfl_up(acc, d);
        if (lane >= d) acc = ed_add(o, acc, k2d);
    }
    if (lane == 63 && wave < WAVES - 1) sh.wave_total[wave] = acc;
    __syncthreads();
    EdExt carry = ed_identity();  // the sum of the waves below
    if (wave) {
        carry = sh.wave_total[0];
#pragma unroll 1
        for (unsigned v = 1; v < wave; v++) carry = ed_add(carry, sh.wave_total[v], k2d);
        acc = ed_add(carry, acc, k2d);
    }
    EdExt q = ed_shfl_up(acc, 1);
    if (lane == 0) q = carry;
    // 3.
    Fr px[4], py[4], pz[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if ((nib >> j) & 1u) ed_madd(q, rows[1u << j]);
        px[j] = q.x;
        py[j] = q.y;
        pz[j] = q.z;
    }
    // 4.
    const Fr a1 = fp_mul(pz[0], pz[1]), a2 = fp_mul(a1, pz[2]), prod = fp_mul(a2, pz[3]);
    Fr pre = prod, suf = prod;  // inclusive products over the lanes below / above
#pragma unroll 1
    for (unsigned d = 1; d < 64; d <<= 1) {
        const Fr o = fr_shfl_up(pre, d);
        const Fr u = fr_shfl_down(suf, d);
        if (lane >= d) pre = fp_mul(o, pre);
        if (lane + d < 64) suf = fp_mul(u, suf);
    }
    if (lane == 63 && wave < WAVES - 1) sh.cross_pre[wave] = pre;
    if (lane == 0 && wave) sh.cross_suf[wave - 1] = suf;
    __syncthreads();
    Fr lo = fp_one<Fr>(), hi = fp_one<Fr>();  // the Z products of the waves below / above
    if (wave) {
        lo = sh.cross_pre[0];
#pragma unroll 1
        for (unsigned v = 1; v < wave; v++) lo = fp_mul(lo, sh.cross_pre[v]);
        pre = fp_mul(lo, pre);
    }
    if (wave < WAVES - 1) {
        hi = sh.cross_suf[wave];
#pragma unroll 1
        for (unsigned v = wave + 1; v < WAVES - 1; v++) hi = fp_mul(hi, sh.cross_suf[v]);
        suf = fp_mul(suf, hi);
    }
    Fr below = fr_shfl_up(pre, 1), above = fr_shfl_down(suf, 1);  // exclusive
    if (lane == 0) below = lo;
    if (lane == 63) above = hi;
    if (tid == LANES - 1) sh.inv = fr_inv_single(pre);  // the total: no Z is zero
    __syncthreads();
    const Fr inv_prod = fp_mul(fp_mul(below, above), sh.inv);
    Fr iz[4];
    iz[3] = fp_mul(inv_prod, a2);
    const Fr inv_a2 = fp_mul(inv_prod, pz[3]);
    iz[2] = fp_mul(inv_a2, a1);
    const Fr inv_a1 = fp_mul(inv_a2, pz[2]);
    iz[1] = fp_mul(inv_a1, pz[0]);
    iz[0] = fp_mul(inv_a1, pz[1]);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        px[j] = fp_mul(px[j], iz[j]);
        py[j] = fp_mul(py[j], iz[j]);
    }
    sh.last_x[tid] = px[3];
    sh.last_y[tid] = py[3];
    __syncthreads();
    // 5.
    Fr X = tid ? sh.last_x[tid - 1] : fp_zero<Fr>();
    Fr Y = tid ? sh.last_y[tid - 1] : fp_one<Fr>();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned k = 4 * tid + j;
        if (k >= 1 && k < nbits) {  // the first bit of a hash is linear in the bit: no witness
            Fr* o = out + MW_COND_ADD * (size_t)(k - 1);
            const Fr t = fp_mul(X, Y);
            o[0] = t;
            if ((nib >> j) & 1u) {
                const EdRow g = rows[1u << j];
                const Fr cx = fp_mul(half, fp_sub(g.ypx, g.ymx)), cy = fp_mul(half, fp_add(g.ypx, g.ymx));
                const Fr cym1 = fp_sub(cy, fp_one<Fr>());
                o[1] = t;
                o[2] = fp_add(fp_mul(cym1, X), fp_mul(cx, Y));
                o[3] = fp_add(fp_mul(cym1, Y), fp_mul(cx, X));
            } else {
                o[1] = fp_zero<Fr>();
                o[2] = fp_zero<Fr>();
                o[3] = fp_zero<Fr>();
            }
            o[4] = px[j];
            o[5] = py[j];
        }
        X = px[j];
        Y = py[j];
    }
    if (tid == LANES - 1) {
        const Fr x = fp_to_std(px[3]);
#pragma unroll
        for (int i = 0; i < 8; i++) sh.cur[i] = x.v[i];
    }
}

}  // namespace swm

// ed_witness.cuh — curve witnesses over one workgroup of 256 lanes, lane i on bit i of a scalar: what schnorr_witness.hip and
// elgamal_witness.hip share.  An inclusive scan of one point per lane with the unified addition, ONE inversion for the Z of
// every lane, the seven witnesses of an affine addition, and the two checks of a point that arrives in wire form.  The
// functions that synchronise are called by all 256 lanes and keep their partial results in SvScanShared, which a kernel's own
// __shared__ struct derives from.
#pragma once
#include <hip/hip_runtime.h>

#include "ed.cuh"
#include "ff.cuh"
#include "frinv.cuh"

namespace swm {

static constexpr unsigned SV_LANES = 256;  // = bits of a scalar
static constexpr unsigned SV_WAVES = SV_LANES / 64;

struct SvScanShared {
    EdExt wave_sum[SV_WAVES];
    Fr wave_prod[SV_WAVES];
    Fr inv;
};

__device__ __forceinline__ Fr sv_shfl_up(const Fr& a, unsigned d) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)__shfl_up((int)a.v[i], d, 64);
    return r;
}
__device__ __forceinline__ Fr sv_shfl_down(const Fr& a, unsigned d) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)__shfl_down((int)a.v[i], d, 64);
    return r;
}
__device__ __forceinline__ EdExt sv_ed_shfl_up(const EdExt& p, unsigned d) {
    EdExt r;
    r.x = sv_shfl_up(p.x, d);
    r.y = sv_shfl_up(p.y, d);
    r.t = sv_shfl_up(p.t, d);
    r.z = sv_shfl_up(p.z, d);
    return r;
}

// Inclusive scan of one point per lane over the 256 lanes.  Called by all lanes; synchronises.
__device__ __noinline__ EdExt sv_scan(EdExt acc, const Fr k2d, SvScanShared& sh) {
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll 1
    for (unsigned d = 1; d < 64; d <<= 1) {
        const EdExt o = sv_ed_shfl_up(acc, d);
        if (lane >= d) acc = ed_add(o, acc, k2d);
    }
    if (lane == 63) sh.wave_sum[wave] = acc;
    __syncthreads();
    if (wave) {
        EdExt below = sh.wave_sum[0];
#pragma unroll 1
        for (unsigned k = 1; k < wave; k++) below = ed_add(below, sh.wave_sum[k], k2d);
        acc = ed_add(below, acc, k2d);
    }
    __syncthreads();  // wave_sum[] has been read
    return acc;
}

// 1 / z of every lane with ONE inversion: prefix and suffix products over the lanes, the inverse of the total on one lane
// (frinv.cuh), two multiplications back.  No z is zero.  Called by all lanes; synchronises.
__device__ __noinline__ Fr sv_batch_inv(const Fr z, SvScanShared& sh) {
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Fr pre = z, suf = z;  // inclusive products over the lanes below / above, within the wave
#pragma unroll 1
    for (unsigned d = 1; d < 64; d <<= 1) {
        const Fr o = sv_shfl_up(pre, d);
        const Fr u = sv_shfl_down(suf, d);
        if (lane >= d) pre = fp_mul(o, pre);
        if (lane + d < 64) suf = fp_mul(u, suf);
    }
    if (lane == 63) sh.wave_prod[wave] = pre;
    __syncthreads();
    Fr below = sv_shfl_up(pre, 1), above = sv_shfl_down(suf, 1);  // exclusive
    if (lane == 0) below = fp_one<Fr>();
    if (lane == 63) above = fp_one<Fr>();
#pragma unroll 1
    for (unsigned k = 0; k < SV_WAVES; k++) {
        if (k < wave) below = fp_mul(sh.wave_prod[k], below);
        if (k > wave) above = fp_mul(above, sh.wave_prod[k]);
    }
    if (tid == 0) {
        Fr total = sh.wave_prod[0];
#pragma unroll 1
        for (unsigned k = 1; k < SV_WAVES; k++) total = fp_mul(total, sh.wave_prod[k]);
        sh.inv = fr_inv_single(total);
    }
    __syncthreads();
    const Fr r = fp_mul(fp_mul(below, above), sh.inv);
    __syncthreads();  // wave_prod[] and inv have been read
    return r;
}

__device__ __forceinline__ EdExt sv_from_affine(const Fr& x, const Fr& y) {
    EdExt p;
    p.x = x;
    p.y = y;
    p.t = fp_mul(x, y);
    p.z = fp_one<Fr>();
    return p;
}

// x1y2, y1x2, y1y2, x1x2, their product, x3, y3 of (x1, y1) + (x2, y2) = (x3, y3)
__device__ __forceinline__ void sv_add_witnesses(Fr* o, const Fr& x1, const Fr& y1, const Fr& x2, const Fr& y2, const Fr& x3, const Fr& y3) {
    const Fr a = fp_mul(x1, y2), b = fp_mul(y1, x2);
    o[0] = a;
    o[1] = b;
    o[2] = fp_mul(y1, y2);
    o[3] = fp_mul(x1, x2);
    o[4] = fp_mul(a, b);
    o[5] = x3;
    o[6] = y3;
}

SWM_HD bool sv_canonical(const uint32_t* w, Fr* mont) {
    Fr s, r;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        s.v[i] = w[i];
        r.v[i] = FrParams::P[i];
    }
    if (fp_cmp_std(s, r) >= 0) return false;
    *mont = fp_from_std(s);
    return true;
}
// -x^2 + y^2 == 1 + d x^2 y^2
SWM_HD bool sv_on_curve(const Fr& x, const Fr& y, const Fr& d) {
    const Fr x2 = fp_sqr(x), y2 = fp_sqr(y);
    return fp_eq(fp_sub(y2, x2), fp_add(fp_one<Fr>(), fp_mul(d, fp_mul(x2, y2))));
}

}  // namespace swm

// msm_table.hip — the base sets of the G1 MSM (msm.h): the scaled copy of a set, the window multiples of a resident set as XYZZ
// or twisted Edwards rows (msm_table_build[_te], msm_install_bases), the batch normalisation the universal setup shares
// (msm_normalize_run) and the subgroup check of key deserialisation (msm_subgroup_check).  The window layouts the tables are
// built for (msm_table_layout, msm_table_width) are the sort's: msm_sort.hip.
#include <algorithm>
#include "context.h"
#include "fq28.cuh"
#include "fq29.cuh"
#include "g1.cuh"
#include "msm_stages.h"

namespace swm {

// ---- table construction: out[i] = 2^k in[i] as XYZZ (k doublings), then batch normalisation back to affine
__global__ void __launch_bounds__(256) msm_table_shift(const G1Affine* __restrict__ in, size_t n, unsigned k, G1XYZZ* __restrict__ out) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1Affine p = in[i];
    G1XYZZ acc = g1_is_inf(p) ? g1_xyzz_identity() : g1_dbl_affine(p);
    for (unsigned j = 1; j < k; j++) acc = g1_dbl(acc);
    out[i] = acc;
}
// Jacobian-free batch normalisation: 16 consecutive points per lane, prefix products parked in `pref`
static constexpr int TAB_NORM_CHUNK = 16;
__global__ void __launch_bounds__(256) msm_table_normalize(const G1XYZZ* __restrict__ in, size_t n, Fq* __restrict__ pref,
                                                           G1Affine* __restrict__ out) {
    size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    size_t lo = t * TAB_NORM_CHUNK;
    if (lo >= n) return;
    size_t hi = lo + TAB_NORM_CHUNK < n ? lo + TAB_NORM_CHUNK : n;
    Fq acc = fp_one<Fq>();
    for (size_t i = lo; i < hi; i++) {
        pref[i] = acc;
        if (!fp_is_zero(in[i].zz)) acc = fp_mul(acc, fp_mul(in[i].zz, in[i].zzz));
    }
    Fq inv = fp_inv(acc);
    for (size_t i = hi; i-- > lo;) {
        G1XYZZ p = in[i];
        G1Affine a;
        if (fp_is_zero(p.zz)) {
            a.x = fp_zero<Fq>();
            a.y = fp_zero<Fq>();
        } else {
            Fq zi = fp_mul(inv, pref[i]);
            inv = fp_mul(inv, fp_mul(p.zz, p.zzz));
            a.x = fp_mul(p.x, fp_mul(zi, p.zzz));
            a.y = fp_mul(p.y, fp_mul(zi, p.zz));
        }
        out[i] = a;
    }
}

// affine points on y^2 = x^3 + 1 (plain form, radix 2^384) -> twisted Edwards table rows (y - x, y + x, 2 d x y), each
// coordinate x 2^22 (Montgomery radix 2^406) as the thirteen 29-bit limbs msm_accumulate_te multiplies (fq29.cuh) — or, LIMB29
// off, x 2^8 as fourteen 28-bit limbs: the rows of the te28_* functions, kept for the self-test.
// x = f (x_w + 1)/y_w, y = (u - 1)/(u + 1), u = s (x_w + 1): one inversion per TAB_NORM_CHUNK points (of the product of their
// y_w (u + 1)).  The identity (0, 0) becomes the row (1, 1, 0) of (0, 1).
// A point with y_w (u + 1) = 0 (order 2, or mapped to infinity: never in the prime-order subgroup) raises *bad.
template <int N>  // one coordinate's N limbs, zero padded, as the four 16-byte stores of its sector
__device__ __forceinline__ void te_store_sector(uint4* o, const uint32_t (&l)[N]) {
    o[0] = make_uint4(l[0], l[1], l[2], l[3]);
    o[1] = make_uint4(l[4], l[5], l[6], l[7]);
    o[2] = make_uint4(l[8], l[9], l[10], l[11]);
    o[3] = make_uint4(l[12], N > 13 ? l[N - 1] : 0u, 0u, 0u);
}
template <bool LIMB29>
__global__ void __launch_bounds__(256) msm_te_convert(const G1Affine* __restrict__ in, size_t n, Fq* __restrict__ pref,
                                                      G1TE* __restrict__ out, uint32_t* __restrict__ bad) {
    size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    size_t lo = t * TAB_NORM_CHUNK;
    if (lo >= n) return;
    size_t hi = lo + TAB_NORM_CHUNK < n ? lo + TAB_NORM_CHUNK : n;
    const Fq one = fp_one<Fq>(), cs = fq_const(TeParams::S);
    Fq acc = one;
    for (size_t i = lo; i < hi; i++) {
        G1Affine p = in[i];
        pref[i] = acc;
        if (g1_is_inf(p)) continue;
        Fq den = fp_mul(p.y, fp_add(fp_mul(cs, fp_add(p.x, one)), one));
        if (fp_is_zero(den)) atomicOr(bad, 1u);
        else acc = fp_mul(acc, den);
    }
    Fq inv = fp_inv(acc);
    const uint32_t k256[12] = SWM_FQ_SCALE256_MONT, k22[12] = SWM_FQ_SCALE22_MONT;
    Fq c256, one256;  // the scale of the limb form (2^8, or 2^22 for LIMB29) and one in it
#pragma unroll
    for (int j = 0; j < 12; j++) c256.v[j] = LIMB29 ? k22[j] : k256[j];
    one256 = fp_mul(one, c256);
    for (size_t i = hi; i-- > lo;) {
        G1Affine p = in[i];
        Fq ymx, ypx, kt;
        Fq x1 = fp_add(p.x, one), u = fp_mul(cs, x1), up1 = fp_add(u, one), den = fp_mul(p.y, up1);
        if (g1_is_inf(p) || fp_is_zero(den)) {
            ymx = one256;
            ypx = one256;
            kt = fp_zero<Fq>();
        } else {
            Fq di = fp_mul(inv, pref[i]);
            inv = fp_mul(inv, den);
            Fq xt = fp_mul(fp_mul(fq_const(TeParams::F), x1), fp_mul(di, up1));  // f (x_w + 1) / y_w
            Fq yt = fp_mul(fp_sub(u, one), fp_mul(di, p.y));                       // (u - 1) / (u + 1)
            ymx = fp_mul(fp_sub(yt, xt), c256);
            ypx = fp_mul(fp_add(yt, xt), c256);
            kt = fp_mul(fp_mul(fq_const(TeParams::K2D), fp_mul(xt, yt)), c256);
        }
        // canonical values split into the limbs the accumulation multiplies, one 64-byte sector per coordinate
        uint4* o = reinterpret_cast<uint4*>(&out[i]);
        if (LIMB29) {
            te_store_sector<13>(o, fq29_unpack(ymx).l);
            te_store_sector<13>(o + 4, fq29_unpack(ypx).l);
            te_store_sector<13>(o + 8, fq29_unpack(kt).l);
        } else {
            te_store_sector<14>(o, fq28_unpack(ymx).l);
            te_store_sector<14>(o + 4, fq28_unpack(ypx).l);
            te_store_sector<14>(o + 8, fq28_unpack(kt).l);
        }
    }
}
// [r]P = O and P on the curve, for every point that is not the identity (0, 0): double-and-add over the 253 bits of r
__global__ void __launch_bounds__(256) msm_subgroup_kernel(const G1Affine* __restrict__ in, size_t n, uint32_t* __restrict__ bad) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1Affine p = in[i];
    if (g1_is_inf(p)) return;
    if (!g1_is_on_curve(p)) {
        atomicOr(bad, 1u);
        return;
    }
    G1XYZZ acc = g1_xyzz_identity();
    bool started = false;
#pragma unroll 1
    for (int b = 252; b >= 0; b--) {
        if (started) acc = g1_dbl(acc);
        if ((FrParams::P[b >> 5] >> (b & 31)) & 1) {
            g1_add_mixed(acc, p);
            started = true;
        }
    }
    if (!g1_is_inf(acc)) atomicOr(bad, 2u);
}

// bases28[i] = (2^8 x, 2^8 y): the same points with coordinates in Montgomery radix 2^392 (infinity stays (0, 0))
__global__ void __launch_bounds__(256) msm_scale_bases(const G1Affine* __restrict__ in, size_t n, G1Affine* __restrict__ out,
                                                       uint32_t* __restrict__ inf_mask) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (inf_mask) {
        uint32_t z = 0;
        for (int j = 0; j < 12; j++) z |= in[i].x.v[j] | in[i].y.v[j];
        if (z == 0) atomicOr(&inf_mask[i >> 5], 1u << (i & 31));
    }
    const uint32_t k[12] = SWM_FQ_SCALE256_MONT;
    Fq c;
#pragma unroll
    for (int j = 0; j < 12; j++) c.v[j] = k[j];
    G1Affine p = in[i];
    p.x = fp_mul(p.x, c);
    p.y = fp_mul(p.y, c);
    out[i] = p;
}
int msm_scale_bases_run(swm_ctx* ctx, const G1Affine* d_in, size_t n, G1Affine* d_out, uint32_t* d_inf_mask) {
    if (n == 0) return SWM_OK;
    SWM_LAUNCH(ctx, "msm_scale_bases", msm_scale_bases, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d_in, n, d_out,
               d_inf_mask);
    return SWM_OK;
}

// The rows w = 0 .. W - 1 of the table of d_points[0 .. n) for width c, 2^(bit_w) P each: scaled affine points (row 0 is the plain
// scaled copy of the set) or, te, twisted Edwards points.  te: *out stays null (and SWM_OK is returned) when a point has no image.
static int msm_table_rows(swm_ctx* ctx, const G1Affine* d_points, size_t n, unsigned c, bool te, void** out) {
    *out = nullptr;
    if (n == 0 || c < 2) return set_err(ctx, SWM_ERR_INVALID_ARG, "msm table: bad arguments");
    const WinLayout L = msm_table_layout(c);
    const unsigned W = L.nwin;
    const size_t row = n * (te ? sizeof(G1TE) : sizeof(G1Affine));
    char* tab = nullptr;
    hipError_t e = hipMalloc((void**)&tab, W * row);
    if (e != hipSuccess) (void)hipGetLastError();  // not sticky: the caller falls back to a smaller form
    if (e != hipSuccess) return set_err(ctx, SWM_ERR_OOM, "msm table (%u windows x %zu points): %s", W, n, hipGetErrorString(e));
    G1XYZZ* x = nullptr;
    Fq* pref = nullptr;
    G1Affine* cur = nullptr;  // 2^(bit_w) P in the plain form, input of the next shift
    uint32_t* d_bad = nullptr;
    uint32_t bad = 0;
    int rc = SWM_OK;
    do {
        if ((rc = scratch(ctx, "tab.xyzz", n * sizeof(G1XYZZ), (void**)&x)) != SWM_OK) break;
        if ((rc = scratch(ctx, "tab.pref", n * sizeof(Fq), (void**)&pref)) != SWM_OK) break;
        if ((rc = scratch(ctx, "tab.cur", n * sizeof(G1Affine), (void**)&cur)) != SWM_OK) break;
        if (te && (rc = scratch(ctx, "tab.bad", 64, (void**)&d_bad)) != SWM_OK) break;
        if (te && hipMemsetAsync(d_bad, 0, 4, ctx->stream) != hipSuccess) {
            rc = set_err(ctx, SWM_ERR_HIP, "msm table: memset failed");
            break;
        }
        const G1Affine* src = d_points;
        const unsigned grid = (unsigned)((n + 255) / 256), gridn = (unsigned)(((n + TAB_NORM_CHUNK - 1) / TAB_NORM_CHUNK + 255) / 256);
        for (unsigned w = 0; w < W && rc == SWM_OK; w++) {
            if (w > 0) {
                hipLaunchKernelGGL(msm_table_shift, dim3(grid), dim3(256), 0, ctx->stream, src, n, (unsigned)L.c[w - 1], x);
                hipLaunchKernelGGL(msm_table_normalize, dim3(gridn), dim3(256), 0, ctx->stream, (const G1XYZZ*)x, n, pref, cur);
                src = cur;
            }
            if (te) hipLaunchKernelGGL(msm_te_convert<true>, dim3(gridn), dim3(256), 0, ctx->stream, src, n, pref, (G1TE*)(tab + w * row), d_bad);
            if (hipGetLastError() != hipSuccess) rc = set_err(ctx, SWM_ERR_HIP, "msm table: launch failed");
            if (rc == SWM_OK && !te) rc = msm_scale_bases_run(ctx, src, n, (G1Affine*)(tab + w * row));
        }
        if (rc == SWM_OK && ((te && hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) ||
                             hipStreamSynchronize(ctx->stream) != hipSuccess))
            rc = set_err(ctx, SWM_ERR_HIP, "msm table: sync failed");
    } while (0);
    scratch_release(ctx, "tab.xyzz");
    scratch_release(ctx, "tab.pref");
    scratch_release(ctx, "tab.cur");
    if (rc != SWM_OK || bad) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(tab);
        return rc;  // bad: SWM_OK with *out == nullptr — a point without an image; the caller keeps the XYZZ form
    }
    *out = tab;
    return SWM_OK;
}
int msm_table_build(swm_ctx* ctx, const G1Affine* d_points, size_t n, unsigned c, G1Affine** out) {
    return msm_table_rows(ctx, d_points, n, c, false, (void**)out);
}
int msm_table_build_te(swm_ctx* ctx, const G1Affine* d_points, size_t n, unsigned c, G1TE** out) {
    return msm_table_rows(ctx, d_points, n, c, true, (void**)out);
}
int msm_normalize_run(swm_ctx* ctx, const G1XYZZ* in, size_t n, Fq* pref, G1Affine* out) {
    const unsigned grid = (unsigned)(((n + TAB_NORM_CHUNK - 1) / TAB_NORM_CHUNK + 255) / 256);
    SWM_LAUNCH(ctx, "srs_normalize", msm_table_normalize, dim3(grid), dim3(256), 0, in, n, pref, out);
    return SWM_OK;
}

bool msm_table_fits(size_t bytes) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return true;  // cannot tell: let the allocation decide
    return bytes <= free_b - free_b / 4;
}
int msm_subgroup_check(swm_ctx* ctx, const G1Affine* d_points, size_t n, bool* ok) {
    *ok = true;
    if (n == 0) return SWM_OK;
    uint32_t* d_bad = nullptr;
    SWM_TRY(scratch(ctx, "tab.bad", 64, (void**)&d_bad));
    SWM_HIP(ctx, hipMemsetAsync(d_bad, 0, 4, ctx->stream));
    SWM_LAUNCH(ctx, "msm_subgroup_check", msm_subgroup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d_points, n, d_bad);
    uint32_t h = 0;
    SWM_HIP(ctx, hipMemcpyAsync(&h, d_bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *ok = h == 0;
    return SWM_OK;
}
// Everything a resident base set needs for its MSMs, in one place (swm_srs_upload, the prover's committer keys):
//   *c    table width (0: the set is too small, its table would not fit, or n * windows >= 2^31 — per-window schedule only)
//   *te   twisted Edwards table when the set qualifies (subgroup established, SWM_MSM_TE != 0, it fits): the flat schedule
//         then runs in that form and *d28 is just the scaled copy of the set (n points) for the per-window schedule
//   *d28  otherwise the XYZZ table (row 0 = the scaled copy) when *c != 0, else the scaled copy
// A table that cannot be allocated is not an error: the next cheaper form is used (TE -> XYZZ table -> no table).
int msm_install_bases(swm_ctx* ctx, const G1Affine* d_points, size_t n, bool in_subgroup, G1Affine** d28, G1TE** te, unsigned* c,
                      uint32_t* d_inf_mask) {
    *d28 = nullptr;
    *te = nullptr;
    *c = msm_table_width(n);
    // A context that is one rank of a sharded proof (swm_set_msm_sharding before the key is built) accumulates n / G points per
    // MSM into the same bucket set, and the bucket stage — which every rank runs over all 2^(c-1) buckets — becomes the largest
    // replicated item: the table is as many bits narrower as the width rule gives for the rank's share of the set, at most
    // log2(G) - 1.  Measured per rank (tools/ubench/shard_emulate.py, same box): 2^20 constraints, G = 8: c = 20 / 18 / 17 ->
    // 23.7 / 20.9 / 20.9 ms; G = 4: flat; 2^22 constraints (1.5 M points per rank and more): 20 stays best (18: + 3 %).
    if (*c > 12 && ctx->shard_world >= 4 && !sw(SW_MSM_TABLE_C)) {
        unsigned lg = 0;
        while ((2u << lg) <= ctx->shard_world) lg++;
        const unsigned share = msm_table_width(std::max<size_t>(n / ctx->shard_world, 512));
        const unsigned delta = share && share < *c ? std::min(*c - share, lg - 1) : 0;
        *c = std::max(12u, *c - delta);
    }
    if (sw(SW_TRACE) >= 1) fprintf(stderr, "[swm] base set of %zu points: table width %u (world %u)\n", n, *c, ctx->shard_world);
    if (*c && (uint64_t)n * msm_table_windows(*c) >= (1ull << 31)) *c = 0;  // the sort addresses table rows with 31 bits
    const unsigned W = *c ? msm_table_windows(*c) : 0;
    if (*c && sw(SW_MSM_TE)) {
        bool ok = in_subgroup;
        if (!ok) SWM_TRY(msm_subgroup_check(ctx, d_points, n, &ok));
        if (ok && msm_table_fits((size_t)W * n * sizeof(G1TE) + n * sizeof(G1Affine))) {
            int rc = msm_table_build_te(ctx, d_points, n, *c, te);
            if (rc != SWM_OK && rc != SWM_ERR_OOM) return rc;
        }
    }
    if (*c && !*te) {
        int rc = SWM_ERR_OOM;
        if (msm_table_fits((size_t)W * n * sizeof(G1Affine))) rc = msm_table_build(ctx, d_points, n, *c, d28);
        if (rc == SWM_ERR_OOM) *c = 0;  // no room for a table: the per-window schedule needs 1x the set
        else if (rc != SWM_OK) return rc;
    }
    if (!*d28) {
        hipError_t e = hipMalloc((void**)d28, std::max<size_t>(n, 1) * sizeof(G1Affine));
        if (e != hipSuccess) {
            if (*te) (void)hipFree(*te);
            *te = nullptr;
            return set_err(ctx, SWM_ERR_OOM, "msm bases (%zu points): %s", n, hipGetErrorString(e));
        }
    }
    // the scaled copy (row 0 of an XYZZ table is written again: same bytes) and, when asked for, the infinity mask
    int rc = msm_scale_bases_run(ctx, d_points, n, *d28, d_inf_mask);
    if (rc == SWM_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = set_err(ctx, SWM_ERR_HIP, "msm bases: sync failed");
    if (rc != SWM_OK) {
        (void)hipFree(*d28);
        if (*te) (void)hipFree(*te);
        *d28 = nullptr;
        *te = nullptr;
    }
    return rc;
}

// The point-layer self-test's launch of msm_te_convert (msm_selftest.hip: P28T_ROWS, P28T_ROWS29), and the only reason this function
// exists: a kernel is launched in the unit that defines it, so the self-test cannot launch it itself.  The 28-bit rows
// (msm_te_convert<false>) are instantiated for it alone; the tables above are built from the 29-bit rows.
int msm_te_convert_run(swm_ctx* ctx, bool limb29, const G1Affine* in, size_t n, Fq* pref, G1TE* out, uint32_t* bad) {
    const unsigned gridn = (unsigned)(((n + TAB_NORM_CHUNK - 1) / TAB_NORM_CHUNK + 255) / 256);
    SWM_LAUNCH(ctx, "selftest_p28_rows", limb29 ? msm_te_convert<true> : msm_te_convert<false>, dim3(gridn), dim3(256), 0, in, n, pref,
               out, bad);
    return SWM_OK;
}

}  // namespace swm

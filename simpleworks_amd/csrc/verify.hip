// verify.hip — batch verification of Marlin proofs against one verifying key (swm_verify_proofs_batch).
//
// The single verifier (host/ahp.h: verify) spends most of its ~6.5 ms on work that a batch shares or that a GPU does in bulk:
// the checked parse of the proof's 13 points (a square root and [r]P == O each), the host MSMs and two pairings.  Here:
//   1. the host reads the byte layout of every proof (counts, bools, Fr elements, trailing bytes) and packs the point
//      encodings into one upload;
//   2. verify_points_kernel checks and decodes every point of the batch, one lane per point, with a status word per point
//      (the caller learns WHICH proof is malformed);
//   3. the per-proof scalar plans (verify_plan: transcript, linear combinations, batch_check coefficients) run on the
//      context's host pool, one task per proof;
//   4. proof p's two openings are weighted by its own two 128-bit randomizers r[p][0], r[p][1], and the batch is summed into
//          TW = sum_p (r[p][0] w_p0 + r[p][1] w_p1),   TC = sum_p (r[p][0] C_p0 + r[p][1] C_p1),
//      one MSM each (K1: TC over the 13 points of every proof plus the verifying key's <= 16 shared bases, whose scalars are
//      summed across the batch; TW over the 2 witnesses of every proof), and one two-pairing product
//      e(-TW, beta_h) e(TC, h) == 1 decides the batch.
// Soundness: write proof p's opening i check as the GT exponent d_pi (zero iff the KZG opening equation holds).  The batch
// product is sum_{p,i} r[p][i] d_pi; if some d_pi != 0 it vanishes for at most one value of that r[p][i] given all others, so a
// batch holding an invalid proof passes with probability at most 2^-128 (128-bit randomizers, drawn independently of the
// proofs).  Every randomizer is random — the single verifier's first one is 1, which would let two invalid proofs cancel.
#include <string.h>
#include <algorithm>
#include <chrono>
#include <memory>
#include "devops.cuh"
#include "g1.cuh"
#include "host/ahp.h"
#include "host/host_handles.h"
#include "msm.h"
using namespace swm;

namespace {

// per-point status of verify_points_kernel (0 = a valid point in the prime-order subgroup, or the identity)
// (the bits of g1.cuh's decoders; fq_std_lt_p and the [r]P ladder, g1_in_subgroup_dev, are shared with the key codec's kernels)
enum : uint32_t { PT_OK = 0, PT_ENCODING = G1_BAD_ENCODING, PT_NOT_ON_CURVE = G1_OFF_CURVE, PT_NOT_IN_SUBGROUP = G1_OFF_SUBGROUP };

// ByteReader::g1 (host/marlin_types.h) for every point of a batch, one lane per point: flags, x (and y) < q, the square root and
// the choice of y (compressed: 12 words, x with the flags in the top bits of word 11) or the curve equation (uncompressed: 24
// words, x then y with the flags in the top bits of word 23), then [r]P == O.  out[i] = the affine point (Montgomery), or the
// identity when status[i] != PT_OK.  A plain store per lane: no atomics, no shared state.
// ~13 lanes per proof make a small grid: 64-lane workgroups spread a batch over as many CUs as it has waves.  Per lane the
// work is one Tonelli-Shanks root (compressed) and 252 doublings + the additions of r's set bits; expected latency, an
// estimate until measured: ~1-2 ms per launch whatever the batch size up to a few thousand proofs.
__global__ void __launch_bounds__(64) verify_points_kernel(const uint32_t* __restrict__ in, size_t n, int uncompressed,
                                                           G1Affine* __restrict__ out, uint32_t* __restrict__ status) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* src = in + (uncompressed ? 24 : 12) * i;
    Fq xs, ys;
    for (int k = 0; k < 12; k++) xs.v[k] = src[k];
    uint32_t flags;
    if (uncompressed) {
        for (int k = 0; k < 12; k++) ys.v[k] = src[12 + k];
        flags = ys.v[11] >> 30;
        ys.v[11] &= 0x3fffffffu;
    } else {
        flags = xs.v[11] >> 30;
        xs.v[11] &= 0x3fffffffu;
    }
    G1Affine r = g1_affine_identity();
    uint32_t st = PT_OK;
    if (flags == 3 || !fq_std_lt_p(xs) || (uncompressed && !fq_std_lt_p(ys))) {
        st = PT_ENCODING;
    } else if (!(flags & 1)) {  // (flags & 1: the infinity flag; x, y were range-checked and are otherwise ignored)
        r.x = fp_from_std(xs);
        const Fq rhs = fp_add(fp_mul(fp_sqr(r.x), r.x), fp_one<Fq>());
        if (uncompressed) {
            r.y = fp_from_std(ys);
            if (!fp_eq(fp_sqr(r.y), rhs)) st = PT_NOT_ON_CURVE;
        } else {
            Fq y;
            if (!fq_sqrt_dev(rhs, &y)) {
                st = PT_NOT_ON_CURVE;
            } else {
                Fq ny = fp_neg(y);
                bool y_is_larger = fp_cmp_std(fp_to_std(y), fp_to_std(ny)) > 0;
                r.y = (y_is_larger == ((flags & 2) != 0)) ? y : ny;
            }
        }
        if (st == PT_OK && !g1_in_subgroup_dev(r)) st = PT_NOT_IN_SUBGROUP;  // [r]P == O
    }
    out[i] = st == PT_OK ? r : g1_affine_identity();
    status[i] = st;
}

#define VLAUNCH(ctx, name, kernel, grid, block, ...)                               \
    do {                                                                           \
        prof_begin(ctx, name);                                                     \
        hipLaunchKernelGGL(kernel, grid, block, 0, (ctx)->stream, __VA_ARGS__);    \
        prof_end(ctx);                                                             \
        hip_check(ctx, hipGetLastError(), name);                                   \
    } while (0)

// Below this many proofs (that reach the pairing inputs) the batch sums are formed on the host: each proof's own Straus MSM on
// a worker of the host pool (the same sums the per-proof verdicts need after a failed batch), added up.  From here on one
// K1 MSM per input is cheaper than the pool's ~15 workers each taking a ~1 ms Straus chain per proof.  (A choice, not a
// measurement; both paths are tested at the sizes they serve.)
constexpr size_t kHostBatchBelow = 8;

struct BatchProof {
    int status = 0;  // 0: parsed and planned; < 0: the code swm_verify_proof returns for these bytes
    bool planned = false;
    Proof proof;
    size_t first = 0, npts = 0;  // its points in the batch's flat point list
    VerifyPlan plan;
    Fr r[2];
    G1Affine tw, tc;  // its own pairing inputs (host path, or a failed batch)
};

// Proof p's part of the batch scalars: its points' scalars in sc[first ..), its shared-base scalars in shared[0 .. nvk).
void scale_plan(const BatchProof& bp, Fr* sc, Fr* shared) {
    for (int i = 0; i < 2; i++)
        for (auto& t : bp.plan.c[i]) {
            Fr& dst = t.base >= kPlanVkBase ? shared[t.base - kPlanVkBase] : sc[t.base];
            dst = fp_add(dst, fp_mul(bp.r[i], t.s));
        }
}

G1Affine msm_affine(swm_ctx* ctx, const G1Affine* d_bases, const Fr* h_scalars, size_t n) {
    DBuf<Fr> sc(ctx, n);
    DBuf<G1Affine> b28(ctx, n);
    DBuf<uint32_t> mask(ctx, (n + 31) / 32);
    mask.zero();
    hip_check(ctx, hipMemcpyAsync(sc.p, h_scalars, n * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream), "h2d");
    rc_check(ctx, msm_scale_bases_run(ctx, d_bases, n, b28.p, mask.p));
    G1XYZZ r;
    rc_check(ctx, msm_run(ctx, d_bases, b28.p, sc.p, n, /*mont=*/1, &r, MsmInfMask{mask.p, 0}));
    return g1_to_affine(r);
}

void verify_batch_impl(swm_ctx* ctx, const VerifyingKey& vk, const uint64_t* public_inputs, size_t n_inputs,
                       const uint8_t* const* proofs, const size_t* lens, size_t count, bool uncompressed, ChaChaRng& rng,
                       int* ok, int* results, G1Affine* tw_out, G1Affine* tc_out) {
    static const bool trace = sw(SW_TRACE) >= 1;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t0 = now();
    auto mark = [&](const char* what) {
        if (!trace) return;
        auto t = now();
        fprintf(stderr, "[swm trace] verify batch (%zu): %-22s %8.3f ms\n", count, what,
                std::chrono::duration<double, std::milli>(t - t0).count());
        t0 = t;
    };
    std::vector<BatchProof> bp(count);
    // randomizers first: 2 x count draws in proof order, whatever the outcome
    for (size_t p = 0; p < count; p++)
        for (int i = 0; i < 2; i++) {
            uint64_t v[2];
            rng.gen_u128(v);
            bp[p].r[i] = fr_from_u128(v);
        }
    // 1. byte layout; the point encodings of the proofs that parse, packed for one upload
    const size_t words = uncompressed ? 24 : 12;
    std::vector<uint32_t> enc;
    size_t npts = 0;
    for (size_t p = 0; p < count; p++) {
        std::vector<const uint8_t*> at;
        try {
            bp[p].proof = deserialize_proof(proofs[p], lens[p], uncompressed, &at);
        } catch (const MarlinError& e) {
            bp[p].status = e.code;
            continue;
        }
        bp[p].first = npts;
        bp[p].npts = at.size();
        npts += at.size();
        enc.resize(npts * words);
        for (size_t k = 0; k < at.size(); k++) memcpy(&enc[(bp[p].first + k) * words], at[k], words * 4);
    }
    mark("byte layout");
    // 2. every point of the batch on the device; room behind them for the verifying key's shared bases (TC's MSM)
    const uint32_t nvk = plan_vk_bases(vk);
    DBuf<G1Affine> d_pts(ctx, npts + nvk);
    std::vector<G1Affine> pts(npts);
    if (npts) {
        DBuf<uint32_t> d_enc(ctx, npts * words), d_st(ctx, npts);
        hip_check(ctx, hipMemcpyAsync(d_enc.p, enc.data(), npts * words * 4, hipMemcpyHostToDevice, ctx->stream), "h2d");
        VLAUNCH(ctx, "verify_points", verify_points_kernel, dim3((unsigned)((npts + 63) / 64)), dim3(64), d_enc.p, npts,
                uncompressed ? 1 : 0, d_pts.p, d_st.p);
        std::vector<uint32_t> st = d_st.download(0, npts);
        hip_check(ctx, hipMemcpyAsync(pts.data(), d_pts.p, npts * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->stream), "d2h");
        hip_check(ctx, hipStreamSynchronize(ctx->stream), "sync");
        for (size_t p = 0; p < count; p++) {
            if (bp[p].status) continue;
            for (size_t k = 0; k < bp[p].npts; k++)
                if (st[bp[p].first + k] != PT_OK) bp[p].status = SWM_ERR_SERIALIZATION;
            if (bp[p].status) continue;
            std::vector<G1Affine*> slots = proof_points(bp[p].proof);
            for (size_t k = 0; k < slots.size(); k++) *slots[k] = pts[bp[p].first + k];
        }
    }
    mark("point check kernel");
    // 3. the per-proof plans on the host pool
    HostPool* pool = host_pool_of(ctx);
    pool->parallel_for((int)count, [&](int p) {
        BatchProof& b = bp[p];
        if (b.status) return;
        try {
            std::vector<Fr> pi(n_inputs);
            for (size_t k = 0; k < n_inputs; k++)
                pi[k] = fp_from_limbs<Fr>((const uint32_t*)(public_inputs + 4 * (n_inputs * p + k)));
            b.planned = verify_plan(vk, std::move(pi), b.proof, b.plan);
        } catch (const MarlinError& e) {
            b.status = e.code;
        } catch (const std::bad_alloc&) {
            b.status = SWM_ERR_OOM;
        } catch (const std::exception&) {
            b.status = SWM_ERR_INTERNAL;
        }
    });
    std::vector<size_t> live;
    bool all = true;
    for (size_t p = 0; p < count; p++) {
        if (bp[p].planned && !bp[p].status) live.push_back(p);
        else all = false;
        if (results) results[p] = bp[p].status ? bp[p].status : 0;
    }
    mark("plans");
    // 4. the batch sums and one pairing product
    G1Affine tw = g1_affine_identity(), tc = g1_affine_identity();
    auto own_inputs = [&](int t) {
        BatchProof& b = bp[live[t]];
        std::vector<const G1Affine*> pp = proof_points(static_cast<const Proof&>(b.proof));
        plan_pairing_inputs(vk, pp.data(), b.plan, b.r, &b.tw, &b.tc);
    };
    const bool host_sums = live.size() < kHostBatchBelow;
    const bool need_sums = !live.empty() && (all || results || tw_out || tc_out);
    if (need_sums && host_sums) {
        pool->parallel_for((int)live.size(), own_inputs);
        G1XYZZ sw = g1_xyzz_identity(), sc = g1_xyzz_identity();
        for (size_t p : live) {
            g1_add_mixed(sw, bp[p].tw);
            g1_add_mixed(sc, bp[p].tc);
        }
        tw = g1_to_affine(sw);
        tc = g1_to_affine(sc);
    } else if (need_sums) {
        // TC: every point of the batch (zero scalars for the proofs that are out) + the shared bases; TW: the live witnesses
        const size_t n = npts + nvk, L = live.size();
        std::vector<Fr> sc(n, fp_zero<Fr>()), shared((size_t)L * nvk, fp_zero<Fr>());
        pool->parallel_for((int)L, [&](int t) {
            const BatchProof& b = bp[live[t]];
            scale_plan(b, &sc[b.first], &shared[(size_t)t * nvk]);
        });
        for (size_t t = 0; t < L; t++)
            for (uint32_t j = 0; j < nvk; j++) sc[npts + j] = fp_add(sc[npts + j], shared[t * nvk + j]);
        std::vector<G1Affine> vkb(nvk), wb(2 * L);
        std::vector<Fr> ws(2 * L);
        for (uint32_t j = 0; j < nvk; j++) vkb[j] = plan_vk_base(vk, j);
        for (size_t t = 0; t < L; t++)
            for (int i = 0; i < 2; i++) {
                const BatchProof& b = bp[live[t]];
                wb[2 * t + i] = pts[b.first + b.plan.w[i]];
                ws[2 * t + i] = b.r[i];
            }
        hip_check(ctx, hipMemcpyAsync(d_pts.p + npts, vkb.data(), nvk * sizeof(G1Affine), hipMemcpyHostToDevice, ctx->stream), "h2d");
        DBuf<G1Affine> d_w(ctx, 2 * L);
        hip_check(ctx, hipMemcpyAsync(d_w.p, wb.data(), 2 * L * sizeof(G1Affine), hipMemcpyHostToDevice, ctx->stream), "h2d");
        mark("msm inputs");
        tc = msm_affine(ctx, d_pts.p, sc.data(), n);
        tw = msm_affine(ctx, d_w.p, ws.data(), 2 * L);
    }
    mark("msms");
    bool pass = !live.empty() && pairing_check(vk, tw, tc);
    mark("pairing");
    if (tw_out) *tw_out = tw;
    if (tc_out) *tc_out = tc;
    if (results) {
        if (pass) {
            for (size_t p : live) results[p] = 1;
        } else if (!live.empty()) {  // each proof on its own, with its own two randomizers
            pool->parallel_for((int)live.size(), [&](int t) {
                BatchProof& b = bp[live[t]];
                if (!host_sums) own_inputs(t);
                results[live[t]] = pairing_check(vk, b.tw, b.tc) ? 1 : 0;
            });
            mark("per-proof checks");
        }
    }
    *ok = all && pass ? 1 : 0;
}

void verify_batch_entry(swm_ctx* ctx, const VerifyingKey& vk, const uint64_t* public_inputs, size_t n_inputs,
                        const uint8_t* const* proofs, const size_t* lens, size_t count, bool uncompressed, ChaChaRng& rng, int* ok,
                        int* results, uint64_t* tw_xy, uint64_t* tc_xy) {
    G1Affine tw, tc;
    const bool want = tw_xy || tc_xy;
    verify_batch_impl(ctx, vk, public_inputs, n_inputs, proofs, lens, count, uncompressed, rng, ok, results, want ? &tw : nullptr,
                      want ? &tc : nullptr);
    if (tw_xy) memcpy(tw_xy, &tw, sizeof(G1Affine));
    if (tc_xy) memcpy(tc_xy, &tc, sizeof(G1Affine));
}

}  // namespace

extern "C" {

int swm_selftest_verify_batch(swm_ctx* ctx, const swm_vk* vk, const uint64_t* public_inputs, size_t n_inputs,
                              const uint8_t* const* proofs, const size_t* lens, size_t count, unsigned flags, swm_rng* rng,
                              int* ok, int* results, uint64_t tw_xy[12], uint64_t tc_xy[12]) {
    if (!ctx || !vk || !rng || !ok || (flags & ~(unsigned)SWM_PROOF_UNCOMPRESSED)) return SWM_ERR_INVALID_ARG;
    if (count && (!proofs || !lens || (n_inputs && !public_inputs))) return SWM_ERR_INVALID_ARG;
    for (size_t p = 0; p < count; p++)
        if (!proofs[p]) return SWM_ERR_INVALID_ARG;
    if (tw_xy) memset(tw_xy, 0, 12 * sizeof(uint64_t));
    if (tc_xy) memset(tc_xy, 0, 12 * sizeof(uint64_t));
    if (count == 0) {  // nothing launched, nothing drawn
        *ok = 1;
        return SWM_OK;
    }
    SWM_ON_DEVICE(ctx);
    SWM_GUARD(ctx, verify_batch_entry(ctx, vk->vk, public_inputs, n_inputs, proofs, lens, count,
                                      (flags & SWM_PROOF_UNCOMPRESSED) != 0, rng->r, ok, results, tw_xy, tc_xy));
}

int swm_verify_proofs_batch(swm_ctx* ctx, const swm_vk* vk, const uint64_t* public_inputs, size_t n_inputs,
                            const uint8_t* const* proofs, const size_t* lens, size_t count, unsigned flags, swm_rng* rng,
                            int* ok, int* results) {
    return swm_selftest_verify_batch(ctx, vk, public_inputs, n_inputs, proofs, lens, count, flags, rng, ok, results, nullptr,
                                     nullptr);
}

}  // extern "C"

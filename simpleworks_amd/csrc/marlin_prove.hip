// marlin_prove.hip — the Marlin prover (ark-marlin 0.3.0's AHP rounds, MarlinKZG10 commitments and openings) with every polynomial
// resident in HBM between the NTTs (K2), the mat-vecs (K3), the support kernels (K4, devops.cuh) and the commitments (K1, through
// marlin_commit.hip); the host drives the schedule, owns the Fiat-Shamir transcript and touches only O(1)-sized data per round.
//
// Deviations from arkworks' *schedule* that leave every proof byte unchanged (polynomials are canonical objects):
//   * round 2 multiplies in evaluation form on the 4|H| domain directly (5 FFT + 1 iFFT instead of 8 + 2);
//   * round 3 forms (a - b f) in evaluation form on the 4|K| domain (1 FFT + 1 iFFT instead of 3 iFFT + 2 FFT + 1 iFFT).
#include <chrono>
#include <functional>
#include <type_traits>
#include "marlin_units.h"

namespace {

// ================================================================================================ host helpers
Fr fr_one() { return fp_one<Fr>(); }

// host polynomial helpers for the degree-<=2 blinding polynomials
void hp_add_scaled(HPoly& acc, const HPoly& p, const Fr& k) {
    if (acc.size() < p.size()) acc.resize(p.size(), fp_zero<Fr>());
    for (size_t i = 0; i < p.size(); i++) acc[i] = fp_add(acc[i], fp_mul(p[i], k));
}
bool hp_is_zero(const HPoly& p) {
    for (auto& c : p)
        if (!fp_is_zero(c)) return false;
    return true;
}
HPoly hp_div_linear(const HPoly& p, const Fr& z) {
    HPoly t = p;
    while (!t.empty() && fp_is_zero(t.back())) t.pop_back();
    if (t.size() <= 1) return {};
    HPoly q(t.size() - 1);
    Fr carry = fp_zero<Fr>();
    for (size_t i = t.size() - 1; i >= 1; i--) {
        carry = fp_add(t[i], fp_mul(carry, z));
        q[i - 1] = carry;
    }
    return q;
}

// ================================================================================================ prover
// labelled device polynomial as the opening phase sees it
struct LPoly {
    const Fr* p = nullptr;
    size_t n = 0;
    bool has_bound = false;
    uint64_t bound = 0;
    bool hiding = false;
    PolyRand rand;
};

// SWM_TRACE=1: wall-clock per prover phase on stderr (synchronises at phase ends; diagnostic only)
struct PhaseTrace {
    swm_ctx* ctx;
    bool on;
    std::chrono::steady_clock::time_point t0;
    bool host_only;  // SWM_TRACE=2: host timestamps only (no synchronisation: the schedule is left undisturbed)
    std::chrono::steady_clock::time_point start;
    explicit PhaseTrace(swm_ctx* c)
        : ctx(c), on(sw(SW_TRACE) >= 1), t0(std::chrono::steady_clock::now()), host_only(sw(SW_TRACE) == 2), start(t0) {}
    void tick(const char* what) {
        if (!host_only) return;
        fprintf(stderr, "[swm host] %-34s at %8.3f ms\n", what,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - start).count());
    }
    void mark(const char* what) {
        if (!on) return;
        if (host_only) {
            tick(what);
            return;
        }
        (void)hipStreamSynchronize(ctx->stream);
        auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[swm trace] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

// Host -> device copy of the caller's (pageable) instance / witness buffers.  hipMemcpyAsync from pageable memory locks the
// pages first: ~0.3 ms before anything moves, whatever the size — a tenth of a 2^12-constraint proof (r04 trace: the first
// kernel that needs z started 0.37 ms into the proof).  Up to H2D_STAGE_BYTES per proof go through a pinned staging area of
// the context instead (a host memcpy of a few hundred KB, then a truly asynchronous copy); larger buffers keep the direct
// path, where the one-off lock is small against the transfer and a host-side copy of tens of MB would not be.
static constexpr size_t H2D_STAGE_BYTES = 1u << 20;
void upload_small(swm_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return;
    if (bytes <= H2D_STAGE_BYTES - ctx->h2d_stage_used) {
        if (!ctx->h2d_stage) hip_check(ctx, hipHostMalloc(&ctx->h2d_stage, H2D_STAGE_BYTES, hipHostMallocDefault), "pinned staging");
        char* at = (char*)ctx->h2d_stage + ctx->h2d_stage_used;
        memcpy(at, src, bytes);
        ctx->h2d_stage_used += (bytes + 255) & ~(size_t)255;
        hip_check(ctx, hipMemcpyAsync(dst, at, bytes, hipMemcpyHostToDevice, ctx->stream), "h2d");
        return;
    }
    hip_check(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream), "h2d");
}
// padded shape (pad_input_for_indexer_and_prover + make_matrices_square); the witness itself is uploaded straight
// from the caller's buffer, padding is filled on the device
struct ProveShape {
    std::vector<Fr> inst;  // padded to a power of two
    size_t nwit_orig = 0, nwit = 0, ncons = 0;
};
ProveShape prove_shape(const swm_r1cs* cs, const swm_pk& pk) {
    if (!cs || cs->num_instance == 0 || !cs->instance || (cs->num_witness && !cs->witness))
        throw MarlinError(SWM_ERR_INVALID_ARG, "r1cs: bad arguments");
    ProveShape s;
    for (size_t i = 0; i < cs->num_instance; i++) s.inst.push_back(fp_from_limbs<Fr>((const uint32_t*)(cs->instance + 4 * i)));
    if (!fp_is_one(s.inst[0])) throw MarlinError(SWM_ERR_INVALID_ARG, "r1cs: instance[0] must be one");
    s.inst.resize(HDomain(s.inst.size()).size, fp_zero<Fr>());
    s.nwit_orig = cs->num_witness;
    const size_t nv = s.inst.size() + cs->num_witness, nc = cs->num_constraints;
    s.nwit = nv > nc ? cs->num_witness : cs->num_witness + (nc - nv);
    s.ncons = nv > nc ? nv : nc;
    if (s.ncons != pk.info.num_constraints || s.inst.size() + s.nwit != pk.info.num_variables ||
        s.inst.size() != pk.info.num_instance_variables)
        throw MarlinError(SWM_ERR_MISMATCH, "InstanceDoesNotMatchIndex");
    return s;
}
// One proof over G ranks: which rounds run on a rank's share.  A domain of 2^log points can be split when G is a power of two
// up to 16 and every rank's share holds at least 16 BLOCKS of G points (ntt_sharded_run).
bool shard_fits(unsigned SG, unsigned slog_g, unsigned log) { return SG > 1 && (1u << slog_g) == SG && SG <= 16 && log >= 2 * slog_g + 4; }
struct ShardPlan {
    unsigned SG = 0, slog_g = 0;  // ranks, log2 of that
    bool r1 = false, r2 = false, r3 = false;
    size_t sm = 0;          // coefficients (evaluations) of H per rank
    size_t Mloc = 0, Mblk = 0;  // the rank's points of the 4|H| domain and its BLOCKS size (r2), or the whole domain
    size_t rank = 0;
};
ShardPlan shard_plan(swm_ctx* ctx, const swm_pk& pk) {
    ShardPlan sp;
    sp.SG = ctx->shard_world;
    sp.rank = ctx->shard_rank;
    while ((1u << sp.slog_g) < sp.SG) sp.slog_g++;
    const size_t M = 4 * pk.H;
    sp.r1 = shard_fits(sp.SG, sp.slog_g, pk.logH) && !sw(SW_SHARD_R1_OFF) && commit_cyclic_possible(ctx, pk, pk.H / sp.SG);
    sp.r2 = shard_fits(sp.SG, sp.slog_g, pk.logH + 2) && !sw(SW_SHARD_R2_OFF);
    sp.r3 = sp.r2 && shard_fits(sp.SG, sp.slog_g, pk.logB) && pk.K % sp.SG == 0;
    sp.sm = pk.H / (sp.SG ? sp.SG : 1);
    sp.Mloc = sp.r2 ? M / sp.SG : M;
    sp.Mblk = sp.r2 ? sp.Mloc / sp.SG : M;
    return sp;
}
// The rank's share of coeffs[0 .. n) zero-extended to 2^log coefficients, in evaluation form: the CYCLIC share (coefficient
// rank + G j at j) goes through the sharded forward transform, which leaves the rank's BLOCKS of evaluations.
DVec shard_evals(swm_ctx* ctx, const ShardPlan& sp, const Fr* coeffs, size_t n, unsigned log) {
    const size_t len = ((size_t)1 << log) / sp.SG;
    DVec loc(ctx, len);
    Fr* out = loc.p;
    const size_t s_rank = sp.rank, s_world = sp.SG;
    ew(ctx, "shard_take_cyclic", len, [=] __device__(size_t j) {
        const size_t i = s_rank + s_world * j;
        out[j] = i < n ? coeffs[i] : fp_zero<Fr>();
    });
    rc_check(ctx, ntt_sharded_run(ctx, loc.p, log, 0, 0));
    return loc;
}
// dst[0 .. n) from the ranks' CYCLIC shares of `per` elements each: element i is element i / G of rank i mod G
void shard_gather_cyclic(swm_ctx* ctx, const Fr* loc, size_t per, unsigned lg, Fr* dst, size_t n) {
    DVec all(ctx, per << lg);
    rc_check(ctx, shard_allgather_dev(ctx, loc, per * sizeof(Fr), all.p));
    const Fr* src = all.p;
    ew(ctx, "shard_interleave", n, [=] __device__(size_t i) { dst[i] = src[(i & (((size_t)1 << lg) - 1)) * per + (i >> lg)]; });
}
// poly += rho * (X^H - 1); poly has H + 1 slots of which the first H hold a polynomial of degree < H: slot H is written, not read
// (the buffers come from the pool without a fill: a transform overwrites the first H slots, this the last)
void add_rho_vh(swm_ctx* ctx, Fr* poly, uint64_t H, const Fr& rho) {
    ew(ctx, "add_rho_vh", 1, [=] __device__(size_t) {
        poly[0] = fp_sub(poly[0], rho);
        poly[H] = rho;
    });
}
// (h, X g) = divide_by_vanishing_poly(q, H) over q[0 .. total), part = |H|; or on a rank's CYCLIC share with part = |H| / G:
// coefficient j + k|H| of q sits on the same rank, |H| / G places further
void div_vh(swm_ctx* ctx, const Fr* q, size_t part, size_t total, Fr* h, Fr* g) {
    ew(ctx, "div_vh", 3 * part, [=] __device__(size_t j) {
        Fr acc = q[j + part];
        if (j + 2 * part < total) acc = fp_add(acc, q[j + 2 * part]);
        if (j + 3 * part < total) acc = fp_add(acc, q[j + 3 * part]);
        h[j] = acc;
        if (j < part) g[j] = fp_add(q[j], acc);
    });
}
// h = q / v_K over q[0 .. total), part = |K|; or on a rank's CYCLIC share with part = |K| / G (as div_vh)
void div_vk(swm_ctx* ctx, const Fr* q, size_t part, size_t total, Fr* h) {
    ew(ctx, "div_vk", 3 * part, [=] __device__(size_t j) {
        Fr acc = fp_zero<Fr>();
        for (uint64_t i = 1; j + i * part < total; i++) acc = fp_add(acc, q[j + i * part]);
        h[j] = acc;
    });
}
// Round 2 on three cosets of H (s_k H, s_k = w_4|H|^k, k = 0, 1, 2: the points i = k mod 4 of the 4|H| domain) instead of the whole
// 4|H| domain: q_1 - mask has degree 3|H| - 1 (deg r(alpha, X) = |H| - 1, deg z_A = deg z_B = |H| with zk bound 1; t z: 2|H| - 1), so
// three cosets determine it (tests/test_outer_cosets_degree.py checks the bound on the model).  Coset 0 is H itself, where every
// factor is known without a transform; cosets 1 and 2 come from ntt_cosets_fwd (two |H|-point transforms in one launch per pass
// instead of a 4|H|-point one) and the way back is ntt_cosets_inv plus cosets3_solve (devops.cuh).  -DSWM_OUTER_COSETS=0 builds the 4|H| path.
#ifndef SWM_OUTER_COSETS
#define SWM_OUTER_COSETS 1
#endif
static constexpr uint64_t OUTER_COSETS_MIN_H = 16;
// alpha^|H| - X^|H| on the 4|H| domain, where X^|H| = i4^(i mod 4), i4 = w4^|H| a primitive fourth root of unity
struct RAlphaNumerators {
    Fr n0, n1, n2, n3;
    __device__ __forceinline__ Fr at(size_t i) const {
        const unsigned q = (unsigned)(i & 3);
        return q == 0 ? n0 : q == 1 ? n1 : q == 2 ? n2 : n3;
    }
};
RAlphaNumerators r_alpha_numerators(const Fr& alpha, unsigned logH, uint64_t M) {
    Fr aH = alpha;
    for (unsigned i = 0; i < logH; i++) aH = fp_sqr(aH);
    Fr i4 = HDomain(M).gen;
    for (unsigned i = 0; i < logH; i++) i4 = fp_sqr(i4);
    return {fp_sub(aH, fp_one<Fr>()), fp_sub(aH, i4), fp_sub(aH, fp_sqr(i4)), fp_sub(aH, fp_mul(fp_sqr(i4), i4))};
}
// Which point i of a product domain (4|H| in round 2, 4|K| in round 3; D = H or K) position p of a buffer of evaluations holds:
//   dense:  point p;
//   blocks: a rank's share of a sharded proof (the BLOCKS layout of ntt.hip), `loc` points in blocks of `blk`;
//   cosets: point 4 j + k at k |D| + j (coset k of D in one piece).
struct DenseMap {
    __host__ __device__ size_t index(size_t p) const { return p; }
};
struct BlocksMap {
    size_t loc, blk, rank;
    __host__ __device__ size_t index(size_t p) const { return loc * (p / blk) + rank * blk + (p % blk); }
};
struct CosetsMap {
    unsigned logD;
    __host__ __device__ size_t index(size_t p) const { return ((p & (((size_t)1 << logD) - 1)) << 2) + (p >> logD); }
    __host__ __device__ size_t position(size_t i) const { return ((i & 3) << logD) + (i >> 2); }
};
// f(map) for the layout of a round: `sharded` (a share of `loc` points), else `cosets` of a domain of 2^logD points, else dense.
// f is instantiated once per layout, and so is every pointwise kernel in it: none of them branches on the layout.
template <class F>
void with_product_map(const ShardPlan& sp, bool sharded, size_t loc, bool cosets, unsigned logD, F&& f) {
    if (sharded) f(BlocksMap{loc, loc / sp.SG, sp.rank});
    else if (cosets) f(CosetsMap{logD});
    else f(DenseMap{});
}
// round 2's outer-sumcheck form at one point: q_1 - mask = r(alpha, .) (eta_c z_A z_B + eta_a z_A + eta_b z_B) - z t
__device__ __forceinline__ Fr round2_outer_form(const Fr& eta_a, const Fr& eta_b, const Fr& eta_c, const Fr& ra, const Fr& a,
                                                const Fr& b, const Fr& z, const Fr& t) {
    const Fr summed = fp_add(fp_add(fp_mul(eta_c, fp_mul(a, b)), fp_mul(eta_a, a)), fp_mul(eta_b, b));
    return fp_sub(fp_mul(ra, summed), fp_mul(z, t));
}
// round 3's a - b f at point i of the 4|K| domain, from the index's twelve evaluations there
struct IndexOnB {
    const Fr *ar, *ac, *arc, *av;  // row, col, row_col, val of A
    const Fr *br, *bc, *brc, *bv;
    const Fr *cr, *cc, *crc, *cv;
};
struct Round3Challenges {
    Fr alpha, beta, ab, ve_a, ve_b, ve_c;  // ab = beta alpha, ve_M = v_H(alpha) v_H(beta) eta_M
};
// With u_M = ve_M val_M:  a = u_a (d_b d_c) + d_a (u_b d_c + u_c d_b),  b = d_a (d_b d_c):  6 products for the denominators, 3 for
// the u, 5 for a, 2 for b f and b: 16 (the form that multiplies every term out takes 18; same field element, so the same bytes).
__device__ __forceinline__ Fr round3_a_minus_bf(const IndexOnB& x, const Round3Challenges& c, size_t i, const Fr& f) {
    Fr da = fp_add(fp_sub(fp_sub(c.ab, fp_mul(x.ar[i], c.alpha)), fp_mul(c.beta, x.ac[i])), x.arc[i]);
    Fr db = fp_add(fp_sub(fp_sub(c.ab, fp_mul(x.br[i], c.alpha)), fp_mul(c.beta, x.bc[i])), x.brc[i]);
    Fr dc = fp_add(fp_sub(fp_sub(c.ab, fp_mul(x.cr[i], c.alpha)), fp_mul(c.beta, x.cc[i])), x.crc[i]);
    Fr dbc = fp_mul(db, dc);
    Fr ua = fp_mul(c.ve_a, x.av[i]), ub = fp_mul(c.ve_b, x.bv[i]), uc = fp_mul(c.ve_c, x.cv[i]);
    Fr a_val = fp_add(fp_mul(ua, dbc), fp_mul(da, fp_add(fp_mul(ub, dc), fp_mul(uc, db))));
    Fr b_val = fp_mul(da, dbc);
    return fp_sub(a_val, fp_mul(b_val, f));
}
// What the stages of one proof share.  The device buffers are declared in the order the stages allocate them, so that they
// return to the context's pool in the same order as when they were the locals of one function.
struct ProveState {
    ChaChaRng& zk;
    PhaseTrace& tr;
    const ProveShape shape;
    const ShardPlan sp;
    const uint64_t H, K, X, Bsz, M;  // M: mul_domain = next_pow2(3|H| + 1)
    const unsigned logM;
    const size_t nvars, ninst;
    const size_t mask_len;  // degree 3|H| + 2 zk_bound - 3
    const HDomain dh;
    const std::vector<Fr> public_input;
    FiatShamirRng fs;
    VerifierState st;
    Fr rho_w, rho_a, rho_b;
    int lane = 0;
    LPoly P_w, P_za, P_zb, P_mask, P_t, P_g1, P_h1, P_g2, P_h2;
    LPoly idx_polys[12];
    std::map<std::string, LPoly*> polys;
    CommitJob j1[4], j2[3], j3[2];
    std::vector<Commitment> comms1 = std::vector<Commitment>(4), comms2 = std::vector<Commitment>(3),
                            comms3 = std::vector<Commitment>(2);
    bool mask_late = false;  // the mask is drawn from a caller-owned generator after the rest of round 1 is enqueued
    unsigned mask_pieces = 1;
    AsyncMsm mask_part[2];
    bool ra_closed_form = false;
    bool cosets = false;  // round 2 on the cosets 0, 1, 2 of H (SWM_OUTER_COSETS): e_za, e_zb, e_z hold cosets 1 | 2
    LcSet lcs;
    DVec mask, z, za_evals, zb_evals, za_loc, zb_loc, x_poly, w_poly, za_poly, zb_poly, e_za, e_zb, e_z;
    DVec r_alpha_evals, e_ra, t_poly, q1, h1, g1x, f, h2;

    ProveState(const swm_pk& pk, ChaChaRng& rng, PhaseTrace& t, ProveShape shp, const ShardPlan& plan)
        : zk(rng), tr(t), shape(std::move(shp)), sp(plan), H(pk.H), K(pk.K), X(pk.X), Bsz(pk.B), M(4 * pk.H),
          logM(pk.logH + 2), nvars(pk.info.num_variables), ninst(shape.inst.size()), mask_len(3 * pk.H), dh(pk.H),
          public_input(shape.inst.begin() + 1, shape.inst.end()) {
        fs_init(fs, pk.vk, public_input);
        for (int m = 0; m < 3; m++) {
            const DVec* v[4] = {&pk.ar[m].row, &pk.ar[m].col, &pk.ar[m].val, &pk.ar[m].row_col};
            for (int j = 0; j < 4; j++) {
                idx_polys[4 * m + j].p = v[j]->p;
                idx_polys[4 * m + j].n = K;
                polys[kIndexerPolys[4 * m + j]] = &idx_polys[4 * m + j];
            }
        }
        polys["w"] = &P_w; polys["z_a"] = &P_za; polys["z_b"] = &P_zb; polys["mask_poly"] = &P_mask;
        polys["t"] = &P_t; polys["g_1"] = &P_g1; polys["h_1"] = &P_h1; polys["g_2"] = &P_g2; polys["h_2"] = &P_h2;
    }
};

// ---- round 1: the mask polynomial, 3|H| uniform coefficients drawn from the caller's rng with the H-sum forced to zero,
// and its commitment
void draw_mask(swm_ctx* ctx, const swm_pk& pk, ProveState& s) {
    const uint64_t H = s.H;
    Fr* mp = s.mask.p;
    if (s.mask_pieces > 1) {
        // ONE draw of 3|H| coefficients; whenever the host learns how many are in place (sample_fr_bulk: `progress`) the pieces
        // that are complete are committed: [1, H) | [H, 2H) | [2H, 3H) (three pieces; two: [1, H) | [H, 3H)).  One draw, not
        // three: every draw ends with a geometric tail of ever shorter runs (a run may not reach beyond the candidate that
        // completes the draw), ~1.5 ms each.
        CommitJob& job = s.j1[3];
        job.has_bound = false;
        job.hiding = false;
        unsigned done_pieces = 0;
        struct PieceEvent {  // destroyed on every way out (commit_enqueue may throw from inside the draw's progress callback)
            hipEvent_t e = nullptr;
            ~PieceEvent() {
                if (e) (void)hipEventDestroy(e);
            }
        } piece_guard;
        hip_check(ctx, hipEventCreateWithFlags(&piece_guard.e, hipEventDisableTiming), "event");
        const hipEvent_t piece_ev = piece_guard.e;
        auto enqueue_piece = [&](unsigned pc) {  // the elements of the piece are written by kernels already on the copy stream
            hip_check(ctx, hipEventRecord(piece_ev, ctx->copy_stream), "record");
            hip_check(ctx, hipStreamWaitEvent(ctx->stream, piece_ev, 0), "wait");
            if (pc == 0) commit_enqueue(ctx, &s.lane, pk, 1, mp + 1, H - 1, &job.plain);
            else if (s.mask_pieces == 3) commit_enqueue(ctx, &s.lane, pk, pc * H, mp + pc * H, H, &s.mask_part[pc - 1]);
            else if (pc == 2) commit_enqueue(ctx, &s.lane, pk, H, mp + H, 2 * H, &s.mask_part[0]);
        };
        const std::function<void(size_t)> progress = [&](size_t have) {
            while (done_pieces < 2 && have >= (size_t)(done_pieces + 1) * H) enqueue_piece(done_pieces++);
        };
        sample_fr_bulk(ctx, s.zk, mp, s.mask_len, s.mask_late, &progress);
        while (done_pieces < 3) enqueue_piece(done_pieces++);  // (after the draw ctx->stream waits for all of it anyway)
    } else {
        sample_fr_bulk(ctx, s.zk, mp, s.mask_len, s.mask_late);
    }
    ew(ctx, "mask_fix", 1, [=] __device__(size_t) {
        // remainder mod v_H at coefficient 0 = c[0] + c[H] + c[2H]; subtracting it from c[0] leaves -(c[H] + c[2H])
        mp[0] = fp_neg(fp_add(mp[H], mp[2 * H]));
    });
    s.P_mask.p = mp;
    s.P_mask.n = s.mask_len;
    // (the mask's 3|H|-point commitment enqueued behind w's or behind z_B's instead of first: + 0.4 ... + 1.9 ms at 2^20, r05)
    if (s.mask_pieces == 1) pc_commit_begin(ctx, pk, &s.lane, s.P_mask.p, s.P_mask.n, false, 0, false, &s.j1[3]);
}
void begin_mask(swm_ctx* ctx, const swm_pk& pk, ProveState& s) {
    s.mask = DVec(ctx, s.mask_len);
    // A caller-owned generator (swm_rng_from_callback) produces the mask on the HOST, through its fill_bytes: ~170 MB at
    // |H| = 2^20, i.e. tens of milliseconds of the caller's ChaCha.  That draw is therefore requested AFTER the rest of
    // round 1 has been enqueued (witness upload, mat-vecs, the three other polynomials and their commitments, the
    // challenge-independent transforms of round 2), so that the GPU works while the host draws.  The draw ORDER is
    // untouched: nothing between here and there touches `zk` (rho_w, rho_a, rho_b were drawn before, the blinding
    // polynomials are drawn after the round's last commitment is enqueued, as before).
    s.mask_late = s.zk.ext != nullptr;
    // r05: with a caller-owned generator the commitment is computed IN PIECES — the MSM over the coefficients [1, |H|) is
    // enqueued as soon as the first |H| coefficients are there and runs while the host draws the next |H|, and so on; what is
    // exposed behind the draw is a third of the MSM instead of all of it.  Coefficient 0 is only known after the whole draw
    // (mask_fix): its term [c_0] g is one scalar multiplication on the host.  A commitment is a sum over coefficients, so
    // the pieces add up to the same group element: same bytes (test_callback_rng_reproduces_golden_bytes).  SWM_MASK_PIECES=1:
    // one piece (r02 - r04).  Sharded proofs keep one piece (their commitments are split over the ranks already).
    s.mask_pieces = s.mask_late && ctx->shard_world <= 1 && s.H >= 4096 ? (unsigned)sw(SW_MASK_PIECES) : 1u;
    if (s.mask_late) sample_fr_ext_mark(ctx);  // the transfers of the late draw only wait for what precedes the allocation
    else draw_mask(ctx, pk, s);
}

// ---- z on the device, z_A = A z, z_B = B z  (K3)
// One proof over G GPUs: z_A = A z and z_B = B z are computed BY ROWS — every rank the rows of its blocks
// (the BLOCKS layout of ntt.hip; z is the witness every rank was handed, so no broadcast is needed) — interpolated by the
// sharded inverse transform (one all-to-all each), which leaves the coefficients CYCLIC over the ranks, and committed
// where they are (commit_enqueue_cyclic): no gather between mat-vec, transform and MSM.  The rest of the proof still
// works on whole polynomials, so the pieces are all-gathered once afterwards (H x 32 B per polynomial over all links).
void upload_witness(swm_ctx* ctx, const swm_pk& pk, ProveState& s, const swm_r1cs* cs) {
    const ProveShape& shape = s.shape;
    s.z = DVec(ctx, s.nvars);
    // (the staging area is free again: whatever the previous proof of this context staged was consumed before that proof returned)
    ctx->h2d_stage_used = 0;
    upload_small(ctx, s.z.p, shape.inst.data(), s.ninst * sizeof(Fr));
    if (shape.nwit_orig && ctx->witness_dev)  // a witness synthesised on this device (merkle_witness.hip): no host round trip
        hip_check(ctx, hipMemcpyAsync(s.z.p + s.ninst, ctx->witness_dev, shape.nwit_orig * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream), "d2d");
    else if (shape.nwit_orig) upload_small(ctx, s.z.p + s.ninst, cs->witness, shape.nwit_orig * sizeof(Fr));
    if (shape.nwit > shape.nwit_orig) {  // dummy unconstrained variables have the value one
        Fr* zp = s.z.p + s.ninst + shape.nwit_orig;
        ew(ctx, "z_pad", shape.nwit - shape.nwit_orig, [=] __device__(size_t i) { zp[i] = fp_one<Fr>(); });
    }
    if (s.sp.r1) {
        const size_t sm = s.sp.sm;
        s.za_loc = dv_zeros(ctx, sm + 1);
        s.zb_loc = dv_zeros(ctx, sm + 1);
        const unsigned blk_log = pk.logH - 2 * s.sp.slog_g;
        const size_t row0 = s.sp.rank << blk_log;
        auto rows_of_my_blocks = [&](const DevCsr& mtx, Fr* out) {
            const uint32_t* rowptr = mtx.rowptr.p;
            const uint32_t* col = mtx.col.p;
            const Fr* val = mtx.val.p;
            const Fr* zz = s.z.p;
            const size_t nrows = mtx.rows;
            ctx->stat_spmv_calls++;
            ctx->stat_spmv_rows += sm;
            ew(ctx, "spmv_rows_blocks", sm, [=] __device__(size_t x) {
                const size_t r = ((x >> blk_log) * sm) + row0 + (x & (((size_t)1 << blk_log) - 1));  // row m k1 + rank blk + t
                Fr acc = fp_zero<Fr>();
                if (r < nrows)
                    for (uint32_t k = rowptr[r], e = rowptr[r + 1]; k < e; k++) {
                        Fr c = val[k];
                        Fr zv = zz[col[k]];
                        acc = fp_add(acc, fp_is_one(c) ? zv : fp_mul(zv, c));
                    }
                out[x] = acc;
            });
        };
        rows_of_my_blocks(pk.a, s.za_loc.p);
        rows_of_my_blocks(pk.b, s.zb_loc.p);
    } else {
        s.za_evals = dv_zeros(ctx, s.H);
        s.zb_evals = dv_zeros(ctx, s.H);
        rc_check(ctx, spmv_run(ctx, pk.a.rowptr.p, pk.a.col.p, pk.a.val.p, s.z.p, s.za_evals.p, pk.a.rows, &pk.a.plan));
        rc_check(ctx, spmv_run(ctx, pk.b.rowptr.p, pk.b.col.p, pk.b.val.p, s.z.p, s.zb_evals.p, pk.b.rows, &pk.b.plan));
    }
}

// sharded form of "interpolate, add rho v_H, commit" for z_A or z_B: the rank's evaluations `loc` become its CYCLIC
// coefficients, committed where they are; `poly` receives the whole polynomial
void sharded_interpolate_and_commit(swm_ctx* ctx, const swm_pk& pk, ProveState& s, DVec& loc, const Fr& rho, DVec& poly,
                                    CommitJob* job) {
    const uint64_t H = s.H;
    const size_t sm = s.sp.sm;
    rc_check(ctx, ntt_sharded_run(ctx, loc.p, pk.logH, 1, 1));  // evaluations in BLOCKS -> coefficients rank + G j at loc[j]
    shard_gather_cyclic(ctx, loc.p, sm, s.sp.slog_g, poly.p, H);  // the whole polynomial for the replicated rest of the proof
    add_rho_vh(ctx, poly.p, H, rho);
    if (ctx->shard_rank == 0) {  // coefficients 0 and H = 0 + G (H / G) both live on rank 0
        Fr* lp = loc.p;
        const size_t top = sm;
        ew(ctx, "add_rho_vh", 1, [=] __device__(size_t) {
            lp[0] = fp_sub(lp[0], rho);
            lp[top] = rho;
        });
    }
    job->has_bound = false;
    job->hiding = true;
    commit_enqueue_cyclic(ctx, &s.lane, pk, loc.p, ctx->shard_rank == 0 ? sm + 1 : sm, &job->plain);
}
// ---- round 1: w, z_A and z_B as polynomials, and their commitments
void round1_polys(swm_ctx* ctx, const swm_pk& pk, ProveState& s) {
    const uint64_t H = s.H, X = s.X;
    // x_poly = interpolate(formatted input over X)
    s.x_poly = DVec(ctx, X);
    s.x_poly.upload(s.shape.inst.data(), X);
    dv_ntt(ctx, s.x_poly, pk.logX, true);
    // w v_X = interp_H(z - x on H) = interp_H(z) - x: interpolation is linear and deg x < |X| <= |H|, so x is never evaluated on H.
    // The assignment on H: the instance (the head of z) on the X-subgroup positions, w_extended[k - k/ratio - 1] elsewhere; one
    // inverse transform; x_poly subtracted from the first |X| coefficients (tests/test_known_work_identities.py).
    const uint64_t ratio = H / X;
    const size_t nwit = s.shape.nwit, ninst = s.ninst;
    s.w_poly = DVec(ctx, H + 1);  // no fill: w_evals writes the first H slots, add_rho_vh slot H
    {
        Fr* out = s.w_poly.p;
        const Fr* zz = s.z.p;
        ew(ctx, "w_evals", H, [=] __device__(size_t k) {
            Fr v;
            if (k % ratio == 0) {
                v = zz[k / ratio];
            } else {
                size_t wi = k - k / ratio - 1;
                v = wi < nwit ? zz[ninst + wi] : fp_zero<Fr>();
            }
            out[k] = v;
        });
    }
    rc_check(ctx, ntt_run(ctx, s.w_poly.p, pk.logH, 1, 0));  // in place on the first H of its H + 1 slots
    {
        Fr* out = s.w_poly.p;
        const Fr* xp = s.x_poly.p;
        ew(ctx, "w_sub_x", X, [=] __device__(size_t i) { out[i] = fp_sub(out[i], xp[i]); });
    }
    add_rho_vh(ctx, s.w_poly.p, H, s.rho_w);
    // divide by v_X (exact): quotient = strided suffix sums, w_poly <- quotient (degree <= H - X)
    suffix_recurrence(ctx, s.w_poly.p, H + 1, X, fr_one());
    s.P_w.p = s.w_poly.p + X;  // quotient[j] = s[j + X]
    s.P_w.n = H + 1 - X;
    s.P_w.hiding = true;
    pc_commit_begin(ctx, pk, &s.lane, s.P_w.p, s.P_w.n, false, 0, true, &s.j1[0]);
    s.za_poly = DVec(ctx, H + 1);  // no fill: the inverse transform (or the gather of a sharded one) writes the first H slots,
    s.zb_poly = DVec(ctx, H + 1);  // add_rho_vh slot H
    s.P_za.p = s.za_poly.p; s.P_za.n = H + 1; s.P_za.hiding = true;
    s.P_zb.p = s.zb_poly.p; s.P_zb.n = H + 1; s.P_zb.hiding = true;
    if (s.sp.r1) {
        sharded_interpolate_and_commit(ctx, pk, s, s.za_loc, s.rho_a, s.za_poly, &s.j1[1]);
        sharded_interpolate_and_commit(ctx, pk, s, s.zb_loc, s.rho_b, s.zb_poly, &s.j1[2]);
    } else {
        rc_check(ctx, ntt_run_from(ctx, s.za_poly.p, pk.logH, 1, 0, s.za_evals.p, H));  // evaluations -> the first H of H + 1 slots
        add_rho_vh(ctx, s.za_poly.p, H, s.rho_a);
        rc_check(ctx, ntt_run_from(ctx, s.zb_poly.p, pk.logH, 1, 0, s.zb_evals.p, H));
        add_rho_vh(ctx, s.zb_poly.p, H, s.rho_b);
        // (enqueue order only: the results are awaited and blinded in label order; z_B's ahead of z_A's: + 0.9 ms at 2^20, r05)
        pc_commit_begin(ctx, pk, &s.lane, s.P_za.p, s.P_za.n, false, 0, true, &s.j1[1]);
        pc_commit_begin(ctx, pk, &s.lane, s.P_zb.p, s.P_zb.n, false, 0, true, &s.j1[2]);
    }
}

// Round 2 over G ranks (r03): the four transforms of size 4|H| into the product domain, the pointwise outer-sumcheck form and
// the transform back run on a rank's share — CYCLIC coefficients (every rank holds the polynomials: it takes g, g + G, ...)
// -> BLOCKS evaluations by ONE all-to-all each (ntt_sharded_run), pointwise on the blocks, BLOCKS -> CYCLIC back; the mask
// and the division by v_H are local in the CYCLIC layout (G divides |H|: index j + k|H| stays on its rank).  h_1 and X g_1 are
// all-gathered afterwards (4|H| x 32 B per proof): the openings work on whole polynomials.  SWM_SHARD_R2_OFF disables it.
// coeffs[0 .. n) in evaluation form in the proof's round-2 layout: the 4|H| domain, the rank's BLOCKS of it, or cosets 1 | 2 of H
// (coset 0 is H itself and needs no transform)
DVec on_round2_layout(swm_ctx* ctx, const ProveState& s, const Fr* coeffs, size_t n) {
    if (s.sp.r2) return shard_evals(ctx, s.sp, coeffs, n, s.logM);
    if (!s.cosets) return dv_ntt_from(ctx, coeffs, n, s.logM, false);
    static const unsigned ks[2] = {1, 2};
    DVec v(ctx, 2 * s.H);
    rc_check(ctx, ntt_cosets_fwd(ctx, coeffs, n, s.dh.log, ks, 2, v.p));
    return v;
}
// ---- the challenge-independent part of round 2, issued before the round-1 commitments are awaited so that it runs under
// them: z_A, z_B and z = w v_X + x in evaluation form in the round's layout
void round2_prework(swm_ctx* ctx, ProveState& s) {
    const uint64_t H = s.H, X = s.X;
    s.cosets = SWM_OUTER_COSETS && !s.sp.r1 && !s.sp.r2 && H >= OUTER_COSETS_MIN_H;  // single-GPU rounds (the sharded ones keep 4|H|)
    s.e_za = on_round2_layout(ctx, s, s.za_poly.p, H + 1);
    s.e_zb = on_round2_layout(ctx, s, s.zb_poly.p, H + 1);
    DVec z_poly(ctx, H + 1);  // (every slot is written below)
    Fr* out = z_poly.p;
    const Fr* wc = s.P_w.p;
    const size_t w_len = s.P_w.n;
    const Fr* xp = s.x_poly.p;
    ew(ctx, "z_poly", H + 1, [=] __device__(size_t i) {
        Fr v = fp_zero<Fr>();
        if (i >= X && i - X < w_len) v = wc[i - X];
        if (i < w_len) v = fp_sub(v, wc[i]);
        if (i < X) v = fp_add(v, xp[i]);
        out[i] = v;
    });
    s.e_z = on_round2_layout(ctx, s, z_poly.p, H + 1);
}

// ---- end of round 1: blinding, the rest of a mask committed in pieces, the commitments
void round1_commitments(swm_ctx* ctx, const swm_pk& pk, ProveState& s) {
    // blinding draws and hiding terms (label order: w, z_a, z_b, mask) while the MSMs run
    pc_commit_blind(pk, &s.j1[0], &s.zk, &s.P_w.rand);
    pc_commit_blind(pk, &s.j1[1], &s.zk, &s.P_za.rand);
    pc_commit_blind(pk, &s.j1[2], &s.zk, &s.P_zb.rand);
    pc_commit_blind(pk, &s.j1[3], nullptr, &s.P_mask.rand);
    if (s.mask_pieces > 1) {  // the other pieces of the mask commitment and the term of coefficient 0
        Fr c0 = s.mask.download(0, 1)[0];
        Fr c0s = fp_to_std(c0);
        G1XYZZ extra = g1_mul_limbs(pk.vk.vk.g, c0s.v, 8);
        for (unsigned k = 0; k + 1 < s.mask_pieces; k++) g1_add(extra, commit_wait(ctx, &s.mask_part[k]));
        s.j1[3].has_extra = true;
        s.j1[3].extra = extra;
    }
    commit_gather(ctx, {&s.j1[0].plain, &s.j1[1].plain, &s.j1[2].plain, &s.j1[3].plain});
    pc_commit_end_round(ctx, pk, {&s.j1[0], &s.j1[1], &s.j1[2], &s.j1[3]}, {&s.zk, &s.zk, &s.zk, nullptr},
                        {&s.P_w.rand, &s.P_za.rand, &s.P_zb.rand, &s.P_mask.rand}, s.comms1.data());
}

// r(alpha, X) = v_H(alpha) / (alpha - X) on H
void r_alpha_on_h(swm_ctx* ctx, const swm_pk& pk, ProveState& s) {
    const Fr alpha = s.st.alpha;
    PowTable wh = root_pow_table(ctx, pk.logH);
    Fr* rh = s.r_alpha_evals.p;
    ew(ctx, "r_alpha_den", s.H, [=] __device__(size_t i) { rh[i] = fp_sub(alpha, wh.at(i)); });
    rc_check(ctx, batch_inverse_run(ctx, rh, s.H));
    Fr vh = s.dh.vanishing(alpha);
    ew(ctx, "r_alpha_scale", s.H, [=] __device__(size_t i) { rh[i] = fp_mul(rh[i], vh); });
}
// ---- round 2: r(alpha, X) = (alpha^|H| - X^|H|) / (alpha - X) is needed on H (input of the transposed mat-vecs) and on the
// 4|H| domain (outer sumcheck).  On the 4|H| domain X^|H| takes four values (r_alpha_numerators), so both come from ONE batch
// inversion of alpha - w4^i over the points of the round's layout — instead of an inversion over H, an inverse transform of size
// |H| and a forward one into the layout (r03).  H is every fourth point of that domain.  (alpha on the 4|H| domain — probability
// 2^-231 — would make a denominator vanish: the transforms are kept for that case, round2_q1; SWM_RALPHA_TRANSFORMS=1 takes it.)
void r_alpha(swm_ctx* ctx, const swm_pk& pk, ProveState& s) {
    const Fr alpha = s.st.alpha;
    s.r_alpha_evals = DVec(ctx, s.H);
    {
        Fr a4h = alpha;
        for (unsigned i = 0; i < s.logM; i++) a4h = fp_sqr(a4h);
        s.ra_closed_form = !fp_is_one(a4h) && !sw(SW_RALPHA_TRANSFORMS);  // (test hook: the path of the 2^-231 case)
    }
    if (!s.ra_closed_form) return r_alpha_on_h(ctx, pk, s);
    // one inversion over the layout's points: the rank's BLOCKS, cosets 0 | 1 | 2 of H, or all of the 4|H| domain
    const size_t n = s.cosets ? 3 * s.H : s.sp.Mloc;
    s.e_ra = DVec(ctx, n);
    PowTable wt = root_pow_table(ctx, s.logM);
    Fr* out = s.e_ra.p;
    Fr* rh = s.r_alpha_evals.p;
    const RAlphaNumerators nu = r_alpha_numerators(alpha, pk.logH, s.M);
    with_product_map(s.sp, s.sp.r2, n, s.cosets, pk.logH, [&](auto map) {
        ew(ctx, "r_alpha_den", n, [=] __device__(size_t p) { out[p] = fp_sub(alpha, wt.at(map.index(p))); });
        rc_check(ctx, batch_inverse_run(ctx, out, n));
        ew(ctx, "r_alpha_scale", n, [=] __device__(size_t p) {
            const size_t i = map.index(p);
            const Fr v = fp_mul(out[p], nu.at(i));
            out[p] = v;
            if constexpr (!std::is_same_v<decltype(map), BlocksMap>)
                if ((i & 3) == 0) rh[i >> 2] = v;
        });
    });
    // (a rank's share holds a part of H only, and every rank needs all of it for the transposed mat-vecs: its own inversion)
    if (s.sp.r2) r_alpha_on_h(ctx, pk, s);
}

// ---- round 2: t evaluations on H, t[reindex(c)] = sum_M eta_M (M^T r_alpha)[c], interpolated, and its commitment
void round2_t(swm_ctx* ctx, const swm_pk& pk, ProveState& s) {
    const uint64_t H = s.H, X = s.X;
    const size_t nvars = s.nvars;
    const Fr eta_a = s.st.eta_a, eta_b = s.st.eta_b, eta_c = s.st.eta_c;
    s.t_poly = dv_zeros(ctx, H);
    {
        DVec ta(ctx, nvars), tb(ctx, nvars), tc(ctx, nvars);
        const Fr* ra = s.r_alpha_evals.p;
        rc_check(ctx, spmv_run(ctx, pk.at.rowptr.p, pk.at.col.p, pk.at.val.p, ra, ta.p, nvars, &pk.at.plan));
        rc_check(ctx, spmv_run(ctx, pk.bt.rowptr.p, pk.bt.col.p, pk.bt.val.p, ra, tb.p, nvars, &pk.bt.plan));
        rc_check(ctx, spmv_run(ctx, pk.ct.rowptr.p, pk.ct.col.p, pk.ct.val.p, ra, tc.p, nvars, &pk.ct.plan));
        Fr* out = s.t_poly.p;
        const Fr *pa = ta.p, *pb = tb.p, *pc = tc.p;
        ew(ctx, "t_evals", nvars, [=] __device__(size_t c) {
            Fr v = fp_add(fp_add(fp_mul(eta_a, pa[c]), fp_mul(eta_b, pb[c])), fp_mul(eta_c, pc[c]));
            out[reindex_by_subdomain(H, X, c)] = v;
        });
        if (s.cosets) {
            // coset 0 (= H) of q_1 - mask from what is known on H: r(alpha, .), z_A and z_B (their hiding terms vanish on H),
            // t (before its interpolation) and z = w v_X + x (the assignment where w_evals put it: x on the X-subgroup is the
            // instance, the head of s.z)
            s.q1 = DVec(ctx, 3 * H);
            Fr* q = s.q1.p;
            const Fr *rh = s.r_alpha_evals.p, *za = s.za_evals.p, *zb = s.zb_evals.p, *th = s.t_poly.p, *zz = s.z.p;
            const uint64_t ratio = H / X;
            const size_t nwit = s.shape.nwit, ninst = s.ninst;
            ew(ctx, "round2_pointwise_h", H, [=] __device__(size_t k) {
                Fr zk;
                if (k % ratio == 0) {
                    zk = zz[k / ratio];
                } else {
                    const size_t wi = k - k / ratio - 1;
                    zk = wi < nwit ? zz[ninst + wi] : fp_zero<Fr>();
                }
                q[k] = round2_outer_form(eta_a, eta_b, eta_c, rh[k], za[k], zb[k], zk, th[k]);
            });
        }
        dv_ntt(ctx, s.t_poly, pk.logH, true);
    }
    s.tr.tick("r2: t polynomial enqueued");
    s.P_t.p = s.t_poly.p;
    s.P_t.n = H;
    pc_commit_begin(ctx, pk, &s.lane, s.P_t.p, s.P_t.n, false, 0, false, &s.j2[0]);  // overlaps the 4|H|-domain work below
}

// ---- round 2: q_1 = r(alpha, X) sum_M eta_M z_M - t z + mask in the round's layout, and (h_1, X g_1) = q_1 / v_H
// On cosets the form covers cosets 1 | 2 (coset 0 is in place since round2_t); the way back is three |H|-point inverse transforms,
// then the three blocks of q_1 - mask recovered, the mask added and v_H divided out in one pass: h_1 = q[H, 3H) + q[2H, 3H) X^H,
// X g_1 = q0 + q1 + q2
void round2_q1(swm_ctx* ctx, const swm_pk& pk, ProveState& s) {
    const uint64_t H = s.H, M = s.M;
    const size_t Mloc = s.sp.Mloc;
    const Fr eta_a = s.st.eta_a, eta_b = s.st.eta_b, eta_c = s.st.eta_c;
    const size_t off = s.cosets ? H : 0, n = s.cosets ? 2 * H : Mloc;  // what the form is evaluated on, and where in q1
    if (!s.cosets) s.q1 = DVec(ctx, Mloc);  // the whole product domain, or the rank's share of it (shard_r2)
    const Fr* mp = s.mask.p;
    {
        const Fr* pra = s.e_ra.p + off;  // (r_alpha's closed form covers coset 0 too)
        if (!s.ra_closed_form) {
            DVec ra_poly = dv_ntt_from(ctx, s.r_alpha_evals.p, H, pk.logH, true);
            s.e_ra = on_round2_layout(ctx, s, ra_poly.p, H);
            pra = s.e_ra.p;
        }
        DVec e_t = on_round2_layout(ctx, s, s.t_poly.p, H);
        Fr* out = s.q1.p + off;
        const Fr *pza = s.e_za.p, *pzb = s.e_zb.p, *pt = e_t.p, *pz = s.e_z.p;
        ew(ctx, "round2_pointwise", n, [=] __device__(size_t i) {
            out[i] = round2_outer_form(eta_a, eta_b, eta_c, pra[i], pza[i], pzb[i], pz[i], pt[i]);
        });
        s.e_za.release();
        s.e_zb.release();
        s.e_z.release();
    }
    s.h1 = DVec(ctx, 3 * H);
    s.g1x = DVec(ctx, H);
    Fr* q = s.q1.p;
    if (s.cosets) {
        rc_check(ctx, ntt_cosets_inv(ctx, q, pk.logH, 3));
        Fr *h = s.h1.p, *g = s.g1x.p;
        const Fr iota = HDomain(4).gen, half = fr_half();
        ew(ctx, "q1_cosets_solve_div_vh", H, [=] __device__(size_t j) {
            const Cosets3 c = cosets3_solve(q[j], q[j + H], q[j + 2 * H], iota, half);
            const Fr p0 = fp_add(c.p0, mp[j]), p1 = fp_add(c.p1, mp[j + H]), p2 = fp_add(c.p2, mp[j + 2 * H]);
            const Fr hj = fp_add(p1, p2);
            h[j] = hj;
            h[j + H] = p2;
            h[j + 2 * H] = fp_zero<Fr>();
            g[j] = fp_add(p0, hj);
        });
    } else if (!s.sp.r2) {
        dv_ntt(ctx, s.q1, s.logM, true);
        ew(ctx, "q1_add_mask", s.mask_len, [=] __device__(size_t i) { q[i] = fp_add(q[i], mp[i]); });
        div_vh(ctx, q, H, M, s.h1.p, s.g1x.p);
    } else {
        rc_check(ctx, ntt_sharded_run(ctx, q, s.logM, 1, 1));  // BLOCKS evaluations -> CYCLIC coefficients: q1[j] = q_1[rank + G j]
        const size_t s_rank = s.sp.rank, s_world = s.sp.SG, mask_len = s.mask_len;
        ew(ctx, "q1_add_mask", Mloc, [=] __device__(size_t j) {
            const size_t i = s_rank + s_world * j;
            if (i < mask_len) q[j] = fp_add(q[j], mp[i]);
        });
        const size_t Hl = H / s.sp.SG;
        DVec loc(ctx, 4 * Hl), all(ctx, 4 * Hl * s.sp.SG);  // [h_1 share: 3 Hl | (X g_1) share: Hl]
        div_vh(ctx, q, Hl, Mloc, loc.p, loc.p + 3 * Hl);
        rc_check(ctx, shard_allgather_dev(ctx, loc.p, 4 * Hl * sizeof(Fr), all.p));
        Fr* ph = s.h1.p;
        Fr* pg = s.g1x.p;
        const Fr* pa = all.p;
        const unsigned lg = s.sp.slog_g;
        ew(ctx, "shard_interleave", 3 * H, [=] __device__(size_t i) {
            const size_t r = i & (((size_t)1 << lg) - 1), j = i >> lg;
            ph[i] = pa[r * 4 * Hl + j];
            if (i < Hl << lg) pg[i] = pa[r * 4 * Hl + 3 * Hl + j];  // |H| of them
        });
    }
}

// ---- round 2: the commitments to t, g_1, h_1 and the outer sumcheck's remainder check
void round2_commitments(swm_ctx* ctx, const swm_pk& pk, ProveState& s) {
    const uint64_t H = s.H;
    s.P_g1.p = s.g1x.p + 1; s.P_g1.n = H - 1; s.P_g1.has_bound = true; s.P_g1.bound = H - 2; s.P_g1.hiding = true;
    s.P_h1.p = s.h1.p; s.P_h1.n = 2 * H + 1;  // degree <= 2|H| + 2 zk_bound - 2 (higher slots are zero)
    pc_commit_begin(ctx, pk, &s.lane, s.P_h1.p, s.P_h1.n, false, 0, false, &s.j2[2]);  // largest first
    pc_commit_begin(ctx, pk, &s.lane, s.P_g1.p, s.P_g1.n, true, H - 2, true, &s.j2[1]);
    commit_flush(ctx);
    // the sumcheck remainder check needs a download; do it while the MSMs run
    Fr rem0 = s.g1x.download(0, 1)[0];
    bool unsat = !fp_is_zero(rem0);
    pc_commit_blind(pk, &s.j2[0], nullptr, &s.P_t.rand);
    pc_commit_blind(pk, &s.j2[1], &s.zk, &s.P_g1.rand);
    pc_commit_blind(pk, &s.j2[2], nullptr, &s.P_h1.rand);
    commit_gather(ctx, {&s.j2[0].plain, &s.j2[1].plain, &s.j2[1].shifted, &s.j2[2].plain});
    pc_commit_end_round(ctx, pk, {&s.j2[0], &s.j2[1], &s.j2[2]}, {nullptr, &s.zk, nullptr},
                        {&s.P_t.rand, &s.P_g1.rand, &s.P_h1.rand}, s.comms2.data());
    // (measurement builds only, -DSWM_MEASURE_HOOKS: a proof during which an EMULATED exchange actually ran — capi.hip — has wrong
    // values by construction and only its time is of interest; the shipped library has no such path)
    if (unsat && !ctx->emulated_exchange)
        throw MarlinError(SWM_ERR_UNSATISFIED, "outer sumcheck does not hold: constraint system is not satisfied");
}

// ---- round 3: f on K, its commitment (as g_2), and h_2 = (a - b f) / v_K via evaluations on the 4|K| domain.
// Over G ranks the second part runs the way round 2 does: f into the 4|K| domain, the pointwise form a - b f (the key's twelve
// arrays read at the rank's BLOCKS indices) and the transform back on a rank's share; the division by v_K is local in the
// CYCLIC layout; h_2 is all-gathered afterwards (3|K| x 32 B).
void round3_polys(swm_ctx* ctx, const swm_pk& pk, ProveState& s) {
    const uint64_t K = s.K, Bsz = s.Bsz;
    const Fr alpha = s.st.alpha, beta = s.st.beta;
    const Fr eta_a = s.st.eta_a, eta_b = s.st.eta_b, eta_c = s.st.eta_c;
    const Fr vhab = fp_mul(s.dh.vanishing(alpha), s.dh.vanishing(beta));
    s.f = DVec(ctx, K);
    // f on K is kept (SWM_OUTER_COSETS): coset 0 of the 4|K| domain, so that f's forward transform covers cosets 1 - 3 only
    const bool f_cosets = SWM_OUTER_COSETS && !s.sp.r3 && Bsz == 4 * K && K >= OUTER_COSETS_MIN_H;
    DVec f_K;
    {
        // the three denominator vectors share one buffer and ONE batch inversion: its cost is the serial Fermat chain of
        // a lane (~0.4 ms whatever the length), so three launches would pay it three times
        DVec inv(ctx, 3 * K);
        for (int m = 0; m < 3; m++) {
            Fr* out = inv.p + (size_t)m * K;
            const Fr *rk = pk.ar[m].row_K.p, *ck = pk.ar[m].col_K.p;
            ew(ctx, "round3_den_K", K, [=] __device__(size_t i) { out[i] = fp_mul(fp_sub(beta, rk[i]), fp_sub(alpha, ck[i])); });
        }
        rc_check(ctx, batch_inverse_run(ctx, inv.p, 3 * K));
        Fr* out = s.f.p;
        const Fr *ia = inv.p, *ib = inv.p + K, *ic = inv.p + 2 * K;
        const Fr *va = pk.ar[0].val_K.p, *vb = pk.ar[1].val_K.p, *vc = pk.ar[2].val_K.p;
        if (f_cosets) {
            f_K = DVec(ctx, K);
            out = f_K.p;
        }
        ew(ctx, "round3_f_K", K, [=] __device__(size_t i) {
            Fr t = fp_add(fp_add(fp_mul(fp_mul(eta_a, va[i]), ia[i]), fp_mul(fp_mul(eta_b, vb[i]), ib[i])),
                          fp_mul(fp_mul(eta_c, vc[i]), ic[i]));
            out[i] = fp_mul(vhab, t);
        });
        if (f_cosets) rc_check(ctx, ntt_run_from(ctx, s.f.p, pk.logK, 1, 0, f_K.p, K));
        else dv_ntt(ctx, s.f, pk.logK, true);
    }
    s.P_g2.p = s.f.p + 1; s.P_g2.n = K - 1; s.P_g2.has_bound = true; s.P_g2.bound = K - 2;
    pc_commit_begin(ctx, pk, &s.lane, s.P_g2.p, s.P_g2.n, true, K - 2, false, &s.j3[0]);  // overlaps the 4|K|-domain work below
    s.h2 = DVec(ctx, 3 * K);
    const IndexOnB ix{pk.ar[0].row_B.p, pk.ar[0].col_B.p, pk.ar[0].row_col_B.p, pk.ar[0].val_B.p,
                      pk.ar[1].row_B.p, pk.ar[1].col_B.p, pk.ar[1].row_col_B.p, pk.ar[1].val_B.p,
                      pk.ar[2].row_B.p, pk.ar[2].col_B.p, pk.ar[2].row_col_B.p, pk.ar[2].val_B.p};
    const Round3Challenges ch{alpha, beta, fp_mul(beta, alpha), fp_mul(vhab, eta_a), fp_mul(vhab, eta_b), fp_mul(vhab, eta_c)};
    // f in the round's layout (cosets: 1 - 3 behind the kept coset 0, f_K), a - b f there, and back to coefficients.  On cosets
    // only f is laid out that way: a - b f itself is dense, so that one 4|K|-point transform takes it back.
    const size_t Bloc = s.sp.r3 ? Bsz / s.sp.SG : Bsz;
    with_product_map(s.sp, s.sp.r3, Bloc, f_cosets, pk.logK, [&](auto map) {
        constexpr bool blocks = std::is_same_v<decltype(map), BlocksMap>, cosets = std::is_same_v<decltype(map), CosetsMap>;
        DVec e_f;
        if constexpr (blocks) {
            e_f = shard_evals(ctx, s.sp, s.f.p, K, pk.logB);
        } else if constexpr (cosets) {
            static const unsigned ks[3] = {1, 2, 3};
            e_f = DVec(ctx, 3 * K);
            rc_check(ctx, ntt_cosets_fwd(ctx, s.f.p, K, pk.logK, ks, 3, e_f.p));
        } else {
            e_f = dv_ntt_from(ctx, s.f.p, K, pk.logB, false);
        }
        DVec ab(ctx, Bloc);
        Fr* out = ab.p;
        // Every fourth point of the 4|K| domain is a point of K, where f IS a / b (round3_f_K; row_col = row col there): a - b f
        // vanishes on coset 0 exactly and is written as zero, not computed.  On cosets f_K is then not read here.
        const bool on_K_every_4th = Bsz == 4 * K;  // (|K| = 2 has a product domain of 2|K| points: computed everywhere)
        const Fr* pf = e_f.p;
        ew(ctx, "round3_pointwise_B", Bloc, [=] __device__(size_t p) {
            if constexpr (cosets) {  // (a - b f is dense: p is the point; f sits at cosets 1 | 2 | 3 behind the kept coset 0)
                out[p] = (p & 3) == 0 ? fp_zero<Fr>() : round3_a_minus_bf(ix, ch, p, pf[map.position(p) - K]);
            } else {
                const size_t i = map.index(p);
                out[p] = on_K_every_4th && (i & 3) == 0 ? fp_zero<Fr>() : round3_a_minus_bf(ix, ch, i, pf[p]);
            }
        });
        if constexpr (blocks) {
            const size_t Kl = K / s.sp.SG;
            rc_check(ctx, ntt_sharded_run(ctx, ab.p, pk.logB, 1, 1));  // -> CYCLIC coefficients: ab[j] = (a - b f)[rank + G j]
            DVec loc(ctx, 3 * Kl);
            div_vk(ctx, ab.p, Kl, Bloc, loc.p);
            shard_gather_cyclic(ctx, loc.p, 3 * Kl, s.sp.slog_g, s.h2.p, 3 * K);
        } else {
            dv_ntt(ctx, ab, pk.logB, true);
            div_vk(ctx, ab.p, K, Bsz, s.h2.p);
        }
    });
    s.P_h2.p = s.h2.p;
    s.P_h2.n = 3 * K >= 3 ? 3 * K - 3 : 0;  // degree <= 3|K| - 4
}

// ---- evaluations.  Everything asked at beta depends on rounds 1-2 only, so it is enqueued before the round-3 commitments
// are awaited and runs under them; then gamma and the evaluations at gamma; then the linear combinations.  Returns the
// proof's evaluations (label order).
std::vector<Fr> evaluations(swm_ctx* ctx, const swm_pk& pk, ProveState& s) {
    // every evaluation the linear combinations can ask for, enqueued back to back and downloaded once
    std::map<std::pair<std::string, bool>, Fr> eval_cache;  // (label, at_gamma)
    {
        std::vector<std::pair<std::string, bool>> want;
        for (const char* l : {"z_b", "t", "g_1", "mask_poly", "z_a", "w", "h_1"}) want.push_back({l, false});
        for (int i = 0; i < 12; i++) want.push_back({kIndexerPolys[i], true});
        want.push_back({"g_2", true});
        want.push_back({"h_2", true});
        DVec slots(ctx, want.size());
        auto enqueue_at = [&](bool at_gamma, const EvalPoint& ep) {
            std::vector<EvalItem> items;
            for (size_t i = 0; i < want.size(); i++) {
                if (want[i].second != at_gamma) continue;
                LPoly* lp = s.polys.at(want[i].first);
                items.push_back({lp->p, lp->n, slots.p + i});
            }
            poly_eval_many(ctx, items, ep);
        };
        EvalPoint ep_beta = eval_point(ctx, s.st.beta);
        enqueue_at(false, ep_beta);
        commit_gather(ctx, {&s.j3[0].plain, &s.j3[0].shifted, &s.j3[1].plain});
        pc_commit_end_round(ctx, pk, {&s.j3[0], &s.j3[1]}, {nullptr, nullptr}, {&s.P_g2.rand, &s.P_h2.rand}, s.comms3.data());
        s.tr.mark("round 3 commitments");
        fs_absorb_commitments(s.fs, s.comms3);
        s.st.gamma = s.fs.rand_fr();
        EvalPoint ep_gamma = eval_point(ctx, s.st.gamma);
        enqueue_at(true, ep_gamma);
        std::vector<Fr> vals = slots.download(0, want.size());
        for (size_t i = 0; i < want.size(); i++) eval_cache[want[i]] = vals[i];
    }
    const Fr beta = s.st.beta, gamma = s.st.gamma;
    auto poly_at = [&](const std::string& label, const Fr& point) {
        bool at_gamma = fp_eq(point, gamma);
        auto key = std::make_pair(label, at_gamma);
        auto it = eval_cache.find(key);
        if (it != eval_cache.end()) return it->second;
        LPoly* lp = s.polys.at(label);
        Fr v = poly_eval(ctx, lp->p, lp->n, point);
        eval_cache[key] = v;
        return v;
    };
    auto provider = [&](const std::string&, const LcTerms& terms, const Fr& point) {
        Fr acc = fp_zero<Fr>();
        for (auto& t : terms) acc = fp_add(acc, t.second.empty() ? t.first : fp_mul(t.first, poly_at(t.second, point)));
        return acc;
    };
    s.lcs = construct_linear_combinations(pk.info, s.public_input, provider, s.st);
    std::vector<std::pair<std::string, Fr>> evals;
    for (auto& q : kQuerySet) {
        const Fr& pt = std::string(q.point) == "beta" ? beta : gamma;
        Fr v = provider(q.label, s.lcs.at(q.label), pt);
        if (lc_has_zero_eval(q.label)) {
            if (!fp_is_zero(v) && !ctx->emulated_exchange)  // (see the outer sumcheck's check)
                throw MarlinError(SWM_ERR_UNSATISFIED, std::string(q.label) + " does not evaluate to zero: constraint system is not satisfied");
            continue;
        }
        evals.push_back({q.label, v});
    }
    std::sort(evals.begin(), evals.end(), [](auto& a, auto& b) { return a.first < b.first; });
    std::vector<Fr> out;
    for (auto& e : evals) out.push_back(e.second);
    return out;
}

// ---- MarlinKZG10::open_combinations: per query point, labels in sorted order, challenges xi^0, xi^1, ...
// Phase 1 builds the combined polynomial, its witness and the shifted witnesses for BOTH points and enqueues all
// their MSMs; phase 2 waits and adds the host-side hiding terms.  Nothing is awaited before everything is enqueued.
// A point's witness is MSM(powers, wq) + MSM(powers from off on, k sq) (+ hiding), off = srs_max_degree - bound.  Where the
// shifted powers are a sub-range of the powers (swm_pk::in_powers: an SRS of the circuit's own degree) both read one table and
//   MSM(powers, wq) + MSM(powers + off, k sq) = MSM(powers, wq + X^off k sq)
// (G1 has order r, the scalars add in Fr): ONE job per point, and a position costs one mixed addition instead of two wherever
// both quotients are non-zero.  The fold comes after both divisions: the shifted witness is X^off (g / (X - z)), not the quotient
// of X^off g.  -DSWM_OPEN_FOLD=0 builds the two-job path, which a key with shifted powers on a table of their own takes anyway.
#ifndef SWM_OPEN_FOLD
#define SWM_OPEN_FOLD 1
#endif
// wq[t] += k * sq[t], t < n (wq: the plain quotient from X^off on; sq: the bounded member's quotient)
__global__ void __launch_bounds__(256) open_fold_shifted(Fr* __restrict__ wq, const Fr* __restrict__ sq, size_t n, Fr k) {
    SWM_LIGHT_KERNEL();
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x)
        wq[t] = fp_add(wq[t], fp_mul(sq[t], k));
}
std::vector<PcProof> open_combinations(swm_ctx* ctx, const swm_pk& pk, ProveState& s, const Fr& xi) {
    struct ShiftedTerm {
        LPoly* lp;
        Fr ch;
    };
    static constexpr int MAX_COMBINE = 24;
    struct CombineTerms {
        const Fr* src[MAX_COMBINE];
        size_t len[MAX_COMBINE];
        Fr k[MAX_COMBINE];
    };
    struct PointOpen {
        Fr point;
        DivResult wq;
        std::vector<DivResult> sq;
        AsyncMsm wjob;
        std::vector<AsyncMsm> sjobs;
        AsyncMsm folded_slot;  // a folded point's place in the sharded exchange (below): never a job, always the identity
        bool folded = false;
        HPoly r_comb, shifted_r, shifted_r_witness;
        std::vector<ShiftedTerm> shifted_terms;
    };
    const char* points[2] = {"beta", "gamma"};
    PointOpen po[2];
    for (int pi = 0; pi < 2; pi++) {
        const char* pl = points[pi];
        PointOpen& o = po[pi];
        o.point = pi == 0 ? s.st.beta : s.st.gamma;
        const Fr point = o.point;
        std::vector<std::string> labels;
        for (auto& q : kQuerySet)
            if (std::string(q.point) == pl) labels.push_back(q.label);
        std::sort(labels.begin(), labels.end());
        size_t plen = 0;
        for (auto& l : labels)
            for (auto& t : s.lcs.at(l))
                if (!t.second.empty()) plen = std::max(plen, s.polys.at(t.second)->n);
        CombineTerms cterms;
        int nterms = 0;
        Fr ch = fr_one();
        for (auto& l : labels) {
            const LcTerms& terms = s.lcs.at(l);
            bool single_bounded = false;
            for (auto& t : terms) {
                if (t.second.empty()) continue;
                LPoly* lp = s.polys.at(t.second);
                if (terms.size() == 1 && lp->has_bound) single_bounded = true;
                else if (lp->has_bound) throw MarlinError(SWM_ERR_INTERNAL, "EquationHasDegreeBounds");
                Fr k = fp_mul(ch, t.first);
                if (nterms >= MAX_COMBINE) throw MarlinError(SWM_ERR_INTERNAL, "too many terms in an opening");
                cterms.src[nterms] = lp->p;
                cterms.len[nterms] = lp->n;
                cterms.k[nterms] = k;
                nterms++;
                hp_add_scaled(o.r_comb, lp->rand.rand, k);
            }
            ch = fp_mul(ch, xi);
            if (single_bounded) {
                LPoly* lp = s.polys.at(terms[0].second);
                o.shifted_terms.push_back({lp, ch});
                hp_add_scaled(o.shifted_r, lp->rand.shifted_rand, ch);
                if (!hp_is_zero(lp->rand.shifted_rand)) hp_add_scaled(o.shifted_r_witness, hp_div_linear(lp->rand.shifted_rand, point), ch);
                ch = fp_mul(ch, xi);
            }
        }
        // witness = p / (X - point) against the powers; degree-bounded members: shifted witnesses against the shifted powers,
        // folded into the plain quotient where both read the powers' table (then the job follows BOTH divisions)
        size_t wn = plen ? plen - 1 : 0;  // coefficients of the (merged) witness quotient
        std::vector<bool> folded(o.shifted_terms.size(), false);
        for (size_t i = 0; i < o.shifted_terms.size(); i++) {
            const LPoly* lp = o.shifted_terms[i].lp;
            const size_t off = pk.srs_max_degree - lp->bound, qn = lp->n ? lp->n - 1 : 0;
            folded[i] = SWM_OPEN_FOLD && qn && pk.in_powers(off, qn);
            if (folded[i]) wn = std::max(wn, off + qn);
        }
        {   // comb[i] = sum_j k_j * src_j[i]: every polynomial is read once, the combination written once — straight into the
            // buffer it is divided in, zero above it (i >= every length) up to the room the folded quotients need
            DVec work(ctx, std::max<size_t>(plen, wn + 1));
            Fr* out = work.p;
            const int nt = nterms;
            ew(ctx, "open_combine", work.n, [=] __device__(size_t i) {
                Fr acc = fp_zero<Fr>();
                for (int j = 0; j < nt; j++)
                    if (i < cterms.len[j]) acc = fp_add(acc, fp_mul(cterms.k[j], cterms.src[j][i]));
                out[i] = acc;
            });
            s.tr.tick(pi == 0 ? "open beta: combination enqueued" : "open gamma: combination enqueued");
            o.wq = div_linear_in_place(ctx, std::move(work), plen, point);
        }
        s.tr.tick("  witness quotient enqueued");
        const bool fold_any = std::find(folded.begin(), folded.end(), true) != folded.end();
        if (!fold_any) {
            commit_enqueue(ctx, &s.lane, pk, 0, o.wq.work.p + 1, wn, &o.wjob);
            s.tr.tick("  witness commitment enqueued");
        }
        o.sq.resize(o.shifted_terms.size());
        o.sjobs.reserve(o.shifted_terms.size());  // (jobs in flight are referred to by address)
        for (size_t i = 0; i < o.shifted_terms.size(); i++) {
            auto& stt = o.shifted_terms[i];
            o.sq[i] = div_linear(ctx, stt.lp->p, stt.lp->n, point);
            Fr k = stt.ch;
            Fr* q = o.sq[i].work.p;
            const size_t off = pk.srs_max_degree - stt.lp->bound, qn = stt.lp->n ? stt.lp->n - 1 : 0;
            if (folded[i]) {
                const unsigned grid = (unsigned)std::min<size_t>((qn + 255) / 256, 256 * 32);
                LAUNCHX(ctx, "open_fold_shifted", open_fold_shifted, dim3(grid), dim3(256), 0, o.wq.work.p + 1 + off, q + 1, qn, k);
                s.tr.tick("  shifted quotient folded");
                continue;
            }
            ew(ctx, "open_scale", qn, [=] __device__(size_t t) { q[t + 1] = fp_mul(q[t + 1], k); });
            s.tr.tick("  shifted quotient enqueued");
            o.sjobs.emplace_back();
            commit_enqueue(ctx, &s.lane, pk, off, q + 1, qn, &o.sjobs.back());
            s.tr.tick("  shifted commitment enqueued");
        }
        if (fold_any) {
            commit_enqueue(ctx, &s.lane, pk, 0, o.wq.work.p + 1, wn, &o.wjob);
            s.tr.tick("  witness commitment enqueued");
            o.folded = true;
            o.folded_slot.sharded = o.wjob.sharded;
            o.folded_slot.result = g1_xyzz_identity();
        }
    }
    commit_flush(ctx);  // both opening points: two bucket stages (four when the shifted witnesses are jobs of their own), one launch
    s.tr.tick("open: bucket stages enqueued");
    // hiding terms of the two witnesses and the random evaluations: host work that does not depend on the MSMs in flight
    G1XYZZ hide[2];
    std::vector<PcProof> pps(2);
    for (int pi = 0; pi < 2; pi++) {
        PointOpen& o = po[pi];
        hide[pi] = g1_xyzz_identity();
        if (!hp_is_zero(o.r_comb)) {
            g1_add(hide[pi], gamma_msm(pk, hp_div_linear(o.r_comb, o.point)));
            pps[pi].has_random_v = true;
            pps[pi].random_v = host_poly_eval(o.r_comb, o.point);
        }
        if (!o.shifted_terms.empty()) {
            if (!hp_is_zero(o.shifted_r_witness)) g1_add(hide[pi], gamma_msm(pk, o.shifted_r_witness));
            if (!hp_is_zero(o.shifted_r) && pps[pi].has_random_v)
                pps[pi].random_v = fp_add(pps[pi].random_v, host_poly_eval(o.shifted_r, o.point));
        }
    }
    // sharded proving: the openings' exchange is one record of four partial sums per rank, whichever way a point's witness was
    // computed: a folded point's second sum is the identity (192 bytes; the record's size does not depend on the key)
    auto second = [](PointOpen& o) { return !o.sjobs.empty() ? &o.sjobs[0] : o.folded ? &o.folded_slot : nullptr; };
    commit_gather(ctx, {&po[0].wjob, second(po[0]), &po[1].wjob, second(po[1])});
    G1XYZZ wit[2];
    G1Affine wit_aff[2];
    for (int pi = 0; pi < 2; pi++) {
        PointOpen& o = po[pi];
        wit[pi] = commit_wait(ctx, &o.wjob);
        for (AsyncMsm& sj : o.sjobs) g1_add(wit[pi], commit_wait(ctx, &sj));
        g1_add(wit[pi], hide[pi]);
    }
    g1_to_affine_batch(wit, 2, wit_aff);
    for (int pi = 0; pi < 2; pi++) pps[pi].w = wit_aff[pi];
    return pps;
}

}  // namespace

namespace swm {

std::vector<uint8_t> prove_impl(swm_ctx* ctx, const swm_pk& pk, const swm_r1cs* cs, ChaChaRng& zk, bool uncompressed) {
    PhaseTrace tr(ctx);
    if (sw(SW_TRACE) >= 1 || sw(SW_PROOF_MARKS)) hipLaunchKernelGGL(swm_proof_begin, dim3(1), dim3(1), 0, ctx->stream);
    ProveShape shape = prove_shape(cs, pk);
    tr.mark("pad_and_square");
    shard_agree(ctx, pk);  // one proof over several ranks: all of them split the work the same way, or none starts
    ctx->emulated_exchange = false;
    ProveState s(pk, zk, tr, std::move(shape), shard_plan(ctx, pk));
    // every commitment of a small proof on ONE stream of its lane (msm_enqueue: a proof that mixes single-stream and pipelined
    // jobs runs them on aliasing streams); SWM_PROVE_ONE_STREAM_LOG: the largest log2 |H| this applies to
    // (default 19, 0 = never; measured r05, alternating runs: 2^16 7.0 -> 6.5 ms, 2^17 11.2 -> 10.8, 2^18 17.7 -> 17.5, 2^19 29.4 -> 28.6,
    // Merkle circuit 15.0 -> 14.7; at 2^20 the pipelined form is 1 ms ahead: 49.6 vs 50.6)
    struct PipeMinScope {
        swm_ctx* c;
        ~PipeMinScope() { c->msm_pipe_min = 0; }
    } pipe_scope{ctx};
    ctx->msm_pipe_min = pk.logH <= (unsigned)sw(SW_PROVE_ONE_STREAM_LOG) ? ~(size_t)0 : 0;

    // ================= round 1
    // The zero-knowledge draws of round 1 do not depend on the witness: rho_w, rho_a, rho_b, then the mask polynomial
    // (arkworks' order).  The mask is sampled and its commitment — the largest MSM of the round, 3|H| points — enqueued
    // BEFORE the witness upload: a pageable host buffer of 32 MB per 2^20 variables takes ~5 ms to reach HBM, during
    // which the GPU had nothing to do (r02 timeline).
    // Every commitment MSM is enqueued as soon as its polynomial exists (enqueueing a round's commitments together once ALL its
    // polynomials are built — so that the transforms do not run beside an accumulation — measured no gain in r02 / r04: the early
    // MSMs cover more than the slowed transforms cost; CHANGELOG.md).
    s.rho_w = zk.rand_fr();
    s.rho_a = zk.rand_fr();
    s.rho_b = zk.rand_fr();
    begin_mask(ctx, pk, s);
    upload_witness(ctx, pk, s, cs);
    tr.mark("upload z, z_A, z_B");
    round1_polys(ctx, pk, s);
    tr.mark("round 1 polynomials");
    if (!s.mask_late) commit_flush(ctx);  // round 1: all four commitments enqueued here; small ones share one bucket-stage launch
    round2_prework(ctx, s);
    if (s.mask_late) {  // everything else of the round is in flight: now the host draws the mask from the caller's generator
        draw_mask(ctx, pk, s);
        commit_flush(ctx);
    }
    tr.tick("r1: pre-work enqueued");
    round1_commitments(ctx, pk, s);
    tr.mark("round 1 commitments");
    fs_absorb_commitments(s.fs, s.comms1);
    s.st.alpha = s.fs.sample_outside(s.dh);
    s.st.eta_a = s.fs.rand_fr();
    s.st.eta_b = s.fs.rand_fr();
    s.st.eta_c = s.fs.rand_fr();

    // ================= round 2
    r_alpha(ctx, pk, s);
    round2_t(ctx, pk, s);
    round2_q1(ctx, pk, s);
    tr.mark("round 2 polynomials");
    round2_commitments(ctx, pk, s);
    tr.mark("round 2 commitments");
    fs_absorb_commitments(s.fs, s.comms2);
    s.st.beta = s.fs.sample_outside(s.dh);

    // ================= round 3
    round3_polys(ctx, pk, s);
    tr.mark("round 3 polynomials");
    pc_commit_begin(ctx, pk, &s.lane, s.P_h2.p, s.P_h2.n, false, 0, false, &s.j3[1]);
    commit_flush(ctx);

    // ================= evaluations and openings
    Proof proof;
    proof.evaluations = evaluations(ctx, pk, s);
    tr.mark("evaluations");
    fs_absorb_evals(s.fs, proof.evaluations);
    const Fr xi = s.fs.challenge_u128();
    proof.pc_proof = open_combinations(ctx, pk, s, xi);
    tr.mark("openings");
    proof.commitments = {s.comms1, s.comms2, s.comms3};
    return serialize_proof(proof, uncompressed);
}

// witness_host.h: prove_shape's comparison from the counts alone, for a unit that changes state before it calls the prover
bool pk_takes_shape(const swm_pk* pk, size_t num_instance, size_t num_witness, size_t num_constraints) {
    const size_t inst = HDomain(num_instance).size, nv = inst + num_witness, side = nv > num_constraints ? nv : num_constraints;
    return side == pk->info.num_constraints && side == pk->info.num_variables && inst == pk->info.num_instance_variables;
}

}  // namespace swm

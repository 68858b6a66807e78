// marlin.hip — MI355X-native Marlin (universal setup, indexer, prover) behind the surface of
// /root/reference/src/marlin/mod.rs:45-94.  The arithmetic the reference delegates to ark-marlin / ark-poly-commit /
// ark-poly / ark-ec (not vendored; restated from SURVEY.md Appendix A [U]) runs as HIP kernels with all polynomials
// resident in HBM between the NTTs (K2), the mat-vecs (K3), the support kernels (K4) and the commitments (K1);
// the host drives the schedule, owns the Fiat-Shamir transcript and touches only O(1)-sized data per round.
//
// Deviations from arkworks' *schedule* that leave every proof byte unchanged (polynomials are canonical objects):
//   * round 2 multiplies in evaluation form on the 4|H| domain directly (5 FFT + 1 iFFT instead of 8 + 2);
//   * round 3 forms (a - b f) in evaluation form on the 4|K| domain (1 FFT + 1 iFFT instead of 3 iFFT + 2 FFT + 1 iFFT);
//   * only the three gamma-powers KZG hiding needs are generated at setup (arkworks generates max_degree + 2).
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <functional>
#include <memory>
#include <type_traits>
#include "devops.cuh"
#include "g1.cuh"
#include "host/ahp.h"

#include "msm.h"
using namespace swm;

// launch + profile bracket, throwing MarlinError instead of returning a status
#define LAUNCHX(ctx, name, kernel, grid, block, shmem, ...)                         \
    do {                                                                            \
        prof_begin(ctx, name);                                                      \
        hipLaunchKernelGGL(kernel, grid, block, shmem, (ctx)->stream, __VA_ARGS__); \
        prof_end(ctx);                                                              \
        hip_check(ctx, hipGetLastError(), name);                                    \
    } while (0)

// ================================================================================================ handles
#include "host/pk_codec.h"      // HostCsr, the host-side prefix of the proving-key codec
#include "host/host_handles.h"  // swm_rng, swm_vk: host-only handles (shared with the sanitizer harness, tests/native/host_fuzz.cpp)
struct swm_srs {
    ~swm_srs() {
        if (d_powers) (void)hipFree(d_powers);
    }
    size_t max_degree = 0;
    // every power lies in the prime-order subgroup: true by construction for universal_setup, established by a check for an
    // imported SRS (the twisted Edwards MSM tables of the keys derived from it rely on it)
    bool in_subgroup = false;
    G1Affine* d_powers = nullptr;  // [beta^i] g, i <= max_degree (device)
    std::vector<G1Affine> gamma_powers;  // [beta^i] gamma_g, i < 3 (host)
    G2Affine h, beta_h;
};

namespace {

struct DevCsr {
    DBuf<uint32_t> rowptr, col;
    DVec val;
    size_t rows = 0, nnz = 0;
    DBuf<uint32_t> plan_chunks, plan_lrows;  // SpMV plan recorded at upload (spmv.hip): no read-back inside a proof
    SpmvPlan plan;
};
struct MatrixArith {
    DVec row, col, val, row_col;          // coefficient vectors (length K)
    DVec row_K, col_K, val_K;             // evaluations on K
    DVec row_B, col_B, val_B, row_col_B;  // evaluations on the 4K domain
};
// fixed-base table for the 3-point hiding MSMs: tab[j][w][d-1] = d * 16^w * gamma_power[j]
struct GammaTable {
    std::vector<G1Affine> t;  // 3 * 64 * 15
    const G1Affine& at(int j, int w, int d) const { return t[((size_t)j * 64 + w) * 15 + (d - 1)]; }
};

}  // namespace

struct swm_pk {
    ~swm_pk() {  // also runs when index_impl / pk_deserialize unwind with a half-built key
        if (d_powers) (void)hipFree(d_powers);
        if (d_powers28) (void)hipFree(d_powers28);   // the whole table when tab_c != 0
        if (d_shifted) (void)hipFree(d_shifted);
        if (d_shifted28) (void)hipFree(d_shifted28);
        if (d_powers_te) (void)hipFree(d_powers_te);
        if (d_shifted_te) (void)hipFree(d_shifted_te);
    }
    // A key is resident per DEVICE, read-only once built and reference-counted (swm_pk_retain / swm_pk_attach /
    // swm_pk_destroy): any context on that device proves with it, several at once — the prover takes it by const reference
    // and every per-proof buffer, stream and result slot belongs to the context.  The key's device blocks are detached from
    // the pool of the context that built them (own_blocks) so that the key may outlive that context.
    int device = 0;
    std::atomic<int> refs{1};
    void own_blocks() {
        for (DevCsr* m : {&a, &b, &c, &at, &bt, &ct}) {
            m->rowptr.detach(); m->col.detach(); m->val.detach(); m->plan_chunks.detach(); m->plan_lrows.detach();
        }
        for (MatrixArith& m : ar)
            for (DVec* v : {&m.row, &m.col, &m.val, &m.row_col, &m.row_K, &m.col_K, &m.val_K, &m.row_B, &m.col_B, &m.val_B, &m.row_col_B})
                v->detach();
    }
    IndexInfo info;
    uint64_t H = 0, K = 0, X = 0, B = 0;
    unsigned logH = 0, logK = 0, logX = 0, logB = 0;
    HostCsr ha, hb, hc;  // padded, balanced matrices (kept for key serialisation)
    DevCsr a, b, c, at, bt, ct;
    MatrixArith ar[3];
    // committer key as MarlinKZG10::trim lays it out: powers [0, supported_degree] and, for the degree-bound shifts,
    // the top of the SRS [shift_base, srs_max_degree] with shift_base = srs_max_degree - largest enforced bound.
    // d_*28: the same points scaled for the MSM inner loop (msm_scale_bases_run).
    G1Affine* d_powers = nullptr;
    G1Affine* d_powers28 = nullptr;
    G1Affine* d_shifted = nullptr;
    G1Affine* d_shifted28 = nullptr;
    size_t n_powers = 0, n_shifted = 0, shift_base = 0;
    size_t srs_max_degree = 0;
    // precomputed window multiples of both ranges (msm_table_build; width 0: none, the key is small).  Row 0 of a table IS
    // the scaled copy, so d_powers28 / d_shifted28 then point into the tables.
    unsigned tab_c = 0, shtab_c = 0;
    // the tables in twisted Edwards form (msm_table_build_te; the SRS powers lie in the prime-order subgroup): when set, the
    // flat schedule runs on them and d_*28 are the n-point scaled copies only
    G1TE* d_powers_te = nullptr;
    G1TE* d_shifted_te = nullptr;
    // whether bases_at serves the n powers from `offset` on out of the powers' own table: an MSM against them can then be
    // folded into one against the powers from 0 on (open_combinations)
    bool in_powers(size_t offset, size_t n) const { return offset + n <= n_powers; }
    // bases for an MSM of n points starting at SRS power `offset`
    void bases_at(size_t offset, size_t n, const G1Affine** b, const G1Affine** b28, MsmTable* tab) const {
        *tab = MsmTable();
        if (in_powers(offset, n)) {
            *b = d_powers + offset;
            *b28 = d_powers28 + offset;
            if (tab_c) *tab = MsmTable{d_powers_te ? nullptr : d_powers28, n_powers, tab_c, offset, d_powers_te};
        } else if (offset >= shift_base && offset + n <= shift_base + n_shifted) {
            *b = d_shifted + (offset - shift_base);
            *b28 = d_shifted28 + (offset - shift_base);
            if (shtab_c) *tab = MsmTable{d_shifted_te ? nullptr : d_shifted28, n_shifted, shtab_c, offset - shift_base, d_shifted_te};
        } else {
            throw MarlinError(SWM_ERR_INDEX_TOO_LARGE, "polynomial does not fit the committer key");
        }
    }
    std::vector<G1Affine> gamma_powers;
    GammaTable gtab;
    VerifyingKey vk;
};

namespace {

// ================================================================================================ host helpers
Fr fr_one() { return fp_one<Fr>(); }

// batch XYZZ -> affine on the host (one inversion)
std::vector<G1Affine> batch_normalize(const std::vector<G1XYZZ>& pts) {
    std::vector<Fq> pref(pts.size());
    Fq acc = fp_one<Fq>();
    for (size_t i = 0; i < pts.size(); i++) {
        if (!g1_is_inf(pts[i])) acc = fp_mul(acc, fp_mul(pts[i].zz, pts[i].zzz));
        pref[i] = acc;
    }
    Fq inv = fp_inv(acc);
    std::vector<G1Affine> out(pts.size());
    for (size_t i = pts.size(); i-- > 0;) {
        if (g1_is_inf(pts[i])) {
            out[i] = g1_affine_identity();
            continue;
        }
        Fq zi = i ? fp_mul(inv, pref[i - 1]) : inv;  // 1 / (zz * zzz)
        inv = fp_mul(inv, fp_mul(pts[i].zz, pts[i].zzz));
        out[i].x = fp_mul(pts[i].x, fp_mul(zi, pts[i].zzz));
        out[i].y = fp_mul(pts[i].y, fp_mul(zi, pts[i].zz));
    }
    return out;
}

GammaTable build_gamma_table(const std::vector<G1Affine>& gp) {
    std::vector<G1XYZZ> pts;
    pts.reserve(gp.size() * 64 * 15);
    for (size_t j = 0; j < gp.size(); j++) {
        G1XYZZ base = g1_from_affine(gp[j]);
        for (int w = 0; w < 64; w++) {
            G1XYZZ acc = base;
            pts.push_back(acc);
            for (int d = 2; d <= 15; d++) {
                g1_add(acc, base);
                pts.push_back(acc);
            }
            for (int k = 0; k < 4; k++) base = g1_dbl(base);
        }
    }
    GammaTable t;
    t.t = batch_normalize(pts);
    return t;
}
// sum_j coeffs[j] * gamma_power[j]  (KZG10 hiding terms; <= 3 points, host arithmetic)
G1XYZZ gamma_msm(const swm_pk& pk, const std::vector<Fr>& coeffs) {
    G1XYZZ acc = g1_xyzz_identity();
    for (size_t j = 0; j < coeffs.size() && j < pk.gamma_powers.size(); j++) {
        Fr s = fp_to_std(coeffs[j]);
        for (int w = 0; w < 64; w++) {
            unsigned d = (s.v[w >> 3] >> ((w & 7) * 4)) & 15;
            if (d) g1_add_mixed(acc, pk.gtab.at((int)j, w, (int)d));
        }
    }
    return acc;
}

// host polynomial helpers for the degree-<=2 blinding polynomials
typedef std::vector<Fr> HPoly;
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

// ------------------------------------------------------------------------------------------------ R1CS padding
struct PaddedR1cs {
    std::vector<Fr> inst, wit;
    HostCsr a, b, c;
    size_t ncons = 0;
};

HostCsr import_csr(const uint32_t* rowptr, const uint32_t* col, const uint64_t* val, size_t rows, size_t old_ninst,
                   size_t shift, size_t ncols_total) {
    HostCsr m;
    m.rowptr.assign(1, 0);
    if (rows && !rowptr) throw MarlinError(SWM_ERR_INVALID_ARG, "r1cs: null rowptr");
    for (size_t r = 0; r < rows; r++) {
        if (rowptr[r + 1] < rowptr[r]) throw MarlinError(SWM_ERR_INVALID_ARG, "r1cs: rowptr not monotone");
        std::vector<std::pair<uint32_t, Fr>> ent;
        for (uint32_t k = rowptr[r]; k < rowptr[r + 1]; k++) {
            uint32_t c = col[k];
            if (c >= old_ninst) c += (uint32_t)shift;  // witness columns move behind the padded instance
            if (c >= ncols_total) throw MarlinError(SWM_ERR_INVALID_ARG, "r1cs: column out of range");
            Fr v = fp_from_limbs<Fr>((const uint32_t*)(val + 4 * (size_t)k));
            ent.push_back({c, v});
        }
        std::stable_sort(ent.begin(), ent.end(), [](auto& x, auto& y) { return x.first < y.first; });
        for (size_t i = 0; i < ent.size();) {
            Fr acc = ent[i].second;
            size_t j = i + 1;
            while (j < ent.size() && ent[j].first == ent[i].first) acc = fp_add(acc, ent[j++].second);
            if (!fp_is_zero(acc)) {
                m.col.push_back(ent[i].first);
                m.val.push_back(acc);
            }
            i = j;
        }
        m.rowptr.push_back((uint32_t)m.col.size());
    }
    return m;
}

// ark-marlin constraint_systems.rs: pad_input_for_indexer_and_prover + make_matrices_square.
PaddedR1cs pad_and_square(const swm_r1cs* cs) {
    if (!cs || cs->num_instance == 0 || !cs->instance) throw MarlinError(SWM_ERR_INVALID_ARG, "r1cs: bad arguments");
    PaddedR1cs p;
    for (size_t i = 0; i < cs->num_instance; i++) p.inst.push_back(fp_from_limbs<Fr>((const uint32_t*)(cs->instance + 4 * i)));
    for (size_t i = 0; i < cs->num_witness; i++) p.wit.push_back(fp_from_limbs<Fr>((const uint32_t*)(cs->witness + 4 * i)));
    if (!fp_is_one(p.inst[0])) throw MarlinError(SWM_ERR_INVALID_ARG, "r1cs: instance[0] must be one");
    HDomain dx(p.inst.size());
    size_t shift = dx.size - p.inst.size();
    p.inst.resize(dx.size, fp_zero<Fr>());
    size_t nvars = p.inst.size() + p.wit.size();
    size_t ncons = cs->num_constraints;
    size_t total_cols = nvars;
    p.a = import_csr(cs->a_rowptr, cs->a_col, cs->a_val, ncons, cs->num_instance, shift, total_cols);
    p.b = import_csr(cs->b_rowptr, cs->b_col, cs->b_val, ncons, cs->num_instance, shift, total_cols);
    p.c = import_csr(cs->c_rowptr, cs->c_col, cs->c_val, ncons, cs->num_instance, shift, total_cols);
    if (nvars > ncons) {
        for (HostCsr* m : {&p.a, &p.b, &p.c}) m->rowptr.resize(nvars + 1, m->rowptr.back());
        ncons = nvars;
    } else {
        p.wit.resize(p.wit.size() + (ncons - nvars), fp_one<Fr>());  // dummy unconstrained variables (value one)
    }
    p.ncons = ncons;
    return p;
}

// ark-marlin balance_matrices: greedily swap rows between A and B while A is the denser one
void balance_matrices(HostCsr& a, HostCsr& b) {
    size_t rows = a.rows();
    size_t a_density = a.nnz(), b_density = b.nnz();
    size_t max_density = std::max(a_density, b_density);
    bool a_is_denser = a_density == max_density;
    std::vector<uint8_t> swapped(rows, 0);
    for (size_t i = 0; i < rows; i++) {
        if (a_is_denser) {
            size_t la = a.rowptr[i + 1] - a.rowptr[i], lb = b.rowptr[i + 1] - b.rowptr[i];
            swapped[i] = 1;
            a_density = a_density - la + lb;
            b_density = b_density - lb + la;
            max_density = std::max(a_density, b_density);
            a_is_denser = a_density == max_density;
        }
    }
    HostCsr na, nb;
    na.rowptr.assign(1, 0);
    nb.rowptr.assign(1, 0);
    for (size_t i = 0; i < rows; i++) {
        const HostCsr& sa = swapped[i] ? b : a;
        const HostCsr& sb = swapped[i] ? a : b;
        for (uint32_t k = sa.rowptr[i]; k < sa.rowptr[i + 1]; k++) {
            na.col.push_back(sa.col[k]);
            na.val.push_back(sa.val[k]);
        }
        for (uint32_t k = sb.rowptr[i]; k < sb.rowptr[i + 1]; k++) {
            nb.col.push_back(sb.col[k]);
            nb.val.push_back(sb.val[k]);
        }
        na.rowptr.push_back((uint32_t)na.col.size());
        nb.rowptr.push_back((uint32_t)nb.col.size());
    }
    a = std::move(na);
    b = std::move(nb);
}

HostCsr transpose(const HostCsr& m, size_t ncols) {
    HostCsr t;
    t.rowptr.assign(ncols + 1, 0);
    for (auto c : m.col) t.rowptr[c + 1]++;
    for (size_t i = 0; i < ncols; i++) t.rowptr[i + 1] += t.rowptr[i];
    t.col.resize(m.nnz());
    t.val.resize(m.nnz());
    std::vector<uint32_t> cur(t.rowptr.begin(), t.rowptr.end() - 1);
    for (size_t r = 0; r < m.rows(); r++)
        for (uint32_t k = m.rowptr[r]; k < m.rowptr[r + 1]; k++) {
            uint32_t pos = cur[m.col[k]]++;
            t.col[pos] = (uint32_t)r;
            t.val[pos] = m.val[k];
        }
    return t;
}

DevCsr upload_csr(swm_ctx* ctx, const HostCsr& m) {
    DevCsr d;
    d.rows = m.rows();
    d.nnz = m.nnz();
    SpmvPlanHost ph;
    spmv_plan_build(m.rowptr.data(), d.rows, &ph);
    d.plan.nnz = ph.nnz;
    d.plan.max_row = ph.max_row;
    d.plan.n_chunks = (uint32_t)(ph.chunks.size() / 3);
    d.plan.n_lrows = (uint32_t)(ph.lrows.size() / 3);
    if (d.plan.n_chunks) {
        d.plan_chunks = DBuf<uint32_t>(ctx, ph.chunks.size());
        d.plan_chunks.upload(ph.chunks.data(), ph.chunks.size());
        d.plan_lrows = DBuf<uint32_t>(ctx, ph.lrows.size());
        d.plan_lrows.upload(ph.lrows.data(), ph.lrows.size());
        d.plan.d_chunks = d.plan_chunks.p;
        d.plan.d_lrows = d.plan_lrows.p;
    }
    d.rowptr = DBuf<uint32_t>(ctx, m.rowptr.size());
    d.rowptr.upload(m.rowptr.data(), m.rowptr.size());
    d.col = DBuf<uint32_t>(ctx, std::max<size_t>(m.nnz(), 1));
    d.val = DVec(ctx, std::max<size_t>(m.nnz(), 1));
    if (m.nnz()) {
        d.col.upload(m.col.data(), m.nnz());
        d.val.upload(m.val.data(), m.nnz());
    }
    return d;
}

uint64_t ahp_max_degree(uint64_t num_constraints, uint64_t num_variables, uint64_t num_non_zero) {
    uint64_t h = HDomain(std::max(num_constraints, num_variables)).size, k = HDomain(num_non_zero).size;
    uint64_t m = std::max(2 * h - 1, 3 * h - 1);  // zk_bound = 1
    m = std::max(m, h);
    if (3 * k >= 3) m = std::max(m, 3 * k - 3);
    return m;
}

// ================================================================================================ commitments
// One proof over G ranks only works when every rank takes the SAME decisions about how commitments are split and which
// rounds run on a rank's share: those depend on state that is local to a rank — whether its key has window tables (decided
// by the free HBM the rank saw, msm_install_bases), their widths, the experiment switches of its process.  A rank that
// goes cyclic while another splits by range leaves coefficients uncovered (the proof silently fails to verify); ranks that
// disagree on a sharded round stop matching their exchanges (the job hangs).  So that state is all-gathered once per
// call (one 32-byte record per rank) and any difference is an error here, before anything is computed.  
void shard_agree(swm_ctx* ctx, const swm_pk& pk) {
    if (ctx->shard_world <= 1) return;
    struct Rec {
        uint32_t tab_c, shtab_c, te, reserved, n_powers_lo, n_shifted_lo, world, env_hash;
    } mine;
    mine.tab_c = pk.tab_c;
    mine.shtab_c = pk.shtab_c;
    mine.te = (pk.d_powers_te ? 1u : 0u) | (pk.d_shifted_te ? 2u : 0u);
    mine.reserved = 0;
    mine.n_powers_lo = (uint32_t)pk.n_powers;
    mine.n_shifted_lo = (uint32_t)pk.n_shifted;
    mine.world = ctx->shard_world;
    // every switch that can change a result, the split or the schedule, as this process acts on it (two ranks with different blocks
    // of the block-cyclic split would cover some coefficients twice and others never; ranks that differ in a schedule-only switch
    // were not meant to: refused alike)
    mine.env_hash = switch_fingerprint();
    std::vector<Rec> all(ctx->shard_world);
    rc_check(ctx, shard_exchange(ctx, &mine, sizeof(Rec), all.data()));
    for (unsigned g = 0; g < ctx->shard_world; g++)
        if (memcmp(&all[g], &all[0], sizeof(Rec)) != 0)
            throw MarlinError(SWM_ERR_MISMATCH,
                              "sharded proving: rank " + std::to_string(g) + " and rank 0 disagree on the key's window tables (widths " +
                                  std::to_string(all[g].tab_c) + "/" + std::to_string(all[g].shtab_c) + " vs " + std::to_string(all[0].tab_c) + "/" +
                                  std::to_string(all[0].shtab_c) + ", forms " + std::to_string(all[g].te) + " vs " + std::to_string(all[0].te) +
                                  ") or on the path and sharding switches of switches.h (fingerprint " + std::to_string(all[g].env_hash) + " vs " +
                                  std::to_string(all[0].env_hash) + "): every rank must build its key with the same free memory and the same switches");
}
// asynchronous form: alternates between the two MSM lanes of the context
// With swm_set_msm_sharding active the context only takes its own point range of every MSM and the partial sums are
// exchanged in commit_wait (all-gather of one point per rank + the same rank-ordered sum everywhere).
struct AsyncMsm {
    MsmJob job;
    bool sharded = false;
    bool have_result = false;  // set by commit_gather (the exchange of a whole round) before commit_wait is reached
    G1XYZZ result;
};
// twin_offset / twin_lead (msm.h: MsmTwin): this commitment is followed by one of the SAME coefficients against the powers from
// *twin_offset on / follows the commitment twin_lead of the same coefficients — the degree-shifted commitment of a bounded
// polynomial beside its plain one; the second job then takes the first one's sort.
void commit_enqueue(swm_ctx* ctx, int* lane, const swm_pk& pk, size_t offset, const Fr* coeffs, size_t n, AsyncMsm* out,
                    const size_t* twin_offset = nullptr, AsyncMsm* twin_lead = nullptr) {
    const G1Affine *b = nullptr, *b28 = nullptr;
    MsmTable tab;
    if (n) pk.bases_at(offset, n, &b, &b28, &tab);
    size_t lo = 0, hi = n;
    out->have_result = false;
    out->result = g1_xyzz_identity();  // an empty range (n = 0, or a rank's empty shard) contributes the identity
    const bool force_exchange = sw(SW_SHARD_FORCE) != 0;  // test hook: exchange with a world of one
    out->sharded = ctx->shard_world > 1 || (force_exchange && (ctx->rccl_comm || ctx->shard_allgather));
    // Split of a replicated polynomial's commitment over the ranks (every rank holds all n coefficients):
    //  * CYCLIC (default, table schedule): rank g takes the coefficients g, g + G, ... (strided scalars, table rows g + G j).
    //    Polynomials are zero-padded at the top, so a range split hands the last ranks the zeros and the first ranks the
    //    work (2^20, G = 8: 196 M mixed additions on rank 0, 145 M on rank 7); the cyclic split gives every rank the same;
    //  * by point RANGE (no table, or SWM_SHARD_RANGE=1): the r02 split;
    //  * by BUCKET range (SWM_SHARD_BUCKETS=1, table schedule): all points stay, the digits are filtered; accumulation, sort
    //    AND bucket stage shrink with G.  Measured per rank on one GPU (tools/ubench/shard_emulate.py): it balances two ranks
    //    and loses at eight (1/8 of the buckets at full depth are too few lanes for the accumulation), so it is not the default.
    // (The switches are read per call: tests flip them.)
    const bool by_bucket = sw(SW_SHARD_BUCKETS) != 0;
    const bool by_range = sw(SW_SHARD_RANGE) != 0;
    const bool table_split = out->sharded && ctx->shard_world > 1 && n && msm_flat_applies(tab, n) && tab.contiguous();
    size_t first = 0, count = n;   // scalars coeffs[first + map(i)], i < count (map: the table's block map when the scalars are strided)
    if (table_split && by_bucket) {
        tab.shard_rank = ctx->shard_rank;
        tab.shard_world = ctx->shard_world;
    } else if (table_split && !by_range) {
        // BLOCK-cyclic (r04): rank g takes the blocks g, g + G, ... of 2^L consecutive coefficients (L = 12, less when the
        // polynomial is short: every rank gets at least ~8 blocks; SWM_SHARD_BLOCK_LOG=0 is the plain cyclic split of r03).  As
        // balanced as the cyclic split — the zero padding at the top is spread over the ranks block by block — but a rank's
        // table rows are runs of 2^L x 192 B instead of every G-th row: the accumulation's gathers are sensitive to that
        // (per rank at 2^22 and G = 8: 5.4 G additions/s cyclic, 7 - 8 G/s for contiguous ranges: profiles/r04_shard_emulate.jsonl)
        const size_t G = ctx->shard_world, g = ctx->shard_rank;
        unsigned L = (unsigned)sw(SW_SHARD_BLOCK_LOG);
        while (L > 0 && ((size_t)8 * G << L) > n) L--;
        const size_t B = (size_t)1 << L, nblocks = (n + B - 1) / B;
        const size_t mine = nblocks > g ? (nblocks - g + G - 1) / G : 0;            // blocks g, g + G, ... below nblocks
        const bool owns_last = mine && (g + (mine - 1) * G) == nblocks - 1;
        first = g << L;
        count = mine * B - (owns_last ? nblocks * B - n : 0);                        // the polynomial's last block may be short
        tab.offset += g << L;
        tab.blk_log = L;
        tab.bstride = G << L;
        tab.scalar_stride = G;  // != 1: the scalars follow the same block map as the bases (msm_digits)
        // too few points for the table schedule: fall back to the range.  Decided on floor(n / G), the SMALLEST share, so that
        // every rank takes the same branch (the ranks' own counts differ by one when G does not divide n: one rank cyclic
        // and another by range would leave coefficients uncovered — ADVICE r03)
        if (count && !msm_flat_applies(tab, std::max<size_t>(n / G, 1))) {
            tab = MsmTable();
            pk.bases_at(offset, n, &b, &b28, &tab);
            first = 0;
            count = n;
        }
    }
    if (out->sharded && tab.scalar_stride == 1 && tab.shard_world <= 1) {
        lo = (size_t)(((unsigned __int128)n * ctx->shard_rank) / ctx->shard_world);
        hi = (size_t)(((unsigned __int128)n * (ctx->shard_rank + 1)) / ctx->shard_world);
    }
    // Small MSMs defer their bucket stage to the end of the round, where the stages of all its commitments run as one
    // launch: one chain latency instead of four.  With the flat schedule (a table: one bucket set, <= 64 workgroups per
    // stage below 2^18 points) the four stages of a round are resident together (up to 3 x 2^16 points: the commitments of a 2^16 proof) — measured r02: 2^14 proofs 11.7 -> 9.9 ms,
    // 2^16 17.4 -> 14.7 ms.  Per-window schedule (no table): a single stage fills the chip from ~2^15 points, a joint
    // launch only queues them behind one another (2^16: 16.5 -> 20.3 ms) — those keep their own tail, as do large MSMs,
    // whose tail overlaps the next commitment's accumulation.
    // r05: the joint launch pays up to 10^6 points — the commitments of proofs up to 2^18 constraints and of the Merkle circuit of
    // BASELINE config #5.  At those sizes a proof IS its bucket stages (2^19 buckets per commitment, 3 - 13 entries per bucket:
    // the stage of a job takes as long as its accumulation), and one stage after the other on the tail stream — each a full chip of
    // lone waves — was the critical path; the stages of a round's jobs in ONE launch (64 workgroups each, 32 buckets per lane, all
    // resident together) share one chain latency: 2^18: 19.3 -> 17.1 ms, Merkle circuit 17.5 -> 15.1 ms (profiles/r05_*).
    // (SWM_MSM_BATCH_BELOW: the bound in points, 0 = every job keeps its own bucket stage; tests/test_gpu_switches.py)
    static const long batch_env = sw(SW_MSM_BATCH_BELOW);
    const long batch_below = batch_env >= 0 ? batch_env : (tab.any() ? (tab.te ? 1000000 : 200000) : 32768);
    if (tab.scalar_stride != 1) {
        rc_check(ctx, msm_enqueue(ctx, (*lane)++, b, b28, coeffs + first, count, 1, &out->job, MsmInfMask(),
                                  (long)count <= batch_below, tab));
        return;
    }
    tab.offset += lo;
    MsmTwin tw;
    if (!out->sharded && n) {
        if (twin_offset) {
            const G1Affine *b2 = nullptr, *b282 = nullptr;
            pk.bases_at(*twin_offset, n, &b2, &b282, &tw.tab2);
            tw.role = MsmTwin::LEAD;
        } else if (twin_lead && !twin_lead->sharded) {
            tw.role = MsmTwin::FOLLOW;
            tw.lead = &twin_lead->job;
        }
    }
    rc_check(ctx, msm_enqueue(ctx, (*lane)++, b + lo, b28 + lo, coeffs + lo, hi - lo, 1, &out->job, MsmInfMask(),
                              (long)(hi - lo) <= batch_below, tab, tw));
    if (out->job.twin_kept_lane) (*lane)--;  // a follower leaves its lane's scratch set to the next job
}
// The same for coefficients that are ALREADY distributed: this rank holds coefficient rank + G j at local[j] (the CYCLIC
// layout a sharded inverse transform leaves, ntt.hip) and commits to them where they are — the table rows of its scalars
// are rank, rank + G, ... (MsmTable::blk_log = 0, bstride = G).  The partial sums are exchanged like those of a range split.
bool commit_cyclic_possible(swm_ctx* ctx, const swm_pk& pk, size_t n_local) {
    const G1Affine *b, *b28;
    MsmTable tab;
    pk.bases_at(0, 1, &b, &b28, &tab);
    return msm_flat_applies(tab, n_local);
}
void commit_enqueue_cyclic(swm_ctx* ctx, int* lane, const swm_pk& pk, const Fr* local, size_t n_local, AsyncMsm* out) {
    const unsigned G = ctx->shard_world, rank = ctx->shard_rank;
    const G1Affine *b = nullptr, *b28 = nullptr;
    MsmTable tab;
    out->have_result = false;
    out->result = g1_xyzz_identity();
    out->sharded = true;
    if (!n_local) return;
    pk.bases_at(0, rank + (size_t)G * (n_local - 1) + 1, &b, &b28, &tab);  // the highest power this rank touches must exist
    tab.offset += rank;
    tab.blk_log = 0;
    tab.bstride = G;
    static const long batch_env = sw(SW_MSM_BATCH_BELOW);
    const long batch_below = batch_env >= 0 ? batch_env : 200000;
    rc_check(ctx, msm_enqueue(ctx, (*lane)++, b, b28, local, n_local, 1, &out->job, MsmInfMask(),
                              (long)n_local <= batch_below, tab));
}
// every commitment of a round is enqueued: run their bucket stages together
void commit_flush(swm_ctx* ctx) { rc_check(ctx, msm_flush_tails(ctx)); }
// Sum of the per-rank partial sums in rank order: the same group element on every rank.
static G1XYZZ fold_ranks(const G1XYZZ* all, unsigned world) {
    G1XYZZ r = all[0];
    for (unsigned g = 1; g < world; g++) g1_add(r, all[g]);
    return r;
}
// All commitments of a round at once (sharded proving only): wait for every job, then ONE all-gather of k partial sums
// per rank (k x 192 bytes) instead of one exchange per commitment; commit_wait then finds the folded results.
void commit_gather(swm_ctx* ctx, std::initializer_list<AsyncMsm*> jobs) {
    // every job of the round is awaited once and the host folds run side by side (msm_finish_many)
    std::vector<AsyncMsm*> todo;
    for (AsyncMsm* a : jobs)
        if (a && !a->have_result && a->job.active) todo.push_back(a);
    if (!todo.empty()) {
        std::vector<MsmJob*> mj(todo.size());
        std::vector<G1XYZZ> res(todo.size());
        for (size_t i = 0; i < todo.size(); i++) mj[i] = &todo[i]->job;
        rc_check(ctx, msm_finish_many(ctx, mj.data(), (int)mj.size(), res.data()));
        for (size_t i = 0; i < todo.size(); i++) {
            todo[i]->result = res[i];
            todo[i]->have_result = !todo[i]->sharded;  // a sharded job's sum is still this rank's part
        }
    }
    std::vector<AsyncMsm*> sh;
    for (AsyncMsm* a : jobs)
        if (a && a->sharded && !a->have_result) sh.push_back(a);
    if (sh.empty()) return;
    const unsigned world = ctx->shard_world;
    const size_t k = sh.size();
    std::vector<G1XYZZ> mine(k), all(k * world);
    for (size_t i = 0; i < k; i++) {
        if (sh[i]->job.active) rc_check(ctx, msm_finish(ctx, &sh[i]->job, &mine[i]));
        else mine[i] = sh[i]->result;
    }
    rc_check(ctx, shard_exchange(ctx, mine.data(), k * sizeof(G1XYZZ), all.data()));
    for (size_t i = 0; i < k; i++) {
        std::vector<G1XYZZ> col(world);
        for (unsigned g = 0; g < world; g++) col[g] = all[(size_t)g * k + i];
        sh[i]->result = fold_ranks(col.data(), world);
        sh[i]->have_result = true;
    }
}
G1XYZZ commit_wait(swm_ctx* ctx, AsyncMsm* a) {
    if (a->have_result) return a->result;
    G1XYZZ r;
    rc_check(ctx, msm_finish(ctx, &a->job, &r));
    if (a->sharded) {
        std::vector<G1XYZZ> all(ctx->shard_world);
        rc_check(ctx, shard_exchange(ctx, &r, sizeof(G1XYZZ), all.data()));
        r = fold_ranks(all.data(), ctx->shard_world);
    }
    return r;
}

struct PolyRand {
    HPoly rand, shifted_rand;
    bool has_shifted = false;
};

// MarlinKZG10::commit for one labelled polynomial resident in HBM, split in two halves so that the MSMs of a round
// run back to back on the GPU while the host is still enqueueing:
//   pc_commit_begin  enqueues the plain (and, with a degree bound, the shifted) MSM;
//   pc_commit_end    waits, draws the blinding polynomials (plain first, then shifted — the arkworks draw order, so
//                    pc_commit_end must be called in label order) and adds the hiding terms.
struct CommitJob {
    AsyncMsm plain, shifted;
    bool has_bound = false, hiding = false;
    bool blinded = false;  // pc_commit_blind has drawn the blinding polynomials and computed the hiding terms
    G1XYZZ blind_plain, blind_shifted;
    // a commitment computed in pieces (the mask polynomial of a caller-owned generator, prove_impl): `plain` is the first piece,
    // the rest has been summed into `extra`
    bool has_extra = false;
    G1XYZZ extra;
};
// (the first commitment of a round as two MSMs, so that only a small head's sort runs with no accumulation in flight: measured
// in r05 — 50.0 -> 52.3 ... 55.0 ms at 2^20 — and removed in r06)
void pc_commit_begin(swm_ctx* ctx, const swm_pk& pk, int* lane, const Fr* coeffs, size_t n, bool has_bound, uint64_t bound,
                     bool hiding, CommitJob* job) {
    job->has_bound = has_bound;
    job->hiding = hiding;
    const size_t shift = has_bound ? pk.srs_max_degree - bound : 0;
    commit_enqueue(ctx, lane, pk, 0, coeffs, n, &job->plain, has_bound ? &shift : nullptr);
    if (has_bound) commit_enqueue(ctx, lane, pk, shift, coeffs, n, &job->shifted, nullptr, &job->plain);
}
// The blinding half of pc_commit_end: the draws (plain first, then shifted) and the hiding terms sum_j r_j gamma^j G —
// host work (~70 us per term) that depends on the generator only, not on the MSM: the prover calls it for the round's
// polynomials in label order while their MSMs are still running.
void pc_commit_blind(const swm_pk& pk, CommitJob* job, ChaChaRng* rng, PolyRand* pr) {
    pr->rand.clear();
    pr->shifted_rand.clear();
    pr->has_shifted = job->has_bound;
    job->blind_plain = job->blind_shifted = g1_xyzz_identity();
    if (job->hiding) {
        for (int i = 0; i < 3; i++) pr->rand.push_back(rng->rand_fr());  // DensePolynomial::rand(hiding_bound + 1)
        job->blind_plain = gamma_msm(pk, pr->rand);
        if (job->has_bound) {
            for (int i = 0; i < 3; i++) pr->shifted_rand.push_back(rng->rand_fr());
            job->blind_shifted = gamma_msm(pk, pr->shifted_rand);
        }
    }
    job->blinded = true;
}
// XYZZ -> affine for several points with ONE field inversion (Montgomery's trick over the products ZZ * ZZZ): the
// commitments of a round are normalised together, between its last kernel and the Fiat-Shamir challenge.
void g1_to_affine_batch(const G1XYZZ* in, int k, G1Affine* out) {
    std::vector<Fq> pref((size_t)k + 1);
    pref[0] = fp_one<Fq>();
    for (int i = 0; i < k; i++) pref[i + 1] = g1_is_inf(in[i]) ? pref[i] : fp_mul(pref[i], fp_mul(in[i].zz, in[i].zzz));
    Fq inv = fp_inv(pref[k]);
    for (int i = k; i-- > 0;) {
        if (g1_is_inf(in[i])) {
            out[i] = g1_affine_identity();
            continue;
        }
        Fq zi = fp_mul(inv, pref[i]);  // 1 / (ZZ_i ZZZ_i)
        inv = fp_mul(inv, fp_mul(in[i].zz, in[i].zzz));
        out[i].x = fp_mul(in[i].x, fp_mul(zi, in[i].zzz));
        out[i].y = fp_mul(in[i].y, fp_mul(zi, in[i].zz));
    }
}
// Waits for the commitments of a round (label order; pc_commit_blind already called or called here) and normalises them
// together.
void pc_commit_end_round(swm_ctx* ctx, const swm_pk& pk, std::initializer_list<CommitJob*> jobs,
                         std::initializer_list<ChaChaRng*> rngs, std::initializer_list<PolyRand*> prs, Commitment* out) {
    std::vector<G1XYZZ> pts;
    std::vector<std::pair<int, bool>> where;  // (commitment index, shifted?)
    auto rng = rngs.begin();
    auto pr = prs.begin();
    int idx = 0;
    for (CommitJob* job : jobs) {
        if (!job->blinded) pc_commit_blind(pk, job, *rng, *pr);
        G1XYZZ plain = commit_wait(ctx, &job->plain);
        if (job->has_extra) g1_add(plain, job->extra);
        if (job->hiding) g1_add(plain, job->blind_plain);
        pts.push_back(plain);
        where.push_back({idx, false});
        out[idx] = Commitment();
        if (job->has_bound) {
            G1XYZZ sh = commit_wait(ctx, &job->shifted);
            if (job->hiding) g1_add(sh, job->blind_shifted);
            pts.push_back(sh);
            where.push_back({idx, true});
            out[idx].has_shifted = true;
        }
        ++rng;
        ++pr;
        ++idx;
    }
    std::vector<G1Affine> aff(pts.size());
    g1_to_affine_batch(pts.data(), (int)pts.size(), aff.data());
    for (size_t i = 0; i < pts.size(); i++) {
        if (where[i].second) out[where[i].first].shifted = aff[i];
        else out[where[i].first].comm = aff[i];
    }
}

// ================================================================================================ setup
__global__ void __launch_bounds__(256) srs_fixed_base(const G1Affine* __restrict__ table, PowTable beta_pows, size_t n,
                                                      G1XYZZ* __restrict__ out) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr s = fp_to_std(beta_pows.at(i));
    G1XYZZ acc = g1_xyzz_identity();
    for (int k = 0; k < 32; k++) {
        unsigned d = (s.v[k >> 2] >> ((k & 3) * 8)) & 255;
        if (d) g1_add_mixed(acc, table[k * 255 + (d - 1)]);
    }
    out[i] = acc;
}
G1Affine g1_rand(ChaChaRng& rng) {
    static const uint32_t cof[4] = SWM_G1_COFACTOR;
    for (;;) {
        Fq x = rng.rand_fq();
        bool greatest = rng.gen_bool();
        Fq y;
        if (!fq_sqrt(fp_add(fp_mul(fp_sqr(x), x), fp_one<Fq>()), &y)) continue;
        Fq ny = fp_neg(y);
        bool y_lt = fp_cmp(y, ny) < 0;
        G1Affine p;
        p.x = x;
        p.y = (y_lt != greatest) ? y : ny;  // ark: if (y < negy) ^ greatest { y } else { negy }
        return g1_to_affine(g1_mul_limbs(p, cof, 4));
    }
}
G2Affine g2_rand(ChaChaRng& rng) {
    static const uint32_t cof[SWM_G2_COFACTOR_LIMBS] = SWM_G2_COFACTOR;
    for (;;) {
        Fq2 x;
        x.c0 = rng.rand_fq();
        x.c1 = rng.rand_fq();
        bool greatest = rng.gen_bool();
        Fq2 y;
        if (!fq2_sqrt(x.square() * x + g2_coeff_b(), &y)) continue;
        Fq2 ny = -y;
        bool y_lt = fq2_less(y, ny);
        G2Affine p{x, (y_lt != greatest) ? y : ny, false};
        return g2_mul(p, cof, SWM_G2_COFACTOR_LIMBS);
    }
}

// two-level power tables of an arbitrary base on the device (lo: 1024 entries, hi: count/1024 + 1)
struct OwnedPowTable {
    DVec lo, hi;
    PowTable view() const { return PowTable{lo.p, hi.p}; }
};
OwnedPowTable make_pow_table(swm_ctx* ctx, const Fr& base, size_t max_exp) {
    std::vector<Fr> lo(1024), hi((max_exp >> 10) + 2);
    Fr cur = fp_one<Fr>();
    for (auto& v : lo) {
        v = cur;
        cur = fp_mul(cur, base);
    }
    Fr b1024 = cur;  // base^1024
    cur = fp_one<Fr>();
    for (auto& v : hi) {
        v = cur;
        cur = fp_mul(cur, b1024);
    }
    OwnedPowTable t;
    t.lo = DVec(ctx, lo.size());
    t.lo.upload(lo.data(), lo.size());
    t.hi = DVec(ctx, hi.size());
    t.hi.upload(hi.data(), hi.size());
    return t;
}

swm_srs* universal_setup(swm_ctx* ctx, size_t nc, size_t nv, size_t nnz, ChaChaRng& rng) {
    uint64_t max_degree = ahp_max_degree(nc, nv, nnz);
    if (max_degree < 1) throw MarlinError(SWM_ERR_INVALID_ARG, "DegreeIsZero");
    // KZG10::setup draw order: beta, g, gamma_g, h
    Fr beta = rng.rand_fr();
    G1Affine g = g1_rand(rng);
    G1Affine gamma_g = g1_rand(rng);
    G2Affine h = g2_rand(rng);
    std::unique_ptr<swm_srs> srs(new swm_srs());
    srs->max_degree = max_degree;
    srs->in_subgroup = true;  // multiples of g, which g1_rand returns with the cofactor cleared
    srs->h = h;
    srs->beta_h = g2_mul_fr(h, beta);
    Fr bp = fp_one<Fr>();
    for (int i = 0; i < 3; i++) {
        srs->gamma_powers.push_back(g1_mul_fr(gamma_g, bp));
        bp = fp_mul(bp, beta);
    }
    // fixed-base table of g: tab[k][d-1] = d * 256^k * g
    std::vector<G1XYZZ> tabx;
    tabx.reserve(32 * 255);
    G1XYZZ base = g1_from_affine(g);
    for (int k = 0; k < 32; k++) {
        G1XYZZ acc = base;
        tabx.push_back(acc);
        for (int d = 2; d <= 255; d++) {
            g1_add(acc, base);
            tabx.push_back(acc);
        }
        for (int s = 0; s < 8; s++) base = g1_dbl(base);
    }
    std::vector<G1Affine> tab = batch_normalize(tabx);
    size_t n = max_degree + 1;
    DBuf<G1Affine> d_tab(ctx, tab.size());
    d_tab.upload(tab.data(), tab.size());
    OwnedPowTable bt = make_pow_table(ctx, beta, n);
    DBuf<G1XYZZ> d_x(ctx, n);
    DBuf<Fq> d_pref(ctx, n);
    hip_check(ctx, hipMalloc((void**)&srs->d_powers, n * sizeof(G1Affine)), "hipMalloc(srs)");
    LAUNCHX(ctx, "srs_fixed_base", srs_fixed_base, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d_tab.p, bt.view(),
               n, d_x.p);
    rc_check(ctx, msm_normalize_run(ctx, d_x.p, n, d_pref.p, srs->d_powers));
    hip_check(ctx, hipStreamSynchronize(ctx->stream), "sync");
    return srs.release();
}
G1Affine srs_power(swm_ctx* ctx, const G1Affine* d_powers, size_t i) {
    G1Affine p;
    hip_check(ctx, hipMemcpyAsync(&p, d_powers + i, sizeof(p), hipMemcpyDeviceToHost, ctx->stream), "d2h");
    hip_check(ctx, hipStreamSynchronize(ctx->stream), "sync");
    return p;
}

// ================================================================================================ indexer
// ark-marlin 0.3.0 arithmetize_matrix for M* (transpose, scaled by 1/u_H(col, col)) — SURVEY.md A.7 "Indexer".
// entry k of the row-major, column-sorted matrix: row_vec[k] = w^reindex(col), col_vec[k] = w^row,
// val_vec[k] = val * row_vec[k] / |H|; padding (h0, h0, 0).
__device__ __forceinline__ uint64_t reindex_by_subdomain(uint64_t H, uint64_t X, uint64_t index) {
    uint64_t period = H / X;
    if (index < X) return index * period;
    uint64_t i = index - X, x = period - 1;
    return i + (i / x) + 1;
}

void arithmetize(swm_ctx* ctx, swm_pk& pk, const HostCsr& m, MatrixArith& ar) {
    const uint64_t K = pk.K, H = pk.H, X = pk.X;
    std::vector<uint32_t> rows(m.nnz());
    for (size_t r = 0; r < m.rows(); r++)
        for (uint32_t k = m.rowptr[r]; k < m.rowptr[r + 1]; k++) rows[k] = (uint32_t)r;
    DBuf<uint32_t> d_rows(ctx, std::max<size_t>(m.nnz(), 1)), d_cols(ctx, std::max<size_t>(m.nnz(), 1));
    DVec d_vals(ctx, std::max<size_t>(m.nnz(), 1));
    if (m.nnz()) {
        d_rows.upload(rows.data(), m.nnz());
        d_cols.upload(m.col.data(), m.nnz());
        d_vals.upload(m.val.data(), m.nnz());
    }
    ar.row_K = DVec(ctx, K);
    ar.col_K = DVec(ctx, K);
    ar.val_K = DVec(ctx, K);
    DVec rc_K(ctx, K);
    PowTable wt = root_pow_table(ctx, pk.logH);
    Fr h_inv = HDomain(H).size_inv;
    size_t nnz = m.nnz();
    Fr *prow = ar.row_K.p, *pcol = ar.col_K.p, *pval = ar.val_K.p, *prc = rc_K.p;
    const uint32_t *drows = d_rows.p, *dcols = d_cols.p;
    const Fr* dvals = d_vals.p;
    ew(ctx, "index_arith", K, [=] __device__(size_t k) {
        Fr rv, cv, vv;
        if (k < nnz) {
            rv = wt.at(reindex_by_subdomain(H, X, dcols[k]));
            cv = wt.at(drows[k]);
            vv = fp_mul(fp_mul(dvals[k], rv), h_inv);
        } else {
            rv = fp_one<Fr>();
            cv = fp_one<Fr>();
            vv = fp_zero<Fr>();
        }
        prow[k] = rv;
        pcol[k] = cv;
        pval[k] = vv;
        prc[k] = fp_mul(rv, cv);
    });
    auto interp = [&](const DVec& evals) {
        return dv_ntt_from(ctx, evals.p, K, pk.logK, true);
    };
    ar.row = interp(ar.row_K);
    ar.col = interp(ar.col_K);
    ar.val = interp(ar.val_K);
    ar.row_col = interp(rc_K);
    auto on_b = [&](const DVec& coeffs) {
        return dv_ntt_from(ctx, coeffs.p, K, pk.logB, false);
    };
    ar.row_B = on_b(ar.row);
    ar.col_B = on_b(ar.col);
    ar.val_B = on_b(ar.val);
    ar.row_col_B = on_b(ar.row_col);
}

// Copies the two power ranges of a trimmed committer key into the key (device or host source) and derives the scaled twins.
void install_committer_key(swm_ctx* ctx, swm_pk& pk, const G1Affine* powers, size_t n_powers, const G1Affine* shifted,
                           size_t n_shifted, bool device_src, bool in_subgroup) {
    const hipMemcpyKind kind = device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    pk.n_powers = n_powers;
    pk.n_shifted = n_shifted;
    pk.shift_base = pk.srs_max_degree + 1 - n_shifted;
    hip_check(ctx, hipMalloc((void**)&pk.d_powers, n_powers * sizeof(G1Affine)), "hipMalloc(pk powers)");
    hip_check(ctx, hipMalloc((void**)&pk.d_shifted, std::max<size_t>(n_shifted, 1) * sizeof(G1Affine)), "hipMalloc(pk shifted)");
    hip_check(ctx, hipMemcpyAsync(pk.d_powers, powers, n_powers * sizeof(G1Affine), kind, ctx->stream), "copy powers");
    if (n_shifted) hip_check(ctx, hipMemcpyAsync(pk.d_shifted, shifted, n_shifted * sizeof(G1Affine), kind, ctx->stream), "copy shifted");
    // scaled twins and — for keys large enough to profit — the tables of window multiples (twisted Edwards rows when the
    // points are known to lie in the prime-order subgroup: SRS powers generated here are multiples of the generator,
    // deserialised keys went through the checks of their codec, an imported SRS is checked at import)
    rc_check(ctx, msm_install_bases(ctx, pk.d_powers, n_powers, in_subgroup, &pk.d_powers28, &pk.d_powers_te, &pk.tab_c));
    // (narrower tables over prefixes of the powers for the |H|-size commitments of mid-size keys: measured in r05 — 2^18 17.4 ->
    // 17.6 ms, Merkle circuit 14.9 -> 17.4 ms: the widest bucket set IS the low-latency choice for jobs that do not fill the
    // chip, CHANGELOG.md — and removed in r06)
    // With an SRS of exactly the key's degree (srs_max_degree + 1 == n_powers: what generate_universal_srs(n, n, n) of the tests,
    // the bench and the reference's own examples gives) the shifted powers are the TOP of the powers themselves, and bases_at serves
    // every shifted range from the powers' table: a scaled copy and a table of their own would never be read (r06: 2.1 GB of HBM and
    // a table build per 2^20-constraint key).  The affine copy stays: it is what the key's serialisation writes.
    const bool shifted_inside = pk.shift_base + n_shifted <= n_powers;
    if (n_shifted && !shifted_inside) {
        rc_check(ctx, msm_install_bases(ctx, pk.d_shifted, n_shifted, in_subgroup, &pk.d_shifted28, &pk.d_shifted_te, &pk.shtab_c));
    } else {
        hip_check(ctx, hipMalloc((void**)&pk.d_shifted28, sizeof(G1Affine)), "hipMalloc(pk shifted28)");
    }
    hip_check(ctx, hipStreamSynchronize(ctx->stream), "sync");
}

// A finished key leaves the context that built it: everything that context still has in flight for it is awaited (another
// context's streams are not ordered behind this one's), and its blocks stop belonging to this context's pool.
void pk_publish(swm_ctx* ctx, swm_pk& pk) {
    drain_streams(ctx);
    pk.device = ctx->device;
    pk.own_blocks();
}

void index_impl(swm_ctx* ctx, const swm_srs* srs, const swm_r1cs* cs, swm_pk** out_pk, swm_vk** out_vk) {
    PaddedR1cs p = pad_and_square(cs);
    std::unique_ptr<swm_pk> pk(new swm_pk());
    size_t nnz = std::max(p.a.nnz(), std::max(p.b.nnz(), p.c.nnz()));
    // |K| = 1 has no degree bound |K| - 2 (ark-marlin underflows there as well): refused before anything touches the device
    if (nnz < 2)
        throw MarlinError(SWM_ERR_INVALID_ARG, "index: |K| < 2: the densest of A, B, C needs at least two non-zero entries");
    balance_matrices(p.a, p.b);
    pk->info.num_constraints = p.ncons;
    pk->info.num_variables = p.inst.size() + p.wit.size();
    pk->info.num_non_zero = nnz;
    pk->info.num_instance_variables = p.inst.size();
    if (pk->info.num_constraints != pk->info.num_variables) throw MarlinError(SWM_ERR_INTERNAL, "NonSquareMatrix");
    HDomain dh(p.ncons), dk(nnz), dx(p.inst.size());
    HDomain db(3 * dk.size - 3);
    pk->H = dh.size; pk->logH = dh.log;
    pk->K = dk.size; pk->logK = dk.log;
    pk->X = dx.size; pk->logX = dx.log;
    pk->B = db.size; pk->logB = db.log;
    if (pk->X >= pk->H) throw MarlinError(SWM_ERR_INVALID_ARG, "index: the circuit needs at least one witness variable");
    uint64_t max_deg = ahp_max_degree(p.ncons, pk->info.num_variables, nnz);
    if (srs->max_degree < max_deg) throw MarlinError(SWM_ERR_INDEX_TOO_LARGE, "IndexTooLarge");
    // committer key = MarlinKZG10::trim(srs, supported_degree = max_deg, hiding bound 1, bounds {|H| - 2, |K| - 2})
    pk->srs_max_degree = srs->max_degree;
    install_committer_key(ctx, *pk, srs->d_powers, max_deg + 1, srs->d_powers + (srs->max_degree - (std::max(pk->H, pk->K) - 2)),
                          std::max(pk->H, pk->K) - 2 + 1, /*device_src=*/true, srs->in_subgroup);
    pk->gamma_powers = srs->gamma_powers;
    pk->gtab = build_gamma_table(pk->gamma_powers);
    pk->ha = p.a; pk->hb = p.b; pk->hc = p.c;
    pk->a = upload_csr(ctx, p.a);
    pk->b = upload_csr(ctx, p.b);
    pk->c = upload_csr(ctx, p.c);
    size_t ncols = pk->info.num_variables;
    pk->at = upload_csr(ctx, transpose(p.a, ncols));
    pk->bt = upload_csr(ctx, transpose(p.b, ncols));
    pk->ct = upload_csr(ctx, transpose(p.c, ncols));
    const HostCsr* hm[3] = {&p.a, &p.b, &p.c};
    for (int i = 0; i < 3; i++) arithmetize(ctx, *pk, *hm[i], pk->ar[i]);
    // verifier key
    VerifyingKey& vk = pk->vk;
    vk.info = pk->info;
    vk.vk.g = srs_power(ctx, srs->d_powers, 0);
    vk.vk.gamma_g = pk->gamma_powers[0];
    vk.vk.h = srs->h;
    vk.vk.beta_h = srs->beta_h;
    std::vector<uint64_t> bounds = {pk->H - 2, pk->K - 2};
    std::sort(bounds.begin(), bounds.end());
    bounds.erase(std::unique(bounds.begin(), bounds.end()), bounds.end());
    for (auto d : bounds) vk.vk.degree_bounds_and_shift_powers.push_back({d, srs_power(ctx, srs->d_powers, srs->max_degree - d)});
    vk.vk.max_degree = srs->max_degree;
    vk.vk.supported_degree = max_deg;
    // commit the 12 index polynomials (no hiding, no degree bounds)
    shard_agree(ctx, *pk);
    int lane = 0;
    for (int i = 0; i < 3; i++) {
        const DVec* polys[4] = {&pk->ar[i].row, &pk->ar[i].col, &pk->ar[i].val, &pk->ar[i].row_col};
        AsyncMsm jobs[4];
        for (int j = 0; j < 4; j++) commit_enqueue(ctx, &lane, *pk, 0, polys[j]->p, pk->K, &jobs[j]);
        commit_flush(ctx);
        commit_gather(ctx, {&jobs[0], &jobs[1], &jobs[2], &jobs[3]});
        for (int j = 0; j < 4; j++) {
            Commitment c;
            c.comm = g1_to_affine(commit_wait(ctx, &jobs[j]));
            vk.index_comms.push_back(c);
        }
    }
    std::unique_ptr<swm_vk> v(new swm_vk());
    v->vk = vk;
    pk_publish(ctx, *pk);
    *out_pk = pk.release();
    *out_vk = v.release();
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
// instead of a 4|H|-point one) and the way back is ntt_cosets_inv plus cosets3_solve.  -DSWM_OUTER_COSETS=0 builds the 4|H| path.
#ifndef SWM_OUTER_COSETS
#define SWM_OUTER_COSETS 1
#endif
static constexpr uint64_t OUTER_COSETS_MIN_H = 16;
// u_k = p0 + c^k p1 + c^2k p2 (k = 0, 1, 2; c = w_4, c^2 = -1; what ntt_cosets_inv leaves) -> the three blocks p0, p1, p2
struct Cosets3 {
    Fr p0, p1, p2;
};
__device__ __forceinline__ Cosets3 cosets3_solve(const Fr& u0, const Fr& u1, const Fr& u2, const Fr& iota, const Fr& half) {
    const Fr p1 = fp_mul(fp_sub(u0, u2), half);
    const Fr e = fp_mul(fp_add(u0, u2), half);  // p0 + p2
    const Fr d = fp_sub(u1, fp_mul(iota, p1));  // p0 - p2
    return {fp_mul(fp_add(e, d), half), p1, fp_mul(fp_sub(e, d), half)};
}
static Fr fr_half() { return fp_inv(fp_from_u64<Fr>(2)); }
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

std::vector<uint8_t> prove_impl(swm_ctx* ctx, const swm_pk& pk, const swm_r1cs* cs, ChaChaRng& zk, bool uncompressed = false) {
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


// ================================================================================================ key (de)serialisation
// serialize_proving_key / deserialize_proving_key (src/marlin/serialization.rs:33-45): the CanonicalSerialize bytes of
// ark_marlin::IndexProverKey<Fr, MarlinKZG10<..>>, field order of ark-marlin / ark-poly-commit / ark-poly 0.3.0's derives
// as recalled [U] (the test suite compares the bytes of small keys with an independent model's):
//   IndexProverKey { index_vk, index_comm_rands: Vec<marlin_pc::Randomness>, index: Index, committer_key }
//   Index { index_info, a, b, c: Matrix = Vec<Vec<(F, usize)>>, a_star_arith, b_star_arith, c_star_arith }
//   MatrixArithmetization { row, col, val, row_col: LabeledPolynomial { label, coeffs, degree_bound, hiding_bound },
//                           evals_on_K { row, col, val }, evals_on_B { row, col, val }, row_col_evals_on_B : Evaluations { evals, domain } }
//   marlin_pc::CommitterKey { powers, shifted_powers: Option<Vec>, powers_of_gamma_g, enforced_degree_bounds: Option<Vec<usize>>, max_degree }
// Bulk data is converted on the GPU (Montgomery -> canonical bytes, affine -> compressed points and back, including the
// curve and subgroup checks CanonicalDeserialize performs).  When a key is loaded, only what defines it is used — the
// matrices, the committer key, the verifying key; everything derived from the matrices (arithmetisation polynomials and
// their evaluation tables) is parsed for shape and then recomputed on the device rather than trusted.
// (FqSqrtConsts and fq_sqrt_dev, the device square root: g1.cuh)
// affine -> ark-serialize compressed form (48 bytes: x little-endian, bit 7 of the last byte = y is the larger root,
// bit 6 = infinity)
__global__ void __launch_bounds__(256) g1_compress_kernel(const G1Affine* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1Affine p = in[i];
    uint32_t w[12];
    if (g1_is_inf(p)) {
        for (int k = 0; k < 12; k++) w[k] = 0;
        w[11] = 0x40000000u;
    } else {
        Fq xs = fp_to_std(p.x), ys = fp_to_std(p.y), ny = fp_to_std(fp_neg(p.y));
        for (int k = 0; k < 12; k++) w[k] = xs.v[k];
        if (fp_cmp_std(ys, ny) > 0) w[11] |= 0x80000000u;
    }
    for (int k = 0; k < 12; k++) out[12 * i + k] = w[k];
}
// compressed -> affine with the checks of CanonicalDeserialize: flags, x < q, on the curve, [r]P = O.  *bad != 0 on failure.
__global__ void __launch_bounds__(256) g1_decompress_kernel(const uint32_t* __restrict__ in, size_t n, G1Affine* __restrict__ out,
                                                            uint32_t* __restrict__ bad) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fq xs;
    for (int k = 0; k < 12; k++) xs.v[k] = in[12 * i + k];
    const uint32_t flags = xs.v[11] >> 30;
    xs.v[11] &= 0x3fffffffu;
    G1Affine r = g1_affine_identity();
    if (flags == 3 || !fq_std_lt_p(xs)) {
        atomicOr(bad, (uint32_t)G1_BAD_ENCODING);
    } else if (!(flags & 1)) {
        r.x = fp_from_std(xs);
        Fq y;
        if (!fq_sqrt_dev(fp_add(fp_mul(fp_sqr(r.x), r.x), fp_one<Fq>()), &y)) {
            atomicOr(bad, (uint32_t)G1_OFF_CURVE);
        } else {
            Fq ny = fp_neg(y);
            bool y_is_larger = fp_cmp_std(fp_to_std(y), fp_to_std(ny)) > 0;
            r.y = (y_is_larger == ((flags & 2) != 0)) ? y : ny;
            if (!g1_in_subgroup_dev(r)) atomicOr(bad, (uint32_t)G1_OFF_SUBGROUP);  // [r]P == O (g1.cuh)
        }
    }
    out[i] = r;
}
// affine -> the serialize_uncompressed form [U: ark-ec 0.3] (ByteWriter::ser_g1 with `uncompressed`): 24 words, x then y in standard
// form, bit 6 of the last byte (bit 30 of word 23) = infinity, the identity as (0, 1).  One lane per point.
// Stores: a lane writes its 96 bytes as six 16-byte stores at a stride of 96 bytes, which no single instruction coalesces.  A
// wave's 64 points are 6144 CONTIGUOUS bytes, though, and its six stores cover them completely within a few instructions, so the
// L2 merges them into whole 128-byte lines before they reach HBM; a transpose through LDS would make each instruction contiguous
// at the price of 24 KB of LDS per workgroup and a barrier that every lane has to reach.  Left out: the kernel runs once per key
// write, moves 96 B per point next to two Montgomery multiplications, and is followed by a device-to-host copy of the same bytes
// over PCIe, which is an order of magnitude slower than either.  (Not measured; tools/pk_load_time.py times the writer as a whole.)
__global__ void __launch_bounds__(256) g1_encode_uncompressed_kernel(const G1Affine* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G1Affine p = in[i];
    uint32_t w[24];
    if (g1_is_inf(p)) {
        for (int k = 0; k < 24; k++) w[k] = 0;
        w[12] = 1;
        w[23] = 0x40000000u;
    } else {
        const Fq xs = fp_to_std(p.x), ys = fp_to_std(p.y);
        for (int k = 0; k < 12; k++) {
            w[k] = xs.v[k];
            w[12 + k] = ys.v[k];
        }
    }
    uint4* o = reinterpret_cast<uint4*>(out + 24 * i);  // 96-byte records in a 16-byte aligned buffer
    for (int k = 0; k < 6; k++) o[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
// the serialize_uncompressed form -> affine.  Both instantiations refuse what Fp / SWFlags refuse in every mode of ark-serialize
// (flags 0xC0, a coordinate >= q: G1_BAD_ENCODING).  Checked = deserialize_uncompressed: y^2 = x^3 + 1 (G1_OFF_CURVE) and [r]P = O
// (G1_OFF_SUBGROUP), no square root.  !Checked = deserialize_unchecked: the coordinates are taken as they are.  *bad collects the
// bits of all lanes (as g1_decompress_kernel); a refused point is written as the identity.  No barrier, no LDS: a lane that meets
// the identity or fails early simply has less to do.  Nothing downstream indexes memory by point data, so an unchecked point that
// is not on the curve can make a proof wrong but not make a kernel fault.
template <bool Checked>
__global__ void __launch_bounds__(256) g1_decode_uncompressed_kernel(const uint32_t* __restrict__ in, size_t n, G1Affine* __restrict__ out,
                                                                     uint32_t* __restrict__ bad) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4* src = reinterpret_cast<const uint4*>(in + 24 * i);
    Fq xs, ys;
    for (int k = 0; k < 3; k++) {
        const uint4 a = src[k], b = src[3 + k];
        xs.v[4 * k] = a.x; xs.v[4 * k + 1] = a.y; xs.v[4 * k + 2] = a.z; xs.v[4 * k + 3] = a.w;
        ys.v[4 * k] = b.x; ys.v[4 * k + 1] = b.y; ys.v[4 * k + 2] = b.z; ys.v[4 * k + 3] = b.w;
    }
    const uint32_t flags = ys.v[11] >> 30;
    ys.v[11] &= 0x3fffffffu;
    G1Affine r = g1_affine_identity();
    if (flags == 3 || !fq_std_lt_p(xs) || !fq_std_lt_p(ys)) {
        atomicOr(bad, (uint32_t)G1_BAD_ENCODING);
    } else if (!(flags & 1)) {  // (flags & 1: infinity; its coordinates were range-checked and are otherwise ignored)
        G1Affine q;
        q.x = fp_from_std(xs);
        q.y = fp_from_std(ys);
        if (!Checked) {
            r = q;
        } else if (!fp_eq(fp_sqr(q.y), fp_add(fp_mul(fp_sqr(q.x), q.x), fp_one<Fq>()))) {
            atomicOr(bad, (uint32_t)G1_OFF_CURVE);
        } else if (!g1_in_subgroup_dev(q)) {
            atomicOr(bad, (uint32_t)G1_OFF_SUBGROUP);
        } else {
            r = q;
        }
    }
    out[i] = r;
}

void put_fr_vec_dev(swm_ctx* ctx, ByteWriter& w, const Fr* d, size_t n) {  // Vec<Fr>: u64 length + canonical bytes
    w.u64(n);
    if (!n) return;
    DVec tmp(ctx, n);
    Fr* t = tmp.p;
    ew(ctx, "ser_to_std", n, [=] __device__(size_t i) { t[i] = fp_to_std(d[i]); });
    size_t at = w.b.size();
    w.b.resize(at + n * sizeof(Fr));
    hip_check(ctx, hipMemcpyAsync(w.b.data() + at, t, n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream), "d2h");
    hip_check(ctx, hipStreamSynchronize(ctx->stream), "sync");
}
void put_domain(ByteWriter& w, const HDomain& d) {  // GeneralEvaluationDomain::Radix2: u8 tag + Radix2EvaluationDomain
    w.u8(0);
    w.u64(d.size);
    uint32_t lg = d.log;
    w.raw(&lg, 4);
    w.fr(d.size_fr);
    w.fr(d.size_inv);
    w.fr(d.gen);
    w.fr(d.gen_inv);
    w.fr(fp_inv(fp_from_u64<Fr>(22)));  // generator_inv = multiplicative_generator^-1
}
void put_g1_vec_dev(swm_ctx* ctx, ByteWriter& w, const G1Affine* d, size_t n) {  // Vec<G1Affine>, in the writer's form
    w.u64(n);
    if (!n) return;
    const size_t words = w.uncompressed ? 24 : 12;
    DBuf<uint32_t> tmp(ctx, n * words);
    if (w.uncompressed)
        LAUNCHX(ctx, "g1_encode_uncompressed", g1_encode_uncompressed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d, n, tmp.p);
    else
        LAUNCHX(ctx, "g1_compress", g1_compress_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d, n, tmp.p);
    size_t at = w.b.size();
    w.b.resize(at + n * words * 4);
    hip_check(ctx, hipMemcpyAsync(w.b.data() + at, tmp.p, n * words * 4, hipMemcpyDeviceToHost, ctx->stream), "d2h");
    hip_check(ctx, hipStreamSynchronize(ctx->stream), "sync");
}
void put_matrix(ByteWriter& w, const HostCsr& m) {
    w.u64(m.rows());
    for (size_t r = 0; r < m.rows(); r++) {
        w.u64(m.rowptr[r + 1] - m.rowptr[r]);
        for (uint32_t k = m.rowptr[r]; k < m.rowptr[r + 1]; k++) {
            w.fr(m.val[k]);
            w.u64(m.col[k]);
        }
    }
}
// trailing zero coefficients are not part of a DensePolynomial
size_t trimmed_len(swm_ctx* ctx, const Fr* d, size_t n) {
    std::vector<Fr> h(n);
    hip_check(ctx, hipMemcpyAsync(h.data(), d, n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream), "d2h");
    hip_check(ctx, hipStreamSynchronize(ctx->stream), "sync");
    while (n && fp_is_zero(h[n - 1])) n--;
    return n;
}

std::vector<uint8_t> pk_serialize(swm_ctx* ctx, const swm_pk& pk, bool uncompressed = false) {
    ByteWriter w;
    w.uncompressed = uncompressed;  // every point below, on the host (gamma powers) and on the device (the two power ranges)
    std::vector<uint8_t> vkb = serialize_verifying_key(pk.vk, uncompressed);
    w.raw(vkb.data(), vkb.size());
    w.u64(pk.vk.index_comms.size());  // index_comm_rands: no hiding -> empty blinding polynomial, no shifted rand
    for (size_t i = 0; i < pk.vk.index_comms.size(); i++) {
        w.u64(0);
        w.u8(0);
    }
    w.u64(pk.info.num_variables);
    w.u64(pk.info.num_constraints);
    w.u64(pk.info.num_non_zero);
    w.u64(pk.info.num_instance_variables);
    put_matrix(w, pk.ha);
    put_matrix(w, pk.hb);
    put_matrix(w, pk.hc);
    HDomain dk(pk.K), db(pk.B);
    for (int m = 0; m < 3; m++) {
        const MatrixArith& ar = pk.ar[m];
        const DVec* polys[4] = {&ar.row, &ar.col, &ar.val, &ar.row_col};
        for (int j = 0; j < 4; j++) {
            const char* label = kIndexerPolys[4 * m + j];
            w.u64(strlen(label));
            w.raw(label, strlen(label));
            put_fr_vec_dev(ctx, w, polys[j]->p, trimmed_len(ctx, polys[j]->p, pk.K));
            w.u8(0);  // degree_bound: None
            w.u8(0);  // hiding_bound: None
        }
        for (const DVec* e : {&ar.row_K, &ar.col_K, &ar.val_K}) {
            put_fr_vec_dev(ctx, w, e->p, pk.K);
            put_domain(w, dk);
        }
        for (const DVec* e : {&ar.row_B, &ar.col_B, &ar.val_B, &ar.row_col_B}) {
            put_fr_vec_dev(ctx, w, e->p, pk.B);
            put_domain(w, db);
        }
    }
    put_g1_vec_dev(ctx, w, pk.d_powers, pk.n_powers);
    w.u8(1);
    put_g1_vec_dev(ctx, w, pk.d_shifted, pk.n_shifted);
    w.u64(pk.gamma_powers.size());
    for (auto& g : pk.gamma_powers) w.ser_g1(g);
    w.u8(1);
    w.u64(pk.vk.vk.degree_bounds_and_shift_powers.size());
    for (auto& ds : pk.vk.vk.degree_bounds_and_shift_powers) w.u64(ds.first);
    w.u64(pk.srs_max_degree);
    return w.b;
}

// Vec<G1Affine> (compressed) -> host affine points, decompressed and checked on the device
std::vector<G1Affine> get_g1_vec_dev(swm_ctx* ctx, ByteReader& r, uint64_t max_n) {
    uint64_t n = r.u64();
    if (n > max_n) throw MarlinError(SWM_ERR_SERIALIZATION, "bad point count");
    std::vector<G1Affine> out(n);
    if (!n) return out;
    const uint8_t* src = r.take(n * 48);
    DBuf<uint32_t> in(ctx, n * 12), bad(ctx, 1);
    DBuf<G1Affine> pts(ctx, n);
    bad.zero();
    hip_check(ctx, hipMemcpyAsync(in.p, src, n * 48, hipMemcpyHostToDevice, ctx->stream), "h2d");
    LAUNCHX(ctx, "g1_decompress", g1_decompress_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, in.p, n, pts.p, bad.p);
    uint32_t b = bad.download(0, 1)[0];
    if (b) throw MarlinError(SWM_ERR_SERIALIZATION, b & 4 ? "committer key: point not in the prime-order subgroup"
                                                        : (b & 2 ? "committer key: x not on the curve" : "committer key: invalid point encoding"));
    hip_check(ctx, hipMemcpyAsync(out.data(), pts.p, n * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->stream), "d2h");
    hip_check(ctx, hipStreamSynchronize(ctx->stream), "sync");
    return out;
}

// Vec<G1Affine> in the serialize_uncompressed form -> affine points that STAY on the device, decoded there (and, when `checked`,
// tested against the curve equation and [r]P = O)
DBuf<G1Affine> get_g1_vec_unc_dev(swm_ctx* ctx, ByteReader& r, uint64_t max_n, bool checked) {
    uint64_t n = r.u64();
    if (n > max_n) throw MarlinError(SWM_ERR_SERIALIZATION, "bad point count");
    if (!n) return DBuf<G1Affine>();
    const uint8_t* src = r.take(n * 96);
    DBuf<uint32_t> in(ctx, n * 24), bad(ctx, 1);
    DBuf<G1Affine> pts(ctx, n);
    bad.zero();
    hip_check(ctx, hipMemcpyAsync(in.p, src, n * 96, hipMemcpyHostToDevice, ctx->stream), "h2d");
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (checked) LAUNCHX(ctx, "g1_decode_uncompressed", g1_decode_uncompressed_kernel<true>, grid, block, 0, in.p, n, pts.p, bad.p);
    else LAUNCHX(ctx, "g1_decode_unchecked", g1_decode_uncompressed_kernel<false>, grid, block, 0, in.p, n, pts.p, bad.p);
    uint32_t b = bad.download(0, 1)[0];  // (synchronises: `in` is no longer read when it goes back to the pool)
    if (b) throw MarlinError(SWM_ERR_SERIALIZATION, b & G1_OFF_SUBGROUP ? "committer key: point not in the prime-order subgroup"
                                                        : (b & G1_OFF_CURVE ? "committer key: point not on the curve" : "committer key: invalid point encoding"));
    return pts;
}

// uncompressed / checked: which of arkworks' three forms the bytes are in (include/swmarlin.h, swm_pk_deserialize_ex).  The
// structural checks, the committer-key / verifying-key comparison and the recomputation of the derived tables are the same in all.
swm_pk* pk_deserialize(swm_ctx* ctx, const uint8_t* bytes, size_t len, bool uncompressed = false, bool checked = true) {
    ByteReader r(bytes, len);
    r.uncompressed = uncompressed;
    r.checked = checked;
    std::unique_ptr<swm_pk> pk(new swm_pk());
    {   // everything in front of the committer key is parsed and checked on the host (host/pk_codec.h: the same text runs under
        // ASan / UBSan in tests/native/host_fuzz.cpp)
        PkPrefix pre = pk_parse_prefix(r);
        pk->vk = std::move(pre.vk);
        pk->info = pre.info;
        pk->ha = std::move(pre.a);
        pk->hb = std::move(pre.b);
        pk->hc = std::move(pre.c);
        pk->H = pre.H; pk->logH = pre.logH;
        pk->K = pre.K; pk->logK = pre.logK;
        pk->X = pre.X; pk->logX = pre.logX;
        pk->B = pre.B; pk->logB = pre.logB;
    }
    // the two power ranges: the compressed form comes back to the host, the uncompressed one stays on the device and only the
    // points the comparison below reads are downloaded
    std::vector<G1Affine> powers, shifted;
    DBuf<G1Affine> d_powers, d_shifted;
    if (uncompressed) {
        d_powers = get_g1_vec_unc_dev(ctx, r, 1ull << 31, checked);
        if (r.boolean()) d_shifted = get_g1_vec_unc_dev(ctx, r, 1ull << 31, checked);
    } else {
        powers = get_g1_vec_dev(ctx, r, 1ull << 31);
        if (r.boolean()) shifted = get_g1_vec_dev(ctx, r, 1ull << 31);
    }
    const size_t n_powers = uncompressed ? d_powers.n : powers.size(), n_shifted = uncompressed ? d_shifted.n : shifted.size();
    auto power_at = [&](size_t i) { return uncompressed ? d_powers.download(i, 1)[0] : powers[i]; };
    auto shifted_at = [&](size_t i) { return uncompressed ? d_shifted.download(i, 1)[0] : shifted[i]; };
    uint64_t ng = r.u64();
    if (ng > 16) throw MarlinError(SWM_ERR_SERIALIZATION, "bad gamma count");
    for (uint64_t i = 0; i < ng; i++) pk->gamma_powers.push_back(r.g1());
    std::vector<uint64_t> bounds;
    if (r.boolean()) {
        uint64_t nb = r.u64();
        if (nb > 64) throw MarlinError(SWM_ERR_SERIALIZATION, "bad degree-bound count");
        for (uint64_t i = 0; i < nb; i++) bounds.push_back(r.u64());
    }
    pk->srs_max_degree = r.u64();
    if (r.pos != len) throw MarlinError(SWM_ERR_SERIALIZATION, "trailing bytes");
    const uint64_t max_bound = std::max(pk->H, pk->K) - 2;
    if (n_powers < ahp_max_degree(pk->info.num_constraints, pk->info.num_variables, pk->info.num_non_zero) + 1 ||
        n_powers > pk->srs_max_degree + 1 || n_shifted != max_bound + 1 || pk->gamma_powers.size() < 3 ||
        pk->srs_max_degree != pk->vk.vk.max_degree)
        throw MarlinError(SWM_ERR_SERIALIZATION, "committer key does not fit the index");
    {   // the committer key has to be the one the embedded verifying key was trimmed from: a key whose halves disagree would
        // load and then produce proofs that never verify.  enforced_degree_bounds = {|H| - 2, |K| - 2}; powers[0] = g; the
        // shift power of bound d is [beta^(max_degree - d)] g = shifted[max_bound - d].
        auto same = [](const G1Affine& a, const G1Affine& b) { return fp_eq(a.x, b.x) && fp_eq(a.y, b.y); };
        std::vector<uint64_t> want = {pk->H - 2, pk->K - 2};
        std::sort(want.begin(), want.end());
        want.erase(std::unique(want.begin(), want.end()), want.end());
        const auto& dbs = pk->vk.vk.degree_bounds_and_shift_powers;
        bool ok = bounds == want && dbs.size() == want.size() && same(power_at(0), pk->vk.vk.g) &&
                  same(pk->gamma_powers[0], pk->vk.vk.gamma_g);
        for (size_t i = 0; ok && i < dbs.size(); i++)
            ok = dbs[i].first == want[i] && same(shifted_at(max_bound - dbs[i].first), dbs[i].second);
        if (!ok) throw MarlinError(SWM_ERR_SERIALIZATION, "committer key and verifying key of the proving key disagree");
    }
    // in_subgroup: the checked readers' kernels tested [r]P = O for every point; for an unchecked key it is the caller's
    // assertion (include/swmarlin.h) — the twisted Edwards tables built on it compute wrong sums for other points, nothing worse
    if (uncompressed)
        install_committer_key(ctx, *pk, d_powers.p, n_powers, d_shifted.p, n_shifted, /*device_src=*/true, /*in_subgroup=*/true);
    else
        install_committer_key(ctx, *pk, powers.data(), n_powers, shifted.data(), n_shifted, /*device_src=*/false, /*in_subgroup=*/true);
    pk->gtab = build_gamma_table(pk->gamma_powers);
    pk->a = upload_csr(ctx, pk->ha);
    pk->b = upload_csr(ctx, pk->hb);
    pk->c = upload_csr(ctx, pk->hc);
    size_t ncols = pk->info.num_variables;
    pk->at = upload_csr(ctx, transpose(pk->ha, ncols));
    pk->bt = upload_csr(ctx, transpose(pk->hb, ncols));
    pk->ct = upload_csr(ctx, transpose(pk->hc, ncols));
    const HostCsr* hm[3] = {&pk->ha, &pk->hb, &pk->hc};
    for (int i = 0; i < 3; i++) arithmetize(ctx, *pk, *hm[i], pk->ar[i]);
    pk_publish(ctx, *pk);
    return pk.release();
}

// ================================================================================================ is_satisfied (K3)
void is_satisfied_impl(swm_ctx* ctx, const swm_r1cs* cs, int* ok, size_t* first_bad) {
    if (!cs || cs->num_instance == 0) throw MarlinError(SWM_ERR_INVALID_ARG, "r1cs: bad arguments");
    size_t ninst = cs->num_instance, nwit = cs->num_witness, rows = cs->num_constraints, nv = ninst + nwit;
    HostCsr a = import_csr(cs->a_rowptr, cs->a_col, cs->a_val, rows, ninst, 0, nv);
    HostCsr b = import_csr(cs->b_rowptr, cs->b_col, cs->b_val, rows, ninst, 0, nv);
    HostCsr c = import_csr(cs->c_rowptr, cs->c_col, cs->c_val, rows, ninst, 0, nv);
    DevCsr da = upload_csr(ctx, a), db = upload_csr(ctx, b), dc = upload_csr(ctx, c);
    DVec z(ctx, nv);
    hip_check(ctx, hipMemcpyAsync(z.p, cs->instance, ninst * 32, hipMemcpyHostToDevice, ctx->stream), "h2d");
    if (nwit) hip_check(ctx, hipMemcpyAsync(z.p + ninst, cs->witness, nwit * 32, hipMemcpyHostToDevice, ctx->stream), "h2d");
    DVec za(ctx, std::max<size_t>(rows, 1)), zb(ctx, std::max<size_t>(rows, 1)), zc(ctx, std::max<size_t>(rows, 1));
    rc_check(ctx, spmv_run(ctx, da.rowptr.p, da.col.p, da.val.p, z.p, za.p, rows, &da.plan));
    rc_check(ctx, spmv_run(ctx, db.rowptr.p, db.col.p, db.val.p, z.p, zb.p, rows, &db.plan));
    rc_check(ctx, spmv_run(ctx, dc.rowptr.p, dc.col.p, dc.val.p, z.p, zc.p, rows, &dc.plan));
    DBuf<unsigned long long> bad(ctx, 1);
    unsigned long long init = ~0ull;
    bad.upload(&init, 1);
    const Fr *pa = za.p, *pb = zb.p, *pc = zc.p;
    unsigned long long* pbad = bad.p;
    ew(ctx, "r1cs_check", rows, [=] __device__(size_t i) {
        if (!fp_eq(fp_mul(pa[i], pb[i]), pc[i])) atomicMin(pbad, (unsigned long long)i);
    });
    unsigned long long res = bad.download(0, 1)[0];
    *ok = res == ~0ull ? 1 : 0;
    if (first_bad) *first_bad = res == ~0ull ? 0 : (size_t)res;
}

}  // namespace

// witness_host.h: prove_shape's comparison from the counts alone, for a unit that changes state before it calls the prover
namespace swm {
bool pk_takes_shape(const swm_pk* pk, size_t num_instance, size_t num_witness, size_t num_constraints) {
    const size_t inst = HDomain(num_instance).size, nv = inst + num_witness, side = nv > num_constraints ? nv : num_constraints;
    return side == pk->info.num_constraints && side == pk->info.num_variables && inst == pk->info.num_instance_variables;
}
}  // namespace swm

// ================================================================================================ C ABI
#include "host/host_abi.inc"  // SWM_GUARD + every entry point that needs no GPU (rng, verifier, proof / vk codecs, hashes)

extern "C" {

int swm_generate_universal_srs(swm_ctx* ctx, size_t nc, size_t nv, size_t nnz, swm_rng* rng, swm_srs** out) {
    if (!ctx || !rng || !out) return SWM_ERR_INVALID_ARG;
    SWM_ON_DEVICE(ctx);
    SWM_GUARD(ctx, *out = universal_setup(ctx, nc, nv, nnz, rng->r));
}
void swm_srs_destroy(swm_ctx* ctx, swm_srs* srs) {
    if (!srs) return;
    swm::DeviceGuard g(ctx);
    if (ctx) drain_streams(ctx);
    delete srs;
}
size_t swm_srs_max_degree(const swm_srs* srs) { return srs ? srs->max_degree : 0; }
int swm_srs_power_of_g(swm_ctx* ctx, const swm_srs* srs, size_t i, uint64_t out_xy[12]) {
    if (!ctx || !srs || !out_xy || i > srs->max_degree) return SWM_ERR_INVALID_ARG;
    SWM_ON_DEVICE(ctx);
    SWM_GUARD(ctx, {
        G1Affine p = srs_power(ctx, srs->d_powers, i);
        memcpy(out_xy, &p, sizeof(p));
    });
}

static void g2_to_limbs(const G2Affine& p, uint64_t out[24]) {
    if (p.inf) {
        memset(out, 0, 24 * 8);
        return;
    }
    memcpy(out, &p.x.c0, 48);
    memcpy(out + 6, &p.x.c1, 48);
    memcpy(out + 12, &p.y.c0, 48);
    memcpy(out + 18, &p.y.c1, 48);
}
static G2Affine g2_from_limbs(const uint64_t in[24]) {
    G2Affine p;
    bool zero = true;
    for (int i = 0; i < 24; i++) zero &= in[i] == 0;
    if (zero) return g2_identity();
    p.inf = false;
    memcpy(&p.x.c0, in, 48);
    memcpy(&p.x.c1, in + 6, 48);
    memcpy(&p.y.c0, in + 12, 48);
    memcpy(&p.y.c1, in + 18, 48);
    return p;
}
int swm_srs_export(swm_ctx* ctx, const swm_srs* srs, size_t first, size_t count, uint64_t* powers_xy, uint64_t gamma_xy[36],
                   uint64_t h[24], uint64_t beta_h[24]) {
    if (!ctx || !srs || first > srs->max_degree + 1 || count > srs->max_degree + 1 - first || (count && !powers_xy))
        return SWM_ERR_INVALID_ARG;
    SWM_ON_DEVICE(ctx);
    SWM_GUARD(ctx, {
        if (count) {
            hip_check(ctx, hipMemcpyAsync(powers_xy, srs->d_powers + first, count * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->stream), "d2h");
            hip_check(ctx, hipStreamSynchronize(ctx->stream), "sync");
        }
        if (gamma_xy)
            for (size_t i = 0; i < 3; i++) memcpy(gamma_xy + 12 * i, &srs->gamma_powers[i], sizeof(G1Affine));
        if (h) g2_to_limbs(srs->h, h);
        if (beta_h) g2_to_limbs(srs->beta_h, beta_h);
    });
}
int swm_srs_import(swm_ctx* ctx, const uint64_t* powers_xy, size_t n_powers, const uint64_t gamma_xy[36], const uint64_t h[24],
                   const uint64_t beta_h[24], swm_srs** out) {
    if (!ctx || !powers_xy || n_powers < 2 || !gamma_xy || !h || !beta_h || !out) return SWM_ERR_INVALID_ARG;
    SWM_ON_DEVICE(ctx);
    SWM_GUARD(ctx, {
        std::unique_ptr<swm_srs> srs(new swm_srs());
        srs->max_degree = n_powers - 1;
        for (size_t i = 0; i < 3; i++) {
            G1Affine g;
            memcpy(&g, gamma_xy + 12 * i, sizeof(G1Affine));
            srs->gamma_powers.push_back(g);
        }
        srs->h = g2_from_limbs(h);
        srs->beta_h = g2_from_limbs(beta_h);
        hip_check(ctx, hipMalloc((void**)&srs->d_powers, n_powers * sizeof(G1Affine)), "hipMalloc(srs)");
        hip_check(ctx, hipMemcpyAsync(srs->d_powers, powers_xy, n_powers * sizeof(G1Affine), hipMemcpyHostToDevice, ctx->stream), "h2d");
        hip_check(ctx, hipStreamSynchronize(ctx->stream), "sync");
        rc_check(ctx, msm_subgroup_check(ctx, srs->d_powers, n_powers, &srs->in_subgroup));
        *out = srs.release();
    });
}

int swm_generate_proving_and_verifying_keys(swm_ctx* ctx, const swm_srs* srs, const swm_r1cs* cs, swm_pk** pk,
                                            swm_vk** vk) {
    if (!ctx || !srs || !cs || !pk || !vk) return SWM_ERR_INVALID_ARG;
    SWM_ON_DEVICE(ctx);
    SWM_GUARD(ctx, index_impl(ctx, srs, cs, pk, vk));
}
void swm_pk_destroy(swm_ctx* ctx, swm_pk* pk) {
    if (!pk) return;
    {
        swm::DeviceGuard g(ctx);
        if (ctx) drain_streams(ctx);  // what THIS holder still has in flight on the key
    }
    if (pk->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;  // other holders remain
    // last holder: the blocks go back to the runtime.  Every holder drained its own context when it let go; a holder that
    // passed ctx == NULL did not, so the device is awaited once here (destroying a multi-GB key is not a hot path)
    const int dev = pk->device;
    int prev = -1;
    (void)hipGetDevice(&prev);
    const bool there = hipSetDevice(dev) == hipSuccess;
    if (there) (void)hipDeviceSynchronize();
    delete pk;
    if (there && prev >= 0 && prev != dev) (void)hipSetDevice(prev);
}
int swm_pk_retain(swm_pk* pk) {
    if (!pk) return SWM_ERR_INVALID_ARG;
    pk->refs.fetch_add(1, std::memory_order_relaxed);
    return SWM_OK;
}
int swm_pk_attach(swm_ctx* ctx, swm_pk* pk) {
    if (!ctx || !pk) return SWM_ERR_INVALID_ARG;
    if (ctx->device != pk->device)
        return set_err(ctx, SWM_ERR_MISMATCH, "swm_pk_attach: the key is resident on device %d, the context runs on device %d", pk->device,
                       ctx->device);
    pk->refs.fetch_add(1, std::memory_order_relaxed);
    return SWM_OK;
}
int swm_pk_device(const swm_pk* pk) { return pk ? pk->device : SWM_ERR_INVALID_ARG; }
int swm_pk_refcount(const swm_pk* pk) { return pk ? pk->refs.load(std::memory_order_relaxed) : SWM_ERR_INVALID_ARG; }
int swm_device_mem_info(swm_ctx* ctx, size_t* free_bytes, size_t* total_bytes) {
    if (!ctx || !free_bytes || !total_bytes) return SWM_ERR_INVALID_ARG;
    SWM_ON_DEVICE(ctx);
    SWM_HIP(ctx, hipMemGetInfo(free_bytes, total_bytes));
    return SWM_OK;
}

int swm_generate_proof(swm_ctx* ctx, const swm_pk* pk, const swm_r1cs* cs, swm_rng* rng, uint8_t* proof_out, size_t cap,
                       size_t* len) {
    return swm_generate_proof_ex(ctx, pk, cs, rng, 0, proof_out, cap, len);
}
int swm_generate_proof_ex(swm_ctx* ctx, const swm_pk* pk, const swm_r1cs* cs, swm_rng* rng, unsigned flags, uint8_t* proof_out,
                          size_t cap, size_t* len) {
    if (!ctx || !pk || !cs || !rng || !proof_out || !len || (flags & ~(unsigned)SWM_PROOF_UNCOMPRESSED)) return SWM_ERR_INVALID_ARG;
    if (ctx->device != pk->device)
        return set_err(ctx, SWM_ERR_MISMATCH, "swm_generate_proof: the key is resident on device %d, the context runs on device %d",
                       pk->device, ctx->device);
    SWM_ON_DEVICE(ctx);
    SWM_GUARD(ctx, {
        std::vector<uint8_t> bytes = prove_impl(ctx, *pk, cs, rng->r, (flags & SWM_PROOF_UNCOMPRESSED) != 0);
        *len = bytes.size();
        if (bytes.size() > cap) throw MarlinError(SWM_ERR_INVALID_ARG, "proof buffer too small");
        memcpy(proof_out, bytes.data(), bytes.size());
    });
}

int swm_pk_serialize_ex(swm_ctx* ctx, const swm_pk* pk, unsigned flags, uint8_t* out, size_t cap, size_t* len) {
    if (!ctx || !pk || !len || !key_flags_ok(flags, true)) return SWM_ERR_INVALID_ARG;
    SWM_ON_DEVICE(ctx);
    SWM_GUARD(ctx, {
        std::vector<uint8_t> b = pk_serialize(ctx, *pk, (flags & SWM_KEY_UNCOMPRESSED) != 0);
        *len = b.size();
        if (out) {
            if (b.size() > cap) throw MarlinError(SWM_ERR_INVALID_ARG, "buffer too small");
            memcpy(out, b.data(), b.size());
        }
    });
}
int swm_pk_serialize(swm_ctx* ctx, const swm_pk* pk, uint8_t* out, size_t cap, size_t* len) {
    return swm_pk_serialize_ex(ctx, pk, 0, out, cap, len);
}
int swm_pk_deserialize_ex(swm_ctx* ctx, const uint8_t* bytes, size_t len, unsigned flags, swm_pk** out) {
    if (!ctx || !bytes || !out || !key_flags_ok(flags, false)) return SWM_ERR_INVALID_ARG;
    SWM_ON_DEVICE(ctx);
    SWM_GUARD(ctx, *out = pk_deserialize(ctx, bytes, len, (flags & SWM_KEY_UNCOMPRESSED) != 0, !(flags & SWM_KEY_UNCHECKED)));
}
int swm_pk_deserialize(swm_ctx* ctx, const uint8_t* bytes, size_t len, swm_pk** out) {
    return swm_pk_deserialize_ex(ctx, bytes, len, 0, out);
}
int swm_r1cs_is_satisfied(swm_ctx* ctx, const swm_r1cs* cs, int* ok, size_t* first_bad) {
    if (!ctx || !cs || !ok) return SWM_ERR_INVALID_ARG;
    SWM_ON_DEVICE(ctx);
    SWM_GUARD(ctx, is_satisfied_impl(ctx, cs, ok, first_bad));
}

// ------------------------------------------------------------------------------------------------ K4 self-tests
// The prover's own host drivers of devops.cuh on host data (include/swmarlin.h: swm_selftest_poly names the ops).
static void selftest_poly_impl(swm_ctx* ctx, int op, void* data, size_t n, size_t m, const uint64_t* z, const uint64_t* pieces,
                               size_t npieces, void* out) {
    Fr zz = fp_zero<Fr>();
    if (z) memcpy(zz.v, z, 32);
    if (op == 8) {  // exclusive scan of n u32 words: out[0..n) and the total at out[n]
        DBuf<uint32_t> in(ctx, n), res(ctx, n);
        if (n) in.upload((const uint32_t*)data, n);
        const uint32_t total = scan_exclusive_u32(ctx, in.p, res.p, n);
        std::vector<uint32_t> h = res.download(0, n);
        if (n) memcpy(out, h.data(), n * 4);
        ((uint32_t*)out)[n] = total;
        return;
    }
    DVec a(ctx, n);
    if (n) a.upload((const Fr*)data, n);
    if (op == 9) {  // ntt_cosets_fwd of data[0..n) (n <= 2^(m+1)) onto the npieces cosets pieces[c] of 2^m points: out[c 2^m + j]
        unsigned ks[4];
        for (size_t c = 0; c < npieces; c++) ks[c] = (unsigned)pieces[c];
        DVec t(ctx, npieces << m);
        rc_check(ctx, ntt_cosets_fwd(ctx, a.p, n, (unsigned)m, ks, (unsigned)npieces, t.p));
        std::vector<Fr> h = t.download(0, t.n);
        memcpy(out, h.data(), t.n * sizeof(Fr));
        return;
    }
    if (op == 10) {  // data = evaluations on the cosets 0, 1, 2 of 2^m points -> out = the 3 2^m coefficients (degree < 3 2^m)
        const size_t N = (size_t)1 << m;
        rc_check(ctx, ntt_cosets_inv(ctx, a.p, (unsigned)m, 3));
        DVec t(ctx, 3 * N);
        const Fr* u = a.p;
        Fr* o = t.p;
        const Fr iota = HDomain(4).gen, half = fr_half();
        ew(ctx, "cosets3_solve", N, [=] __device__(size_t j) {
            const Cosets3 c = cosets3_solve(u[j], u[j + N], u[j + 2 * N], iota, half);
            o[j] = c.p0;
            o[j + N] = c.p1;
            o[j + 2 * N] = c.p2;
        });
        std::vector<Fr> h = t.download(0, t.n);
        memcpy(out, h.data(), t.n * sizeof(Fr));
        return;
    }
    if (op == 11) {  // suffix_recurrence_from: data[0..n) divided by (X - z) into a buffer of m >= n elements that starts as bytes 0xFF
        const size_t cap = std::max<size_t>(m, 1);
        DVec dst(ctx, cap);
        hip_check(ctx, hipMemsetAsync(dst.p, 0xFF, cap * sizeof(Fr), ctx->stream), "memset");
        suffix_recurrence_from(ctx, a.p, dst.p, n, cap, zz);
        std::vector<Fr> h = dst.download(0, cap);
        memcpy(out, h.data(), cap * sizeof(Fr));
        std::vector<Fr> src = a.download(0, n);
        if (n) memcpy(data, src.data(), n * sizeof(Fr));
        return;
    }
    if (op == 0) {  // suffix_recurrence(a, n, m, z) in place
        suffix_recurrence(ctx, a.p, n, m, zz);
        std::vector<Fr> h = a.download(0, n);
        if (n) memcpy(data, h.data(), n * sizeof(Fr));
    } else if (op == 1) {  // div_linear: out[0] = p(z), out[1..n) = the quotient by (X - z)
        DivResult r = div_linear(ctx, a.p, n, zz);
        std::vector<Fr> h = r.work.download(0, n);
        if (n) memcpy(out, h.data(), n * sizeof(Fr));
    } else if (op == 2) {  // poly_eval: out[0] = p(z)
        const Fr v = poly_eval(ctx, a.p, n, zz);
        memcpy(out, v.v, sizeof(Fr));
    } else if (op == 3) {  // poly_eval_many over the pieces (offset, length) of data, one result each
        for (size_t i = 0; i < npieces; i++)
            if (pieces[2 * i] > n || pieces[2 * i + 1] > n - pieces[2 * i]) throw MarlinError(SWM_ERR_INVALID_ARG, "piece out of range");
        DVec res(ctx, npieces);
        std::vector<EvalItem> items;
        for (size_t i = 0; i < npieces; i++) items.push_back({a.p + pieces[2 * i], (size_t)pieces[2 * i + 1], res.p + i});
        EvalPoint ep = eval_point(ctx, zz);
        poly_eval_many(ctx, items, ep);
        std::vector<Fr> h = res.download(0, npieces);
        if (npieces) memcpy(out, h.data(), npieces * sizeof(Fr));
    } else {  // ops 4 - 7: dv_ntt_from of data[0..n) into 2^m elements, inverse = bit 0, coset = bit 1 of op - 4; data gets the
              // source back as the device holds it afterwards
        DVec t = dv_ntt_from(ctx, a.p, n, (unsigned)m, ((op - 4) & 1) != 0, ((op - 4) & 2) != 0);
        std::vector<Fr> h = t.download(0, t.n);
        memcpy(out, h.data(), t.n * sizeof(Fr));
        std::vector<Fr> s = a.download(0, n);
        if (n) memcpy(data, s.data(), n * sizeof(Fr));
    }
}
int swm_selftest_poly(swm_ctx* ctx, int op, void* data, size_t n, size_t m, const uint64_t z[4], const uint64_t* pieces,
                      size_t npieces, void* out) {
    if (!ctx || op < 0 || op > 11 || (n && !data)) return SWM_ERR_INVALID_ARG;
    if (op == 11 && (!z || m < n || m < 1)) return SWM_ERR_INVALID_ARG;
    if ((op >= 1 && op <= 3 && !z) || (op == 0 && (!z || m == 0)) || (op != 0 && !out) || (op == 3 && npieces && !pieces))
        return SWM_ERR_INVALID_ARG;
    if (op >= 4 && op <= 7 && (m < 1 || m > 28 || n > ((size_t)1 << m))) return SWM_ERR_INVALID_ARG;
    if (op == 9) {
        if (m < 1 || m > 26 || n > ((size_t)2 << m) || npieces < 1 || npieces > 4 || !pieces) return SWM_ERR_INVALID_ARG;
        for (size_t c = 0; c < npieces; c++)
            if (pieces[c] > 3) return SWM_ERR_INVALID_ARG;
    }
    if (op == 10 && (m < 1 || m > 26 || n != ((size_t)3 << m))) return SWM_ERR_INVALID_ARG;
    SWM_ON_DEVICE(ctx);
    SWM_GUARD(ctx, selftest_poly_impl(ctx, op, data, n, m, z, pieces, npieces, out));
}
// spmv_run with the plan upload_csr records for a key's matrix, on a host CSR in the memory form
static void selftest_spmv_plan_impl(swm_ctx* ctx, const uint32_t* rowptr, const uint32_t* col, const uint64_t* val, size_t rows,
                                    const uint64_t* z, size_t z_len, uint64_t* out, uint32_t* plan_counts) {
    const size_t nnz = rowptr[rows];
    HostCsr m;
    m.rowptr.assign(rowptr, rowptr + rows + 1);
    m.col.assign(col, col + nnz);
    m.val.resize(nnz);
    if (nnz) memcpy(m.val.data(), val, nnz * sizeof(Fr));
    DevCsr d = upload_csr(ctx, m);
    DVec dz(ctx, z_len), o(ctx, rows);
    dz.upload((const Fr*)z, z_len);
    // a row that no kernel of the schedule writes must show: the pool may hand back a block that holds an earlier result
    hip_check(ctx, hipMemsetAsync(o.p, 0xFF, rows * sizeof(Fr), ctx->stream), "memset");
    rc_check(ctx, spmv_run(ctx, d.rowptr.p, d.col.p, d.val.p, dz.p, o.p, rows, &d.plan));
    std::vector<Fr> h = o.download(0, rows);
    memcpy(out, h.data(), rows * sizeof(Fr));
    if (plan_counts) {
        plan_counts[0] = d.plan.n_chunks;
        plan_counts[1] = d.plan.n_lrows;
    }
}
int swm_selftest_spmv_plan(swm_ctx* ctx, const uint32_t* rowptr, const uint32_t* col, const uint64_t* val, size_t rows,
                           const uint64_t* z, size_t z_len, uint64_t* out, uint32_t plan_counts[2]) {
    if (!ctx || !rowptr || !rows || rows >= ((size_t)1 << 31) || !z || !z_len || !out || rowptr[0] != 0) return SWM_ERR_INVALID_ARG;
    for (size_t r = 0; r < rows; r++)
        if (rowptr[r + 1] < rowptr[r]) return SWM_ERR_INVALID_ARG;
    const size_t nnz = rowptr[rows];
    if (nnz && (!col || !val)) return SWM_ERR_INVALID_ARG;
    for (size_t k = 0; k < nnz; k++)
        if (col[k] >= z_len) return SWM_ERR_INVALID_ARG;
    SWM_ON_DEVICE(ctx);
    SWM_GUARD(ctx, selftest_spmv_plan_impl(ctx, rowptr, col, val, rows, z, z_len, out, plan_counts));
}
// sample_fr_bulk on a generator handle into a device buffer, then the download
static void selftest_sample_impl(swm_ctx* ctx, ChaChaRng& rng, size_t need, uint64_t* out_mont) {
    DVec d(ctx, need);
    sample_fr_bulk(ctx, rng, d.p, need);
    std::vector<Fr> h = d.download(0, need);
    if (need) memcpy(out_mont, h.data(), need * sizeof(Fr));
}
int swm_selftest_sample_fr(swm_ctx* ctx, swm_rng* rng, size_t need, uint64_t* out_mont) {
    if (!ctx || !rng || (need && !out_mont)) return SWM_ERR_INVALID_ARG;
    SWM_ON_DEVICE(ctx);
    SWM_GUARD(ctx, selftest_sample_impl(ctx, rng->r, need, out_mont));
}

// the key codec's point kernels on host buffers (include/swmarlin.h names the ops)
static void selftest_g1_codec_impl(swm_ctx* ctx, int op, const void* in, size_t n, void* out, unsigned* bad) {
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (op == 0) {
        DBuf<G1Affine> pts(ctx, n);
        DBuf<uint32_t> enc(ctx, n * 24);
        pts.upload((const G1Affine*)in, n);
        LAUNCHX(ctx, "g1_encode_uncompressed", g1_encode_uncompressed_kernel, grid, block, 0, pts.p, n, enc.p);
        std::vector<uint32_t> h = enc.download(0, n * 24);
        memcpy(out, h.data(), n * 96);
        return;
    }
    DBuf<uint32_t> enc(ctx, n * 24), flag(ctx, 1);
    DBuf<G1Affine> pts(ctx, n);
    flag.zero();
    enc.upload((const uint32_t*)in, n * 24);
    if (op == 1) LAUNCHX(ctx, "g1_decode_uncompressed", g1_decode_uncompressed_kernel<true>, grid, block, 0, enc.p, n, pts.p, flag.p);
    else LAUNCHX(ctx, "g1_decode_unchecked", g1_decode_uncompressed_kernel<false>, grid, block, 0, enc.p, n, pts.p, flag.p);
    *bad = flag.download(0, 1)[0];
    std::vector<G1Affine> h = pts.download(0, n);
    memcpy(out, h.data(), n * sizeof(G1Affine));
}
int swm_selftest_g1_codec(swm_ctx* ctx, int op, const void* in, size_t n, void* out, unsigned* bad) {
    if (!ctx || op < 0 || op > 2 || (n && (!in || !out)) || (op != 0 && !bad) || n > ((size_t)1 << 31)) return SWM_ERR_INVALID_ARG;
    SWM_ON_DEVICE(ctx);
    if (op != 0) *bad = 0;
    if (n == 0) return SWM_OK;
    SWM_GUARD(ctx, selftest_g1_codec_impl(ctx, op, in, n, out, bad));
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ pairing self-test (host only)
extern "C" int swm_selftest_pairing(unsigned* failed) {
    using namespace swm;
    if (!failed) return SWM_ERR_INVALID_ARG;
    static const uint32_t gx[12] = SWM_G1_GEN_X_MONT, gy[12] = SWM_G1_GEN_Y_MONT;
    G1Affine P;
    for (int i = 0; i < 12; i++) {
        P.x.v[i] = gx[i];
        P.y.v[i] = gy[i];
    }
    G2Affine Q = g2_identity();  // a point of the prime-order subgroup of the twist: first abscissa s + u with a square, cofactor cleared
    for (unsigned s = 1; s < 200 && Q.inf; s++) {
        Fq2 x = {fp_from_u64<Fq>(s), fp_from_u64<Fq>(1)}, y;
        if (fq2_sqrt(x * x * x + g2_coeff_b(), &y)) {
            static const uint32_t cof[SWM_G2_COFACTOR_LIMBS] = SWM_G2_COFACTOR;
            Q = g2_mul({x, y, false}, cof, SWM_G2_COFACTOR_LIMBS);
        }
    }
    if (Q.inf) return SWM_ERR_INTERNAL;
    unsigned bad = 0;
    const Fq12 f = miller_loop(P, Q);
    Fq12 g = f.conjugate() * f.inverse();
    g = frobenius2(g) * g;
    if (!(cyclotomic_square(g) == g * g)) bad |= 1u << 0;
    static const uint32_t e2[SWM_FINAL_EXP2_LIMBS] = SWM_FINAL_EXP2;
    const Fq12 plain = (f.conjugate() * f.inverse()).pow(e2, SWM_FINAL_EXP2_LIMBS);
    const Fq12 win = final_exponentiation_windowed(f);
    if (!(win == plain)) bad |= 1u << 1;
    const Fq12 e = final_exponentiation(f);
    if (!(e == win * win * win)) bad |= 1u << 2;
    if (!(frobenius1(frobenius1(f)) == frobenius2(f))) bad |= 1u << 3;
    const G1Affine P2 = g1_mul_fr(P, fp_from_u64<Fr>(2));
    if (!(final_exponentiation(miller_loop(P2, Q)) == e * e) || e.is_one()) bad |= 1u << 4;
    if (!product_of_pairings_is_one({{P, Q}, {g1_neg(P), Q}}) || product_of_pairings_is_one({{P, Q}, {P, Q}})) bad |= 1u << 5;
    if (!(multi_miller_loop({{P, Q}, {P2, Q}}) == f * miller_loop(P2, Q))) bad |= 1u << 6;
    *failed = bad;
    return SWM_OK;
}


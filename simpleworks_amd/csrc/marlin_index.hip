// marlin_index.hip — building a key from a constraint system: the R1CS padding (ark-marlin constraint_systems.rs), the universal
// setup (KZG10::setup: a fixed-base MSM on the device), the indexer (arithmetisation, committer key, the twelve index commitments)
// and is_satisfied.  Only the three gamma-powers KZG hiding needs are generated at setup (arkworks generates max_degree + 2): no
// proof byte depends on the rest.  marlin_keycodec.hip rebuilds a loaded key's derived tables with the same functions (marlin_units.h).
#include "marlin_units.h"

namespace {

// ================================================================================================ host helpers
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

}  // namespace

namespace swm {

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

}  // namespace swm

namespace {

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

}  // namespace

namespace swm {

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

}  // namespace swm

namespace {

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

}  // namespace

namespace swm {

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

}  // namespace swm

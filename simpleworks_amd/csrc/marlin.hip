// marlin.hip — MI355X-native Marlin (universal setup, indexer, prover) behind the surface of
// /root/reference/src/marlin/mod.rs:45-94.  The arithmetic the reference delegates to ark-marlin / ark-poly-commit /
// ark-poly / ark-ec (not vendored; restated from SURVEY.md Appendix A [U]) runs as HIP kernels with all polynomials
// resident in HBM between the NTTs (K2), the mat-vecs (K3), the support kernels (K4) and the commitments (K1);
// the host drives the schedule, owns the Fiat-Shamir transcript and touches only O(1)-sized data per round.
//
// This unit is the C ABI of that surface (SRS, keys, proof, swm_r1cs_is_satisfied), the entry points that need no GPU
// (host/host_abi.inc) and the K4 / pairing self-tests.  The work is in marlin_commit.hip (commitments), marlin_index.hip (setup,
// indexer, is_satisfied), marlin_prove.hip (prover) and marlin_keycodec.hip (proving-key codec, with its own self-test);
// marlin_units.h is what the five share.
#include "marlin_units.h"

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


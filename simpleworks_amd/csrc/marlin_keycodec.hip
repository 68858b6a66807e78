// marlin_keycodec.hip — the proving key's wire forms (swm_pk_serialize[_ex] / swm_pk_deserialize[_ex]): the four point kernels, the
// writer, the reader, and the self-test that launches those kernels on host buffers.  A loaded key's derived tables are rebuilt
// by the index unit's functions (marlin_units.h); the part of the reader that needs no GPU is host/pk_codec.h.
#include "marlin_units.h"

namespace {

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

}  // namespace

namespace swm {

std::vector<uint8_t> pk_serialize(swm_ctx* ctx, const swm_pk& pk, bool uncompressed) {
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

}  // namespace swm

namespace {

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

}  // namespace

namespace swm {

// uncompressed / checked: which of arkworks' three forms the bytes are in (include/swmarlin.h, swm_pk_deserialize_ex).  The
// structural checks, the committer-key / verifying-key comparison and the recomputation of the derived tables are the same in all.
swm_pk* pk_deserialize(swm_ctx* ctx, const uint8_t* bytes, size_t len, bool uncompressed, bool checked) {
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

}  // namespace swm

// ================================================================================================ self-test
extern "C" {

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

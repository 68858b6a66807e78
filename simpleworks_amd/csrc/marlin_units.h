// marlin_units.h — what the units of the Marlin surface share among themselves: marlin.hip (C ABI, self-tests), marlin_commit.hip
// (commitments), marlin_index.hip (setup, indexer, is_satisfied), marlin_keycodec.hip (proving-key codec), marlin_prove.hip (prover).
// The handle structs, the commitment jobs, and the declarations of the host functions that cross a unit: never a kernel — a
// kernel is launched in the unit that defines it (every ew(...) lambda included: its kernel is instantiated where it is written).
#pragma once
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include "devops.cuh"
#include "g1.cuh"
#include "host/ahp.h"

#include "msm.h"
using namespace swm;  // (as marlin.hip always had it: the two handle structs below are global, everything they are made of is swm's)

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

namespace swm {  // (members of swm_pk, which several units see: no internal linkage)

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

}  // namespace swm

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

namespace swm {

// ================================================================================================ commitments (marlin_commit.hip)
typedef std::vector<Fr> HPoly;  // host polynomial: the degree-<=2 blinding polynomials
// asynchronous form: alternates between the two MSM lanes of the context
// With swm_set_msm_sharding active the context only takes its own point range of every MSM and the partial sums are
// exchanged in commit_wait (all-gather of one point per rank + the same rank-ordered sum everywhere).
struct AsyncMsm {
    MsmJob job;
    bool sharded = false;
    bool have_result = false;  // set by commit_gather (the exchange of a whole round) before commit_wait is reached
    G1XYZZ result;
};
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
void shard_agree(swm_ctx* ctx, const swm_pk& pk);
G1XYZZ gamma_msm(const swm_pk& pk, const std::vector<Fr>& coeffs);
void commit_enqueue(swm_ctx* ctx, int* lane, const swm_pk& pk, size_t offset, const Fr* coeffs, size_t n, AsyncMsm* out,
                    const size_t* twin_offset = nullptr, AsyncMsm* twin_lead = nullptr);
bool commit_cyclic_possible(swm_ctx* ctx, const swm_pk& pk, size_t n_local);
void commit_enqueue_cyclic(swm_ctx* ctx, int* lane, const swm_pk& pk, const Fr* local, size_t n_local, AsyncMsm* out);
void commit_flush(swm_ctx* ctx);
void commit_gather(swm_ctx* ctx, std::initializer_list<AsyncMsm*> jobs);
G1XYZZ commit_wait(swm_ctx* ctx, AsyncMsm* a);
void pc_commit_begin(swm_ctx* ctx, const swm_pk& pk, int* lane, const Fr* coeffs, size_t n, bool has_bound, uint64_t bound,
                     bool hiding, CommitJob* job);
void pc_commit_blind(const swm_pk& pk, CommitJob* job, ChaChaRng* rng, PolyRand* pr);
void g1_to_affine_batch(const G1XYZZ* in, int k, G1Affine* out);
void pc_commit_end_round(swm_ctx* ctx, const swm_pk& pk, std::initializer_list<CommitJob*> jobs,
                         std::initializer_list<ChaChaRng*> rngs, std::initializer_list<PolyRand*> prs, Commitment* out);

// ================================================================================================ setup, indexer (marlin_index.hip)
// position of variable `index` on H: the instance on the X-subgroup, the witness on the rest (indexer: arithmetize; prover: t)
__device__ __forceinline__ uint64_t reindex_by_subdomain(uint64_t H, uint64_t X, uint64_t index) {
    uint64_t period = H / X;
    if (index < X) return index * period;
    uint64_t i = index - X, x = period - 1;
    return i + (i / x) + 1;
}
GammaTable build_gamma_table(const std::vector<G1Affine>& gp);
HostCsr transpose(const HostCsr& m, size_t ncols);
DevCsr upload_csr(swm_ctx* ctx, const HostCsr& m);
uint64_t ahp_max_degree(uint64_t num_constraints, uint64_t num_variables, uint64_t num_non_zero);
swm_srs* universal_setup(swm_ctx* ctx, size_t nc, size_t nv, size_t nnz, ChaChaRng& rng);
G1Affine srs_power(swm_ctx* ctx, const G1Affine* d_powers, size_t i);
void arithmetize(swm_ctx* ctx, swm_pk& pk, const HostCsr& m, MatrixArith& ar);
void install_committer_key(swm_ctx* ctx, swm_pk& pk, const G1Affine* powers, size_t n_powers, const G1Affine* shifted,
                           size_t n_shifted, bool device_src, bool in_subgroup);
void pk_publish(swm_ctx* ctx, swm_pk& pk);
void index_impl(swm_ctx* ctx, const swm_srs* srs, const swm_r1cs* cs, swm_pk** out_pk, swm_vk** out_vk);
void is_satisfied_impl(swm_ctx* ctx, const swm_r1cs* cs, int* ok, size_t* first_bad);

// ================================================================================================ prover (marlin_prove.hip)
std::vector<uint8_t> prove_impl(swm_ctx* ctx, const swm_pk& pk, const swm_r1cs* cs, ChaChaRng& zk, bool uncompressed = false);

// ================================================================================================ key codec (marlin_keycodec.hip)
std::vector<uint8_t> pk_serialize(swm_ctx* ctx, const swm_pk& pk, bool uncompressed = false);
swm_pk* pk_deserialize(swm_ctx* ctx, const uint8_t* bytes, size_t len, bool uncompressed = false, bool checked = true);

}  // namespace swm

// marlin_commit.hip — the commitment layer of the Marlin surface (marlin_units.h: AsyncMsm, PolyRand, CommitJob): MarlinKZG10::commit
// over polynomials resident in HBM as asynchronous MSM jobs (msm.h), their split over the ranks of a sharded proof, the hiding terms
// and the batch normalisation at the end of a round.  Host code only: the kernels are the MSM's.  Used by the indexer
// (marlin_index.hip) and the prover (marlin_prove.hip).
#include "marlin_units.h"

namespace swm {

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
// twin_offset / twin_lead (msm.h: MsmTwin): this commitment is followed by one of the SAME coefficients against the powers from
// *twin_offset on / follows the commitment twin_lead of the same coefficients — the degree-shifted commitment of a bounded
// polynomial beside its plain one; the second job then takes the first one's sort.
void commit_enqueue(swm_ctx* ctx, int* lane, const swm_pk& pk, size_t offset, const Fr* coeffs, size_t n, AsyncMsm* out,
                    const size_t* twin_offset, AsyncMsm* twin_lead) {
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

// MarlinKZG10::commit for one labelled polynomial in two halves (marlin_units.h: CommitJob, PolyRand)
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

}  // namespace swm

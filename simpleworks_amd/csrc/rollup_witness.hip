// rollup_witness.hip — ONE proof for a block of transfers: the witness of the rollup circuit (simpleworks_amd/workloads.py,
// build_rollup / build_pedersen_rollup; host/rollup_shape.h the counts and offsets) laid out on the GPU as one contiguous z, the
// tree and the account table advanced all-or-nothing, and the proof entries on top of it.  There is no circuit handle of its own:
// a rollup takes a transfer circuit (either tree's) and N.  Written once over the two transfer units (transfer_units.h), in the
// style of ledger_witness_host.h: a unit hands over a small struct U, the extern "C" functions are instantiations.
//
// A block of N transfers is
//   snapshot  the tree's nodes copied aside on the device (the table's device copy is the call's own: the caller's is the snapshot)
//   pass      the unit's witness pass (transfer_run_strided / pedersen_transfer_run_strided) at a stride of W_t + 1 into one buffer
//             of N (W_t + 1) - 1 elements: section k's W_t witnesses at k (W_t + 1); the tree and the table advance through the
//             block as the transfers apply, exactly as under swm_transfer_witness_at
//   link      rollup_link_kernel, one wave: lane k < N - 1 converts the root transfer k published (canonical words) to the prover's
//             form and stores it behind section k (root_{k+1}); the N flag bytes and status words reduce to one verdict word, the
//             number of transfers that were not applied
//   results   the two verdict words, the first old root, the last new root, flags and status to the host, one wait
//   rollback  a verdict above zero: the snapshot goes back over the nodes, the table is not returned
// The block is never chunked: z is contiguous.  The prover then reads the buffer where it lies (prove_device_witness).
#include <hip/hip_runtime.h>

#include <string.h>

#include <string>
#include <vector>

#include "context.h"
#include "ff.cuh"
#include "host/rollup_shape.h"
#include "ledger_witness_host.h"
#include "poseidon.h"
#include "swmarlin.h"
#include "transfer_units.h"
#include "witness_host.h"

namespace swm {

static constexpr unsigned RU_LANES = 64;  // one wave: a lane per transfer
static_assert(RU_MAX_TRANSFERS <= RU_LANES, "the link kernel has a lane per transfer");

// One workgroup of one wave.  new_roots: n x 8 canonical words (a tree's nodes); witness: the block's buffer, n x stride - 1
// elements; root_at: W_t.  verdict: how many of the n transfers the pass did not apply.
__global__ void __launch_bounds__(RU_LANES) rollup_link_kernel(const uint32_t* __restrict__ new_roots, const uint8_t* __restrict__ flags,
                                                               const uint32_t* __restrict__ status, unsigned n, size_t stride, size_t root_at,
                                                               Fr* __restrict__ witness, uint32_t* __restrict__ verdict) {
    const unsigned k = threadIdx.x;
    bool refused = false;
    if (k < n) {
        refused = !(flags[k] & TRANSFER_FLAG_APPLIED) || status[k] != 0;
        if (k + 1 < n) {  // the last section has no root behind it: the buffer ends with its last witness
            Fr r;
#pragma unroll
            for (int w = 0; w < 8; w++) r.v[w] = new_roots[8 * k + w];
            r = fp_from_std(r);  // a digest is canonical
            uint4* q = reinterpret_cast<uint4*>(witness + (size_t)k * stride + root_at);
            q[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
            q[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
        }
    }
    const unsigned long long mask = __ballot(refused);
    if (k == 0) *verdict = (uint32_t)__popcll(mask);
}

struct RollupBlock {  // the caller's arrays
    const uint8_t *msgs, *sigs;
    uint8_t *old_root, *new_root, *flags;
    uint32_t* status;
};

// The witness pass of a block: *d_w the block's z on the device ("rollup.w"), *applied whether tree and table were advanced.
// accounts: read, and written when the block applied.  witness (may be NULL): the host copy of z.
template <class U>
int rollup_pass(swm_ctx* ctx, const char* what, const typename U::Circuit* c, typename U::Tree* tree, uint8_t* accounts, const RollupBlock& b,
                const RollupShape& s, uint64_t* witness, Fr** d_w, int* applied) {
    const size_t n = s.transfers, levels = c->shape.levels, table_bytes = PY_LEAF_LEN << levels, node_bytes = tree->num_nodes() * 32;
    const size_t w_bytes = s.num_witness * sizeof(Fr);
    uint8_t *d_accounts = nullptr, *d_in = nullptr, *d_out = nullptr, *d_snap = nullptr;
    SWM_TRY(block_upload_accounts(ctx, U::accounts_scratch, accounts, table_bytes, &d_accounts));
    SWM_TRY(scratch(ctx, "stage.a", n * (64 + PY_MSG_LEN) + 16, (void**)&d_in));
    SWM_HIP(ctx, hipMemcpyAsync(d_in, b.sigs, 64 * n, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(d_in + 64 * n, b.msgs, PY_MSG_LEN * n, hipMemcpyHostToDevice, ctx->stream));
    SWM_TRY(scratch(ctx, "rollup.w", w_bytes + 16, (void**)&d_out));
    SWM_TRY(scratch(ctx, "rollup.snapshot", node_bytes + 16, (void**)&d_snap));  // the nodes | the verdict word
    uint32_t* d_verdict = reinterpret_cast<uint32_t*>(d_snap + node_bytes);
    SWM_HIP(ctx, hipMemcpyAsync(d_snap, tree->d_nodes, node_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    BlockRunOut O;
    SWM_TRY(U::run(ctx, c, tree, d_accounts, d_in + 64 * n, d_in, n, (Fr*)d_out, s.stride, &O));
    SWM_LAUNCH(ctx, "rollup_link", rollup_link_kernel, dim3(1), dim3(RU_LANES), 0, O.roots + 8 * n, O.flags, O.status, (unsigned)n, s.stride,
               s.root_at, (Fr*)d_out, d_verdict);
    uint32_t table_verdict = 0, refused = 0;
    SWM_HIP(ctx, hipMemcpyAsync(&table_verdict, O.verdict, 4, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(&refused, d_verdict, 4, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (table_verdict) return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: the account table is not the tree's leaf level", what);
    SWM_HIP(ctx, hipMemcpyAsync(b.old_root, O.roots, 32, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(b.flags, O.flags, n, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(b.status, O.status, 4 * n, hipMemcpyDeviceToHost, ctx->stream));
    if (witness) SWM_HIP(ctx, hipMemcpyAsync(witness, d_out, w_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (refused) {  // all or nothing: the nodes as they were, the caller's table untouched
        SWM_HIP(ctx, hipMemcpyAsync(tree->d_nodes, d_snap, node_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        SWM_HIP(ctx, hipMemcpyAsync(b.new_root, O.roots + 8 * (2 * n - 1), 32, hipMemcpyDeviceToHost, ctx->stream));
        SWM_HIP(ctx, hipMemcpyAsync(accounts, d_accounts, table_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (refused) memcpy(b.new_root, b.old_root, 32);
    *applied = refused ? 0 : 1;
    *d_w = (Fr*)d_out;
    return SWM_OK;
}

// What both entries check before anything is queued; the block's shape on the way out.
template <class U>
int rollup_check(swm_ctx* ctx, const char* what, const typename U::Circuit* c, const typename U::Tree* tree, size_t count, RollupShape* s) {
    SWM_TRY(U::check_tree(ctx, what, c, tree));
    if (!rollup_shape(c->shape.num_witness, c->shape.num_constraints, count, s))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: %zu transfers in one block (%zu <= transfers <= %zu)", what, count,
                       (size_t)RU_MIN_TRANSFERS, (size_t)RU_MAX_TRANSFERS);
    if (s->num_witness * sizeof(Fr) > ctx->witness_stage_bytes)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: a block of %zu witness bytes, %zu at the most (a block is one vector: it is not chunked)",
                       what, s->num_witness * sizeof(Fr), ctx->witness_stage_bytes);
    return SWM_OK;
}

template <class U>
int rollup_witness_at(swm_ctx* ctx, const typename U::Circuit* c, typename U::Tree* tree, uint8_t* accounts_inout, const uint8_t* messages,
                      const uint8_t* signatures, size_t count, uint64_t* witness_out, uint8_t* old_root, uint8_t* new_root, uint8_t* flags,
                      uint32_t* status, int* applied) {
    const std::string what = std::string(U::name) + "_witness_at";
    if (!ctx || !c || !tree || !accounts_inout || !messages || !signatures || !witness_out || !old_root || !new_root || !flags || !status ||
        !applied)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what.c_str());
    *applied = 0;
    RollupShape s;
    SWM_TRY(rollup_check<U>(ctx, what.c_str(), c, tree, count, &s));
    const RollupBlock b = {messages, signatures, old_root, new_root, flags, status};
    Fr* d_w = nullptr;
    SWM_ON_DEVICE(ctx);
    return drained(ctx, rollup_pass<U>(ctx, what.c_str(), c, tree, accounts_inout, b, s, witness_out, &d_w, applied));
}

template <class U>
int rollup_prove_at(swm_ctx* ctx, const swm_pk* pk, const typename U::Circuit* c, typename U::Tree* tree, uint8_t* accounts_inout,
                    const uint8_t* messages, const uint8_t* signatures, size_t count, swm_rng* rng, unsigned prove_flags, uint8_t* proof_out,
                    size_t cap, size_t* len, uint8_t* old_root, uint8_t* new_root, uint8_t* flags, uint32_t* status, int* applied) {
    const std::string what = std::string(U::name) + "_prove_at";
    if (!ctx || !pk || !c || !tree || !accounts_inout || !messages || !signatures || !rng || !proof_out || !len || !old_root || !new_root ||
        !flags || !status || !applied)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what.c_str());
    *len = 0;
    *applied = 0;
    RollupShape s;
    SWM_TRY(rollup_check<U>(ctx, what.c_str(), c, tree, count, &s));
    // the tree is advanced before the proof is made: a key of another block size is refused while nothing has changed
    if (!pk_takes_shape(pk, s.num_instance, s.num_witness, s.num_constraints))
        return set_err(ctx, SWM_ERR_MISMATCH, "%s: the proving key is not that of a block of %zu transfers of this circuit", what.c_str(),
                       count);
    const RollupBlock b = {messages, signatures, old_root, new_root, flags, status};
    Fr* d_w = nullptr;
    {
        SWM_ON_DEVICE(ctx);
        SWM_TRY(drained(ctx, rollup_pass<U>(ctx, what.c_str(), c, tree, accounts_inout, b, s, nullptr, &d_w, applied)));
    }
    if (!*applied) return SWM_OK;  // rolled back: nothing to prove
    std::vector<Fr> inst(s.num_instance);
    Fr r0, r1;
    (void)ps_load_std(old_root, &r0);  // nodes of the tree: canonical
    (void)ps_load_std(new_root, &r1);
    inst[0] = fp_one<Fr>();
    inst[1] = fp_from_std(r0);
    inst[2] = fp_from_std(r1);
    for (size_t k = 0; k < count; k++) {
        const uint8_t* msg = messages + PY_MSG_LEN * k;
        uint64_t amount = 0;
        for (int i = 0; i < 8; i++) amount |= (uint64_t)msg[2 + i] << (8 * i);
        Fr* item = inst.data() + s.item_instance(k);
        item[0] = fp_from_u64<Fr>(msg[0]);
        item[1] = fp_from_u64<Fr>(msg[1]);
        item[2] = fp_from_u64<Fr>(amount);
    }
    return prove_device_witness(ctx, pk, s.num_instance, s.num_witness, s.num_constraints, inst.data(), d_w, rng, prove_flags, proof_out, cap,
                                len);
}

struct RollupUnit : PoseidonTransfers {
    static constexpr const char* name = "rollup";
};

struct PedersenRollupUnit : PedersenTransfers {
    static constexpr const char* name = "pedersen_rollup";
};

}  // namespace swm

using namespace swm;

extern "C" {

int swm_rollup_witness_at(swm_ctx* ctx, const swm_transfer_circuit* c, swm_poseidon_tree* tree, uint8_t* accounts_inout, const uint8_t* messages,
                          const uint8_t* signatures, size_t count, uint64_t* witness_out, uint8_t old_root[32], uint8_t new_root[32],
                          uint8_t* flags, uint32_t* status, int* applied) {
    return rollup_witness_at<RollupUnit>(ctx, c, tree, accounts_inout, messages, signatures, count, witness_out, old_root, new_root, flags, status,
                                         applied);
}

int swm_rollup_prove_at(swm_ctx* ctx, const swm_pk* pk, const swm_transfer_circuit* c, swm_poseidon_tree* tree, uint8_t* accounts_inout,
                        const uint8_t* messages, const uint8_t* signatures, size_t count, swm_rng* rng, unsigned prove_flags, uint8_t* proof_out,
                        size_t cap, size_t* len, uint8_t old_root[32], uint8_t new_root[32], uint8_t* flags, uint32_t* status, int* applied) {
    return rollup_prove_at<RollupUnit>(ctx, pk, c, tree, accounts_inout, messages, signatures, count, rng, prove_flags, proof_out, cap, len,
                                       old_root, new_root, flags, status, applied);
}

int swm_pedersen_rollup_witness_at(swm_ctx* ctx, const swm_pedersen_transfer_circuit* c, swm_merkle_tree* tree, uint8_t* accounts_inout,
                                   const uint8_t* messages, const uint8_t* signatures, size_t count, uint64_t* witness_out,
                                   uint8_t old_root[32], uint8_t new_root[32], uint8_t* flags, uint32_t* status, int* applied) {
    return rollup_witness_at<PedersenRollupUnit>(ctx, c, tree, accounts_inout, messages, signatures, count, witness_out, old_root, new_root, flags,
                                                 status, applied);
}

int swm_pedersen_rollup_prove_at(swm_ctx* ctx, const swm_pk* pk, const swm_pedersen_transfer_circuit* c, swm_merkle_tree* tree,
                                 uint8_t* accounts_inout, const uint8_t* messages, const uint8_t* signatures, size_t count, swm_rng* rng,
                                 unsigned prove_flags, uint8_t* proof_out, size_t cap, size_t* len, uint8_t old_root[32], uint8_t new_root[32],
                                 uint8_t* flags, uint32_t* status, int* applied) {
    return rollup_prove_at<PedersenRollupUnit>(ctx, pk, c, tree, accounts_inout, messages, signatures, count, rng, prove_flags, proof_out, cap,
                                               len, old_root, new_root, flags, status, applied);
}

}  // extern "C"

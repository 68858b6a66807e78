// ledger_witness_host.h — the host layer of the ledger circuits, written once for both account trees: a batch of payments
// (payment_witness.hip over the Poseidon tree, pedersen_payment_witness.hip over the Pedersen tree) and a block of transfers
// (transfer_witness.hip, pedersen_transfer_witness.hip).  A unit hands over a small struct U: its circuit and tree types, its
// launcher, its tree check, the name its entry points report errors under; the extern "C" functions are instantiations.
#pragma once
#include <string>
#include <vector>

#include "host/payment_shape.h"
#include "witness_host.h"

namespace swm {

// ---- payments: messages of 10 bytes, leaves of 72, whatever the tree hashes with.  U has
//   Circuit, Tree; name ("payment"); run(ctx, c, tree, d_msgs, d_sigs, d_sender_leaves, d_recipient_leaves, d_sender_sib,
//   d_recipient_sib, n, d_w, d_flags, d_status, d_roots_s, d_roots_r); check_tree(ctx, what, c, tree); root_node(tree)

// the host forms' checks: what the device form reports per item (the sibling arrays may be NULL)
int py_check(swm_ctx* ctx, const char* what, size_t height, const uint8_t* msgs, const uint8_t* sender_leaves, const uint8_t* sender_sib,
             const uint8_t* recipient_sib, size_t count);

struct PyStaged {
    const uint8_t *msgs, *sigs, *sender_leaves, *recipient_leaves, *sender_sib, *recipient_sib;
};
// signatures | sender leaves | recipient leaves | the two sibling arrays (may be NULL) | messages of n payments into "stage.a"
int py_stage(swm_ctx* ctx, size_t levels, const uint8_t* msgs, const uint8_t* sigs, const uint8_t* sender_leaves,
             const uint8_t* recipient_leaves, const uint8_t* sender_sib, const uint8_t* recipient_sib, size_t n, PyStaged* out);

struct PyOut {  // "payment.w": witnesses | sender roots | recipient roots | status | flags
    Fr* w;
    uint32_t *roots_s, *roots_r, *status;
    uint8_t* flags;
};
int py_out(swm_ctx* ctx, size_t num_witness, size_t n, PyOut* out);

// the prover over one item's device witnesses; public input one, root, sender, recipient, amount
int py_prove_item(swm_ctx* ctx, const swm_pk* pk, size_t num_witness, size_t num_constraints, const Fr& root_mont, const uint8_t* msg,
                  const Fr* d_w, swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len);
// a resident tree's root (d_root: its last node) in Montgomery form; synchronises the stream
int py_root_mont(swm_ctx* ctx, const uint8_t* d_root, Fr* root_mont);

// n payments staged and run; the results stay in "payment.w"
template <class U>
int payment_chunk(swm_ctx* ctx, const typename U::Circuit* c, const typename U::Tree* tree, const uint8_t* msgs, const uint8_t* sigs,
                  const uint8_t* sender_leaves, const uint8_t* recipient_leaves, const uint8_t* sender_sib, const uint8_t* recipient_sib, size_t n,
                  PyOut* out) {
    PyStaged in;
    SWM_TRY(py_stage(ctx, c->shape.levels, msgs, sigs, sender_leaves, recipient_leaves, sender_sib, recipient_sib, n, &in));
    SWM_TRY(py_out(ctx, c->shape.num_witness, n, out));
    return U::run(ctx, c, tree, in.msgs, in.sigs, in.sender_leaves, in.recipient_leaves, in.sender_sib, in.recipient_sib, n, out->w, out->flags,
                  out->status, out->roots_s, out->roots_r);
}

template <class U>
int payment_host(swm_ctx* ctx, const typename U::Circuit* c, const typename U::Tree* tree, const uint8_t* msgs, const uint8_t* sigs,
                 const uint8_t* sender_leaves, const uint8_t* recipient_leaves, const uint8_t* sender_sib, const uint8_t* recipient_sib,
                 size_t count, uint64_t* witness, uint8_t* flags, uint8_t* sender_roots, uint8_t* recipient_roots) {
    const size_t item = c->shape.num_witness * sizeof(Fr), sib = c->shape.levels * 32;
    for (const WitnessChunk ch : WitnessChunks(witness_stage_items(ctx, item), count)) {
        const size_t base = ch.base, n = ch.count;
        PyOut o;
        SWM_TRY(payment_chunk<U>(ctx, c, tree, msgs + PY_MSG_LEN * base, sigs + 64 * base, sender_leaves + PY_LEAF_LEN * base,
                                 recipient_leaves + PY_LEAF_LEN * base, sender_sib ? sender_sib + sib * base : nullptr,
                                 recipient_sib ? recipient_sib + sib * base : nullptr, n, &o));
        SWM_HIP(ctx, hipMemcpyAsync(reinterpret_cast<uint8_t*>(witness) + base * item, o.w, n * item, hipMemcpyDeviceToHost, ctx->stream));
        if (flags) SWM_HIP(ctx, hipMemcpyAsync(flags + base, o.flags, n, hipMemcpyDeviceToHost, ctx->stream));
        if (sender_roots) SWM_HIP(ctx, hipMemcpyAsync(sender_roots + 32 * base, o.roots_s, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
        if (recipient_roots) SWM_HIP(ctx, hipMemcpyAsync(recipient_roots + 32 * base, o.roots_r, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
        SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the staging buffers are reused by the next chunk
    }
    return SWM_OK;
}

template <class U>
int payment_witness(swm_ctx* ctx, const typename U::Circuit* c, const uint8_t* messages, const uint8_t* signatures, const uint8_t* sender_leaves,
                    const uint8_t* recipient_leaves, const uint8_t* sender_siblings, const uint8_t* recipient_siblings, size_t count,
                    uint64_t* witness, uint8_t* flags, uint8_t* sender_roots, uint8_t* recipient_roots) {
    const std::string what = std::string(U::name) + "_witness";
    if (!ctx || !c || (count && (!messages || !signatures || !sender_leaves || !recipient_leaves || !sender_siblings || !recipient_siblings || !witness)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what.c_str());
    if (!count) return SWM_OK;
    SWM_TRY(py_check(ctx, what.c_str(), c->shape.height, messages, sender_leaves, sender_siblings, recipient_siblings, count));
    SWM_ON_DEVICE(ctx);
    return drained(ctx, payment_host<U>(ctx, c, nullptr, messages, signatures, sender_leaves, recipient_leaves, sender_siblings, recipient_siblings,
                                        count, witness, flags, sender_roots, recipient_roots));
}

template <class U>
int payment_witness_at(swm_ctx* ctx, const typename U::Circuit* c, const typename U::Tree* tree, const uint8_t* messages, const uint8_t* signatures,
                       const uint8_t* sender_leaves, const uint8_t* recipient_leaves, size_t count, uint64_t* witness, uint8_t* flags) {
    const std::string what = std::string(U::name) + "_witness_at";
    if (!ctx || !c || !tree || (count && (!messages || !signatures || !sender_leaves || !recipient_leaves || !witness)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what.c_str());
    SWM_TRY(U::check_tree(ctx, what.c_str(), c, tree));
    if (!count) return SWM_OK;
    SWM_TRY(py_check(ctx, what.c_str(), c->shape.height, messages, sender_leaves, nullptr, nullptr, count));
    SWM_ON_DEVICE(ctx);
    return drained(ctx, payment_host<U>(ctx, c, tree, messages, signatures, sender_leaves, recipient_leaves, nullptr, nullptr, count, witness, flags,
                                        nullptr, nullptr));
}

template <class U>
int payment_witness_dev(swm_ctx* ctx, const typename U::Circuit* c, const typename U::Tree* tree, const void* d_messages, const void* d_signatures,
                        const void* d_sender_leaves, const void* d_recipient_leaves, const void* d_sender_siblings,
                        const void* d_recipient_siblings, size_t count, void* d_witness, void* d_flags, void* d_status, void* d_sender_roots,
                        void* d_recipient_roots) {
    const std::string what = std::string(U::name) + "_witness_dev";
    if (!ctx || !c || (count && (!d_messages || !d_signatures || !d_sender_leaves || !d_recipient_leaves || !d_witness || !d_flags || !d_status)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what.c_str());
    if (count && !tree && (!d_sender_siblings || !d_recipient_siblings))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: neither a tree nor two sibling arrays", what.c_str());
    if (tree) SWM_TRY(U::check_tree(ctx, what.c_str(), c, tree));
    if (((uintptr_t)d_signatures | (uintptr_t)d_sender_siblings | (uintptr_t)d_recipient_siblings | (uintptr_t)d_status |
         (uintptr_t)d_sender_roots | (uintptr_t)d_recipient_roots) & 3 || ((uintptr_t)d_witness & 15))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: signatures, siblings, status and roots must be 4-byte aligned, the witness 16-byte aligned",
                       what.c_str());
    SWM_ON_DEVICE(ctx);
    return U::run(ctx, c, tree, (const uint8_t*)d_messages, (const uint8_t*)d_signatures, (const uint8_t*)d_sender_leaves,
                  (const uint8_t*)d_recipient_leaves, (const uint8_t*)d_sender_siblings, (const uint8_t*)d_recipient_siblings, count, (Fr*)d_witness,
                  (uint8_t*)d_flags, (uint32_t*)d_status, (uint32_t*)d_sender_roots, (uint32_t*)d_recipient_roots);
}

template <class U>
int payment_prove_at(swm_ctx* ctx, const swm_pk* pk, const typename U::Circuit* c, const typename U::Tree* tree, const uint8_t* message,
                     const uint8_t* signature, const uint8_t* sender_leaf, const uint8_t* recipient_leaf, swm_rng* rng, unsigned flags,
                     uint8_t* proof_out, size_t cap, size_t* len) {
    const std::string what = std::string(U::name) + "_prove_at";
    if (!ctx || !pk || !c || !tree || !message || !signature || !sender_leaf || !recipient_leaf || !rng || !proof_out || !len)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what.c_str());
    SWM_TRY(U::check_tree(ctx, what.c_str(), c, tree));
    SWM_TRY(py_check(ctx, what.c_str(), c->shape.height, message, sender_leaf, nullptr, nullptr, 1));
    PyOut o;
    Fr root;
    {
        SWM_ON_DEVICE(ctx);
        SWM_TRY(drained(ctx, payment_chunk<U>(ctx, c, tree, message, signature, sender_leaf, recipient_leaf, nullptr, nullptr, 1, &o)));
        SWM_TRY(py_root_mont(ctx, U::root_node(tree), &root));  // its synchronisation: the inputs were staged from the caller's buffers
    }
    return py_prove_item(ctx, pk, c->shape.num_witness, c->shape.num_constraints, root, message, o.w, rng, flags, proof_out, cap, len);
}

template <class U>
int payment_prove_many_at(swm_ctx* ctx, const swm_pk* pk, const typename U::Circuit* c, const typename U::Tree* tree, const uint8_t* messages,
                          const uint8_t* signatures, const uint8_t* sender_leaves, const uint8_t* recipient_leaves, size_t count, swm_rng* rng,
                          unsigned flags, uint8_t* proofs_out, size_t proof_cap, size_t* lens, uint8_t* item_flags) {
    const std::string what = std::string(U::name) + "_prove_many_at";
    if (!ctx || !pk || !c || !tree || !rng || (count && (!messages || !signatures || !sender_leaves || !recipient_leaves || !proofs_out || !lens ||
                                                         !item_flags)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what.c_str());
    SWM_TRY(U::check_tree(ctx, what.c_str(), c, tree));
    if (!count) return SWM_OK;
    SWM_TRY(py_check(ctx, what.c_str(), c->shape.height, messages, sender_leaves, nullptr, nullptr, count));
    const size_t num_witness = c->shape.num_witness;
    for (size_t i = 0; i < count; i++) {  // whatever ends the call, every entry of the two arrays has been written
        lens[i] = 0;
        item_flags[i] = 0;
    }
    for (const WitnessChunk ch : WitnessChunks(witness_stage_items(ctx, num_witness * sizeof(Fr)), count)) {
        const size_t base = ch.base, n = ch.count;
        PyOut o;
        Fr root;
        {
            SWM_ON_DEVICE(ctx);
            SWM_TRY(drained(ctx, payment_chunk<U>(ctx, c, tree, messages + PY_MSG_LEN * base, signatures + 64 * base,
                                                  sender_leaves + PY_LEAF_LEN * base, recipient_leaves + PY_LEAF_LEN * base, nullptr, nullptr, n,
                                                  &o)));
            SWM_HIP(ctx, hipMemcpyAsync(item_flags + base, o.flags, n, hipMemcpyDeviceToHost, ctx->stream));
            SWM_TRY(py_root_mont(ctx, U::root_node(tree), &root));
        }
        for (size_t i = 0; i < n; i++) {
            if (item_flags[base + i] != 3) continue;  // reported, not proved: its system is unsatisfied
            size_t len = 0;
            const int rc = py_prove_item(ctx, pk, num_witness, c->shape.num_constraints, root, messages + PY_MSG_LEN * (base + i),
                                         o.w + i * num_witness, rng, flags, proofs_out + (base + i) * proof_cap, proof_cap, &len);
            if (rc == SWM_ERR_UNSATISFIED) continue;  // flags 3 and a leaf that is not the tree's: no proof, lens stays 0, the block goes on
            if (rc != SWM_OK) return rc;
            lens[base + i] = len;
        }
    }
    return SWM_OK;
}

// ---- a block of transfers, applied in order.  U has
//   Circuit, Tree; name ("transfer"); accounts_scratch ("transfer.accounts"); check_tree(ctx, what, c, tree);
//   chunk(ctx, what, c, tree, d_accounts, block, base, n, &d_w): chunk [base, base + n) staged, run, its small results copied into the
//   block's arrays and waited for, its witnesses left on the device at *d_w.  A unit's own: how it reports a refused table.

struct TransferBlock {  // the caller's arrays of a whole block; roots may be NULL
    const uint8_t *msgs, *sigs;
    uint8_t *old_roots, *new_roots, *flags;
    uint32_t* status;
};
static constexpr uint8_t TRANSFER_FLAG_APPLIED = 16;  // bit 4 of a transfer's flag byte: the table and the tree were advanced

// the prover over one transfer's device witnesses; public input one, old_root, new_root (32 canonical bytes each), sender,
// recipient, amount
int transfer_prove_item(swm_ctx* ctx, const swm_pk* pk, size_t num_witness, size_t num_constraints, const uint8_t* old_root, const uint8_t* new_root,
                        const uint8_t* msg, const Fr* d_w, swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len);

// the account table (2^levels leaves of 72 bytes) into the unit's scratch buffer
inline int transfer_upload_accounts(swm_ctx* ctx, const char* name, const uint8_t* accounts, size_t bytes, uint8_t** d_accounts) {
    SWM_TRY(scratch(ctx, name, bytes + 16, (void**)d_accounts));
    SWM_HIP(ctx, hipMemcpyAsync(*d_accounts, accounts, bytes, hipMemcpyHostToDevice, ctx->stream));
    return SWM_OK;
}

// The block in chunks.  witness (may be NULL): the host copy of every item; pk (may be NULL): one proof per applied transfer.
template <class U>
int transfer_block(swm_ctx* ctx, const char* what, const swm_pk* pk, const typename U::Circuit* c, typename U::Tree* tree, uint8_t* accounts,
                   const TransferBlock& b, size_t count, uint64_t* witness, swm_rng* rng, unsigned prove_flags, uint8_t* proofs_out,
                   size_t proof_cap, size_t* lens) {
    const size_t num_witness = c->shape.num_witness, item = num_witness * sizeof(Fr), table_bytes = PY_LEAF_LEN << c->shape.levels;
    std::vector<uint8_t> roots;  // the prover needs the root pairs whether the caller asked for them or not
    TransferBlock blk = b;
    if (pk && (!b.old_roots || !b.new_roots)) {
        roots.resize(64 * count);
        if (!b.old_roots) blk.old_roots = roots.data();
        if (!b.new_roots) blk.new_roots = roots.data() + 32 * count;
    }
    uint8_t* d_accounts = nullptr;
    {
        SWM_ON_DEVICE(ctx);
        SWM_TRY(drained(ctx, transfer_upload_accounts(ctx, U::accounts_scratch, accounts, table_bytes, &d_accounts)));
    }
    for (const WitnessChunk ch : WitnessChunks(witness_stage_items(ctx, item), count)) {
        Fr* d_w = nullptr;
        {
            SWM_ON_DEVICE(ctx);
            SWM_TRY(drained(ctx, U::chunk(ctx, what, c, tree, d_accounts, blk, ch.base, ch.count, &d_w)));
            // the tree is advanced from here on: the table goes back with it, whatever the prover does below
            SWM_HIP(ctx, hipMemcpyAsync(accounts, d_accounts, table_bytes, hipMemcpyDeviceToHost, ctx->stream));
            if (witness)
                SWM_HIP(ctx, hipMemcpyAsync(reinterpret_cast<uint8_t*>(witness) + ch.base * item, d_w, ch.count * item, hipMemcpyDeviceToHost,
                                            ctx->stream));
            SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        for (size_t i = ch.base; pk && i < ch.base + ch.count; i++) {
            if (!(blk.flags[i] & TRANSFER_FLAG_APPLIED)) continue;
            size_t len = 0;
            SWM_TRY(transfer_prove_item(ctx, pk, num_witness, c->shape.num_constraints, blk.old_roots + 32 * i, blk.new_roots + 32 * i,
                                        b.msgs + PY_MSG_LEN * i, d_w + (i - ch.base) * num_witness, rng, prove_flags,
                                        proofs_out + i * proof_cap, proof_cap, &len));
            lens[i] = len;
        }
    }
    return SWM_OK;
}

template <class U>
int transfer_witness_at(swm_ctx* ctx, const typename U::Circuit* c, typename U::Tree* tree, uint8_t* accounts_inout, const uint8_t* messages,
                        const uint8_t* signatures, size_t count, uint64_t* witnesses_out, uint8_t* old_roots, uint8_t* new_roots, uint8_t* flags,
                        uint32_t* status) {
    const std::string what = std::string(U::name) + "_witness_at";
    if (!ctx || !c || !tree || !accounts_inout ||
        (count && (!messages || !signatures || !witnesses_out || !old_roots || !new_roots || !flags || !status)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what.c_str());
    SWM_TRY(U::check_tree(ctx, what.c_str(), c, tree));
    if (!count) return SWM_OK;
    if (count > 0x7FFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: %zu transfers in one call", what.c_str(), count);
    const TransferBlock b = {messages, signatures, old_roots, new_roots, flags, status};
    return transfer_block<U>(ctx, what.c_str(), nullptr, c, tree, accounts_inout, b, count, witnesses_out, nullptr, 0, nullptr, 0, nullptr);
}

template <class U>
int transfer_prove_many_at(swm_ctx* ctx, const swm_pk* pk, const typename U::Circuit* c, typename U::Tree* tree, uint8_t* accounts_inout,
                           const uint8_t* messages, const uint8_t* signatures, size_t count, swm_rng* rng, unsigned prove_flags,
                           uint8_t* proofs_out, size_t proof_cap, size_t* lens, uint8_t* old_roots, uint8_t* new_roots, uint8_t* flags,
                           uint32_t* status) {
    const std::string what = std::string(U::name) + "_prove_many_at";
    if (!ctx || !pk || !c || !tree || !accounts_inout || !rng || (count && (!messages || !signatures || !proofs_out || !lens || !flags || !status)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what.c_str());
    SWM_TRY(U::check_tree(ctx, what.c_str(), c, tree));
    if (!count) return SWM_OK;
    if (count > 0x7FFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: %zu transfers in one call", what.c_str(), count);
    for (size_t i = 0; i < count; i++) {  // whatever ends the call, every entry has been written
        lens[i] = 0;
        flags[i] = 0;
        status[i] = 0;
    }
    const TransferBlock b = {messages, signatures, old_roots, new_roots, flags, status};
    return transfer_block<U>(ctx, what.c_str(), pk, c, tree, accounts_inout, b, count, nullptr, rng, prove_flags, proofs_out, proof_cap, lens);
}

}  // namespace swm

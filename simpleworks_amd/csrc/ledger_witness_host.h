// ledger_witness_host.h — the host layer of the ledger circuits, written once for both account trees: a batch of payments
// (payment_witness.hip over the Poseidon tree, pedersen_payment_witness.hip over the Pedersen tree), a block of transfers
// (transfer_witness.hip, pedersen_transfer_witness.hip) and a block of registrations and balance updates
// (account_update_witness.hip, pedersen_account_update_witness.hip).  A unit hands over a small struct U: its circuit and tree
// types, its launcher, its tree check, its scratch names, the name its entry points report errors under; the extern "C" functions
// are instantiations.  The two kinds of block share one loop (ledger_block) and one results step (block_results).
#pragma once
#include <string.h>

#include <string>
#include <vector>

#include "host/payment_shape.h"
#include "witness_host.h"

struct swm_poseidon;
struct swm_poseidon_tree;
struct swm_pedersen;
struct swm_merkle_tree;

namespace swm {

// ---- one check per tree family: a resident tree against a circuit's parameters and height, its leaves of 72 bytes
// (payment_witness.hip, pedersen_payment_witness.hip), and what a ledger circuit over the Pedersen tree asks of its two CRHs:
// windows of 4 bits, 144 of them for a leaf and 128 for two digests.  `what`: the entry point's name.
int ledger_check_tree(swm_ctx* ctx, const char* what, const swm_poseidon* params, size_t height, const swm_poseidon_tree* t);
int ledger_check_tree(swm_ctx* ctx, const char* what, const swm_pedersen* leaf, const swm_pedersen* inner, size_t height, const swm_merkle_tree* t);
int pedersen_tree_crh_check(swm_ctx* ctx, const char* what, const swm_pedersen* leaf, const swm_pedersen* inner);

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

// ---- a block, applied in order against a resident tree and an account table: what transfers and account updates share

struct BlockOut {  // the caller's result arrays of a whole block; roots may be NULL
    uint8_t *old_roots, *new_roots, *flags;
    uint32_t* status;
};

struct BlockRunOut {          // the small results of a unit's pass over n items, on the device (the unit's aux scratch)
    const uint32_t* roots;    // 2 x n x 8 words, canonical: old roots | new roots
    const uint8_t* flags;     // n
    const uint32_t* status;   // n
    const uint32_t* verdict;  // 1: nonzero when the table is not the tree's (then nothing else here is defined)
};

// The results step of chunk [base, base + n), verdict first on ONE wait: the verdict word, roots, status and flags are copied into
// host memory of this call's own and waited for; a refused table is reported before anything is written into the caller's arrays,
// which then hold what they held.  Otherwise roots, flags and status go on into the block's arrays.  leaves (may be NULL): takes the
// chunk's 2 x n x 72 leaf bytes in the same wait (the block loop's buffer, not the caller's).
inline int block_results(swm_ctx* ctx, const char* what, const BlockRunOut& O, const BlockOut& b, size_t base, size_t n,
                         const uint8_t* d_leaves = nullptr, uint8_t* leaves = nullptr) {
    std::vector<uint32_t> host(1 + n + 16 * n + (n + 3) / 4);  // verdict | status | old roots | new roots | flags
    uint32_t *status = host.data() + 1, *roots = status + n;
    uint8_t* flags = reinterpret_cast<uint8_t*>(roots + 16 * n);
    SWM_HIP(ctx, hipMemcpyAsync(host.data(), O.verdict, 4, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(status, O.status, 4 * n, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(roots, O.roots, 64 * n, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(flags, O.flags, n, hipMemcpyDeviceToHost, ctx->stream));
    if (leaves) SWM_HIP(ctx, hipMemcpyAsync(leaves, d_leaves, 2 * PY_LEAF_LEN * n, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (host[0]) return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: the account table is not the tree's leaf level", what);
    if (b.old_roots) memcpy(b.old_roots + 32 * base, roots, 32 * n);
    if (b.new_roots) memcpy(b.new_roots + 32 * base, roots + 8 * n, 32 * n);
    memcpy(b.flags + base, flags, n);
    memcpy(b.status + base, status, 4 * n);
    return SWM_OK;
}

// the account table (2^levels leaves of 72 bytes) into the unit's scratch buffer
inline int block_upload_accounts(swm_ctx* ctx, const char* name, const uint8_t* accounts, size_t bytes, uint8_t** d_accounts) {
    SWM_TRY(scratch(ctx, name, bytes + 16, (void**)d_accounts));
    SWM_HIP(ctx, hipMemcpyAsync(*d_accounts, accounts, bytes, hipMemcpyHostToDevice, ctx->stream));
    return SWM_OK;
}

// the table after a chunk and (witness not NULL) the chunk's witnesses back to the host, waited for
inline int block_download(swm_ctx* ctx, uint8_t* accounts, const uint8_t* d_accounts, size_t table_bytes, uint8_t* witness, const Fr* d_w,
                          size_t witness_bytes) {
    SWM_HIP(ctx, hipMemcpyAsync(accounts, d_accounts, table_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (witness) SWM_HIP(ctx, hipMemcpyAsync(witness, d_w, witness_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWM_OK;
}

// The block in chunks.  witness (may be NULL): the host copy of every item; pk (may be NULL): one proof per applied item.  K is the
// kind of block (TransferBlocks<U>, AccountUpdateBlocks<U> below) and has
//   Unit (its Circuit, Tree, accounts_scratch); Block, the caller's arrays with the BlockOut `out`; applied, the bit of a flag byte
//   that says the table and the tree were advanced; extra_bytes, the host bytes per item that a proof needs beside the block's arrays;
//   chunk(ctx, what, c, tree, d_accounts, block, base, n, &d_w, extra): chunk [base, base + n) staged, run, block_results, its
//   witnesses left on the device at *d_w, its extra bytes (extra not NULL) at extra;
//   prove_item(ctx, pk, c, block, i, extra, k, n, d_w, rng, flags, proof_out, cap, &len): item i of the block, item k of a chunk of n
template <class K>
int ledger_block(swm_ctx* ctx, const char* what, const swm_pk* pk, const typename K::Unit::Circuit* c, typename K::Unit::Tree* tree,
                 uint8_t* accounts, const typename K::Block& b, size_t count, uint64_t* witness, swm_rng* rng, unsigned prove_flags,
                 uint8_t* proofs_out, size_t proof_cap, size_t* lens) {
    const size_t num_witness = c->shape.num_witness, item = num_witness * sizeof(Fr), table_bytes = PY_LEAF_LEN << c->shape.levels;
    std::vector<uint8_t> roots, extra;  // the prover needs the root pairs whether the caller asked for them or not
    typename K::Block blk = b;
    if (pk && (!b.out.old_roots || !b.out.new_roots)) {
        roots.resize(64 * count);
        if (!b.out.old_roots) blk.out.old_roots = roots.data();
        if (!b.out.new_roots) blk.out.new_roots = roots.data() + 32 * count;
    }
    uint8_t* d_accounts = nullptr;
    {
        SWM_ON_DEVICE(ctx);
        SWM_TRY(drained(ctx, block_upload_accounts(ctx, K::Unit::accounts_scratch, accounts, table_bytes, &d_accounts)));
    }
    for (const WitnessChunk ch : WitnessChunks(witness_stage_items(ctx, item), count)) {
        Fr* d_w = nullptr;
        if (pk) extra.resize(K::extra_bytes * ch.count);
        {
            SWM_ON_DEVICE(ctx);
            SWM_TRY(drained(ctx, K::chunk(ctx, what, c, tree, d_accounts, blk, ch.base, ch.count, &d_w, pk ? extra.data() : nullptr)));
            // the tree is advanced from here on: the table goes back with it, whatever the prover does below
            SWM_TRY(drained(ctx, block_download(ctx, accounts, d_accounts, table_bytes,
                                                witness ? reinterpret_cast<uint8_t*>(witness) + ch.base * item : nullptr, d_w, ch.count * item)));
        }
        for (size_t i = ch.base; pk && i < ch.base + ch.count; i++) {
            if (!(blk.out.flags[i] & K::applied)) continue;
            const size_t k = i - ch.base;
            size_t len = 0;
            SWM_TRY(K::prove_item(ctx, pk, c, blk, i, extra.data(), k, ch.count, d_w + k * num_witness, rng, prove_flags,
                                  proofs_out + i * proof_cap, proof_cap, &len));
            lens[i] = len;
        }
    }
    return SWM_OK;
}

// what a prove_many_at writes before anything runs: whatever ends the call, every entry has been written
inline void block_clear(size_t count, size_t* lens, uint8_t* flags, uint32_t* status) {
    for (size_t i = 0; i < count; i++) {
        lens[i] = 0;
        flags[i] = 0;
        status[i] = 0;
    }
}

// ---- a block of transfers.  U has
//   Circuit, Tree; name ("transfer"); accounts_scratch ("transfer.accounts"), witness_scratch ("transfer.w");
//   check_tree(ctx, what, c, tree); run(ctx, c, tree, d_accounts, d_msgs, d_sigs, n, d_w, stride, &out), a BlockRunOut

struct TransferBlock {  // the caller's arrays of a whole block
    const uint8_t *msgs, *sigs;
    BlockOut out;
};
static constexpr uint8_t TRANSFER_FLAG_APPLIED = 16;  // bit 4 of a transfer's flag byte: the table and the tree were advanced

// the prover over one transfer's device witnesses; public input one, old_root, new_root (32 canonical bytes each), sender,
// recipient, amount
int transfer_prove_item(swm_ctx* ctx, const swm_pk* pk, size_t num_witness, size_t num_constraints, const uint8_t* old_root, const uint8_t* new_root,
                        const uint8_t* msg, const Fr* d_w, swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len);

template <class U>
struct TransferBlocks {  // what ledger_block drives
    using Unit = U;
    using Block = TransferBlock;
    static constexpr uint8_t applied = TRANSFER_FLAG_APPLIED;
    static constexpr size_t extra_bytes = 0;

    static int chunk(swm_ctx* ctx, const char* what, const typename U::Circuit* c, typename U::Tree* tree, uint8_t* d_accounts, const Block& b,
                     size_t base, size_t n, Fr** d_w, uint8_t*) {
        const size_t num_witness = c->shape.num_witness;
        uint8_t *d_in = nullptr, *d_out = nullptr;
        SWM_TRY(scratch(ctx, "stage.a", n * (64 + PY_MSG_LEN) + 16, (void**)&d_in));
        SWM_HIP(ctx, hipMemcpyAsync(d_in, b.sigs + 64 * base, 64 * n, hipMemcpyHostToDevice, ctx->stream));
        SWM_HIP(ctx, hipMemcpyAsync(d_in + 64 * n, b.msgs + PY_MSG_LEN * base, PY_MSG_LEN * n, hipMemcpyHostToDevice, ctx->stream));
        SWM_TRY(scratch(ctx, U::witness_scratch, n * num_witness * sizeof(Fr) + 16, (void**)&d_out));
        BlockRunOut O;
        SWM_TRY(U::run(ctx, c, tree, d_accounts, d_in + 64 * n, d_in, n, (Fr*)d_out, num_witness, &O));
        SWM_TRY(block_results(ctx, what, O, b.out, base, n));
        *d_w = (Fr*)d_out;
        return SWM_OK;
    }

    static int prove_item(swm_ctx* ctx, const swm_pk* pk, const typename U::Circuit* c, const Block& b, size_t i, const uint8_t*, size_t, size_t,
                          const Fr* d_w, swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len) {
        return transfer_prove_item(ctx, pk, c->shape.num_witness, c->shape.num_constraints, b.out.old_roots + 32 * i, b.out.new_roots + 32 * i,
                                   b.msgs + PY_MSG_LEN * i, d_w, rng, flags, proof_out, cap, len);
    }
};

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
    const TransferBlock b = {messages, signatures, {old_roots, new_roots, flags, status}};
    return ledger_block<TransferBlocks<U>>(ctx, what.c_str(), nullptr, c, tree, accounts_inout, b, count, witnesses_out, nullptr, 0, nullptr, 0,
                                           nullptr);
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
    block_clear(count, lens, flags, status);
    const TransferBlock b = {messages, signatures, {old_roots, new_roots, flags, status}};
    return ledger_block<TransferBlocks<U>>(ctx, what.c_str(), pk, c, tree, accounts_inout, b, count, nullptr, rng, prove_flags, proofs_out,
                                           proof_cap, lens);
}

// ---- a block of registrations and balance updates.  U has
//   Circuit, Tree; name ("account_update"); accounts_scratch ("account_update.accounts"), witness_scratch ("account_update.w");
//   check_tree(ctx, what, c, tree); run(ctx, c, tree, d_accounts, in, n, d_w, stride, &out): an AuIn, an AuOut (carved out of the
//   unit's third scratch buffer, "account_update.aux", by account_update_aux)

static constexpr unsigned AU_FLAG_APPLIED = 1;
static constexpr unsigned AU_ST_KEY = 1, AU_ST_ID = 2, AU_ST_OCCUPIED = 4, AU_ST_BLANK = 8, AU_ST_ZERO = 16;
static constexpr unsigned AU_KIND_REGISTER = 1;  // kinds[i]: 0 = set balance, 1 = register

struct AuIn {  // the block on the device, n = count
    const uint8_t *ids, *kinds, *keys, *balances;  // n | n | 64 n | 8 n bytes
};

struct AuOut {              // what the advance kernel leaves for the record launches and the bits kernel
    uint32_t* dig;          // 2 x n x (L + 1) x 8 words: the old path's nodes | the new leaf's walk
    uint32_t* sib;          // n x L x 8 words: one sibling array, it serves both
    uint8_t* leaves;        // 2 x n x 72 bytes: the old leaf as the circuit takes it | key || new_balance
    uint64_t* idx;          // n: the id masked to the tree
    uint32_t* roots;        // 2 x n x 8 words: old roots | new roots
    uint8_t* flags;         // n
    uint32_t* status;       // n
    uint32_t* verdict;      // 1: nonzero when the table is not the tree's
};

// the unit's aux scratch buffer `name` for n operations, carved: every piece a multiple of 8 bytes but the last two
inline int account_update_aux(swm_ctx* ctx, const char* name, size_t n, size_t levels, AuOut* O) {
    const size_t dig = 2 * n * (levels + 1) * 8, sib = n * levels * 8;
    uint8_t* aux = nullptr;
    SWM_TRY(scratch(ctx, name, 4 * (dig + sib) + 8 * n + 64 * n + 4 * n + 8 + 2 * PY_LEAF_LEN * n + n + 64, (void**)&aux));
    O->dig = reinterpret_cast<uint32_t*>(aux);
    O->sib = O->dig + dig;
    O->idx = reinterpret_cast<uint64_t*>(O->sib + sib);
    O->roots = reinterpret_cast<uint32_t*>(O->idx + n);
    O->status = O->roots + 16 * n;
    O->verdict = O->status + n;
    O->leaves = reinterpret_cast<uint8_t*>(O->verdict + 2);
    O->flags = O->leaves + 2 * PY_LEAF_LEN * n;
    return SWM_OK;
}

struct AccountUpdateBlock {  // the caller's arrays of a whole block
    const uint8_t *ids, *kinds, *keys, *balances;
    BlockOut out;
};

// the prover over one operation's device witnesses; public input one, old_root, new_root (32 canonical bytes each), id, key_x,
// key_y, old_balance, new_balance, fresh.  old_leaf, new_leaf: the 72 bytes the advance kernel left (account_update_witness.hip)
int account_update_prove_item(swm_ctx* ctx, const swm_pk* pk, size_t num_witness, size_t num_constraints, const uint8_t* old_root,
                              const uint8_t* new_root, unsigned id, unsigned kind, const uint8_t* old_leaf, const uint8_t* new_leaf, const Fr* d_w,
                              swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len);

template <class U>
struct AccountUpdateBlocks {  // what ledger_block drives
    using Unit = U;
    using Block = AccountUpdateBlock;
    static constexpr uint8_t applied = AU_FLAG_APPLIED;
    static constexpr size_t extra_bytes = 2 * PY_LEAF_LEN;  // a chunk's leaves: n old ones | n new ones, for the public input

    static int chunk(swm_ctx* ctx, const char* what, const typename U::Circuit* c, typename U::Tree* tree, uint8_t* d_accounts, const Block& b,
                     size_t base, size_t n, Fr** d_w, uint8_t* leaves) {
        const size_t num_witness = c->shape.num_witness;
        uint8_t *d_in = nullptr, *d_out = nullptr;
        SWM_TRY(scratch(ctx, "stage.a", n * (64 + 8 + 2) + 16, (void**)&d_in));
        const AuIn in = {d_in + 72 * n, d_in + 73 * n, d_in, d_in + 64 * n};
        SWM_HIP(ctx, hipMemcpyAsync(d_in, b.keys + 64 * base, 64 * n, hipMemcpyHostToDevice, ctx->stream));
        SWM_HIP(ctx, hipMemcpyAsync(d_in + 64 * n, b.balances + 8 * base, 8 * n, hipMemcpyHostToDevice, ctx->stream));
        SWM_HIP(ctx, hipMemcpyAsync(d_in + 72 * n, b.ids + base, n, hipMemcpyHostToDevice, ctx->stream));
        SWM_HIP(ctx, hipMemcpyAsync(d_in + 73 * n, b.kinds + base, n, hipMemcpyHostToDevice, ctx->stream));
        SWM_TRY(scratch(ctx, U::witness_scratch, n * num_witness * sizeof(Fr) + 16, (void**)&d_out));
        AuOut O;
        SWM_TRY(U::run(ctx, c, tree, d_accounts, in, n, (Fr*)d_out, num_witness, &O));
        SWM_TRY(block_results(ctx, what, BlockRunOut{O.roots, O.flags, O.status, O.verdict}, b.out, base, n, O.leaves, leaves));
        *d_w = (Fr*)d_out;
        return SWM_OK;
    }

    static int prove_item(swm_ctx* ctx, const swm_pk* pk, const typename U::Circuit* c, const Block& b, size_t i, const uint8_t* leaves, size_t k,
                          size_t n, const Fr* d_w, swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len) {
        return account_update_prove_item(ctx, pk, c->shape.num_witness, c->shape.num_constraints, b.out.old_roots + 32 * i,
                                         b.out.new_roots + 32 * i, b.ids[i], b.kinds[i], leaves + PY_LEAF_LEN * k, leaves + PY_LEAF_LEN * (n + k),
                                         d_w, rng, flags, proof_out, cap, len);
    }
};

// what both block entries refuse before anything runs
template <class U>
int account_update_check_block(swm_ctx* ctx, const char* what, const typename U::Circuit* c, const typename U::Tree* tree, const uint8_t* kinds,
                               size_t count) {
    SWM_TRY(U::check_tree(ctx, what, c, tree));
    if (count > 0x7FFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: %zu operations in one call", what, count);
    for (size_t i = 0; i < count; i++)
        if (kinds[i] > AU_KIND_REGISTER)
            return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: operation %zu: kind %u (0 = set balance, 1 = register)", what, i, (unsigned)kinds[i]);
    return SWM_OK;
}

template <class U>
int account_update_witness_at(swm_ctx* ctx, const typename U::Circuit* c, typename U::Tree* tree, uint8_t* accounts_inout, const uint8_t* ids,
                              const uint8_t* kinds, const uint8_t* keys_xy, const uint8_t* balances, size_t count, uint64_t* witnesses_out,
                              uint8_t* old_roots, uint8_t* new_roots, uint8_t* flags, uint32_t* status) {
    const std::string what = std::string(U::name) + "_witness_at";
    if (!ctx || !c || !tree || !accounts_inout ||
        (count && (!ids || !kinds || !keys_xy || !balances || !witnesses_out || !old_roots || !new_roots || !flags || !status)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what.c_str());
    SWM_TRY(account_update_check_block<U>(ctx, what.c_str(), c, tree, kinds, count));
    if (!count) return SWM_OK;
    const AccountUpdateBlock b = {ids, kinds, keys_xy, balances, {old_roots, new_roots, flags, status}};
    return ledger_block<AccountUpdateBlocks<U>>(ctx, what.c_str(), nullptr, c, tree, accounts_inout, b, count, witnesses_out, nullptr, 0, nullptr,
                                                0, nullptr);
}

template <class U>
int account_update_prove_many_at(swm_ctx* ctx, const swm_pk* pk, const typename U::Circuit* c, typename U::Tree* tree, uint8_t* accounts_inout,
                                 const uint8_t* ids, const uint8_t* kinds, const uint8_t* keys_xy, const uint8_t* balances, size_t count,
                                 swm_rng* rng, unsigned prove_flags, uint8_t* proofs_out, size_t proof_cap, size_t* lens, uint8_t* old_roots,
                                 uint8_t* new_roots, uint8_t* flags, uint32_t* status) {
    const std::string what = std::string(U::name) + "_prove_many_at";
    if (!ctx || !pk || !c || !tree || !accounts_inout || !rng ||
        (count && (!ids || !kinds || !keys_xy || !balances || !proofs_out || !lens || !flags || !status)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what.c_str());
    SWM_TRY(account_update_check_block<U>(ctx, what.c_str(), c, tree, kinds, count));
    // the tree is advanced before the proofs are made: a key of another shape is refused while nothing has changed
    if (!pk_takes_shape(pk, c->shape.num_instance, c->shape.num_witness, c->shape.num_constraints))
        return set_err(ctx, SWM_ERR_MISMATCH, "%s: the proving key is not that of this circuit", what.c_str());
    if (!count) return SWM_OK;
    block_clear(count, lens, flags, status);
    const AccountUpdateBlock b = {ids, kinds, keys_xy, balances, {old_roots, new_roots, flags, status}};
    return ledger_block<AccountUpdateBlocks<U>>(ctx, what.c_str(), pk, c, tree, accounts_inout, b, count, nullptr, rng, prove_flags, proofs_out,
                                                proof_cap, lens);
}

template <class U>
int account_update_prove_at(swm_ctx* ctx, const swm_pk* pk, const typename U::Circuit* c, typename U::Tree* tree, uint8_t* accounts_inout,
                            uint8_t id, uint8_t kind, const uint8_t* key_xy, uint64_t balance, swm_rng* rng, unsigned prove_flags,
                            uint8_t* proof_out, size_t cap, size_t* len, uint8_t* old_root, uint8_t* new_root, uint8_t* flag, uint32_t* status) {
    if (!key_xy || !proof_out || !len || !old_root || !new_root || !flag || !status)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s_prove_at: bad arguments", U::name);
    uint8_t b[8];
    for (int k = 0; k < 8; k++) b[k] = (uint8_t)(balance >> (8 * k));
    return account_update_prove_many_at<U>(ctx, pk, c, tree, accounts_inout, &id, &kind, key_xy, b, 1, rng, prove_flags, proof_out, cap, len,
                                           old_root, new_root, flag, status);
}

}  // namespace swm

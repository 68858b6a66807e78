// payment_witness.hip — the witness of the payment circuit, synthesised on the GPU, and the proof entries on top of it.  The
// statement is Transaction::validate of examples/simple-payments (transaction.rs:89-139) as one system over a Poseidon account
// tree: both leaves hash to the public root at the indices `sender` and `recipient`, the signature verifies under the sender
// leaf's key over sender || recipient || amount, and amount <= balance.  Order and values are those of
// simpleworks_amd/workloads.py, build_payment: that function is the specification, host/payment_shape.h the counts and offsets.
//
// The two large blocks are the existing circuits', written by their own kernels at their own offsets inside the payment's witness
// vector (witness_runs.h: the launchers take the item stride apart from the block's length).  A block of n payments is
//   prep      payment_prep_kernel     the 72-byte sender leaves unzipped into the 64-byte key array the Schnorr kernel reads, and
//                                     the two id bytes of each message as uint64 leaf indices, masked to the tree
//   schnorr   schnorr_witness_kernel  the Schnorr block, and whether the signature verifies
//   sender    walk | gather, record   the sender's membership block
//   recipient walk | gather, record   the recipient's membership block
//   bits      payment_bits_kernel     the 704 bit witnesses that belong to neither block, the flag byte, the refusals
// seven launches, whatever n.  The flag byte needs the Schnorr kernel's verdict, which is why the bits come last and the
// unzipping is a launch of its own before it.
// flag byte: bit 0 = the signature verifies, bit 1 = amount <= balance.  Every witness is written honestly whatever the flags say:
// a payment whose flags are not 3 gives an unsatisfied system (comparison rows of the Schnorr block, or the packing row).
// status (the device form; the host forms refuse the whole call): bit 0 = the sender's key is no canonical point of the curve
// (the Schnorr block of that item is cleared, nothing else of it), bit 1 = a sibling >= r, bit 2 = an id at or above 2^L (the
// membership blocks are then those of the id's low L bits).
#include <hip/hip_runtime.h>

#include <string.h>

#include <memory>
#include <vector>

#include "context.h"
#include "ff.cuh"
#include "host/payment_shape.h"
#include "ledger_bytes.cuh"
#include "poseidon.h"
#include "poseidon_tree.h"
#include "schnorr.h"
#include "swmarlin.h"
#include "ledger_witness_host.h"
#include "witness_runs.h"

struct swm_payment_circuit {
    swm_schnorr_circuit schnorr;      // over PY_MSG_LEN bytes
    swm_poseidon_tree_circuit tree;   // over PY_LEAF_LEN bytes
    swm::PaymentShape shape;
};

namespace swm {

static constexpr unsigned PY_LANES = 256;

// word i of the key array: 16 words per item out of the first 64 bytes of its sender leaf; the lane of word 0 also writes the
// item's two leaf indices
__global__ void __launch_bounds__(PY_LANES) payment_prep_kernel(const uint8_t* __restrict__ msgs, const uint8_t* __restrict__ sender_leaves,
                                                                size_t count, unsigned levels, uint32_t* __restrict__ keys,
                                                                uint64_t* __restrict__ sender_idx, uint64_t* __restrict__ recipient_idx) {
    const size_t i = blockIdx.x * (size_t)PY_LANES + threadIdx.x;
    if (i >= 16 * count) return;
    const size_t item = i >> 4;
    const unsigned word = (unsigned)(i & 15);
    const uint8_t* b = sender_leaves + PY_LEAF_LEN * item + 4 * word;
    keys[i] = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
    if (word == 0) {
        const uint64_t mask = ((uint64_t)1 << levels) - 1;
        sender_idx[item] = msgs[PY_MSG_LEN * item] & mask;
        recipient_idx[item] = msgs[PY_MSG_LEN * item + 1] & mask;
    }
}

struct PyArgs {
    size_t count, stride, balance_at, recipient_bits_at;
    unsigned levels;
};

__device__ __forceinline__ bool py_canonical(const uint32_t* p) {
    Fr x, r;
#pragma unroll
    for (int w = 0; w < 8; w++) {
        x.v[w] = p[w];
        r.v[w] = FrParams::P[w];
    }
    return fp_cmp_std(x, r) < 0;
}

// Element e (0 .. 703) of item p: 64 balance bits, 64 bits of (balance - amount) mod 2^64, 576 recipient leaf bits.  Adjacent
// lanes write adjacent elements, two 16-byte stores each.  The lane of element 0 writes the item's flag byte and completes its
// status word.  sender_siblings / recipient_siblings: NULL when they came from a resident tree.
__global__ void __launch_bounds__(PY_LANES) payment_bits_kernel(PyArgs A, const uint8_t* __restrict__ msgs, const uint8_t* __restrict__ sender_leaves,
                                                                const uint8_t* __restrict__ recipient_leaves,
                                                                const uint32_t* __restrict__ sender_siblings,
                                                                const uint32_t* __restrict__ recipient_siblings,
                                                                const uint8_t* __restrict__ sig_ok, Fr* __restrict__ witness,
                                                                uint8_t* __restrict__ flags, uint32_t* __restrict__ status) {
    const size_t i = blockIdx.x * (size_t)PY_LANES + threadIdx.x;
    if (i >= PY_BIT_WITNESSES * A.count) return;
    const size_t item = i / PY_BIT_WITNESSES;
    const unsigned e = (unsigned)(i % PY_BIT_WITNESSES);
    const uint8_t* msg = msgs + PY_MSG_LEN * item;
    unsigned bit;
    size_t at;
    if (e < 2 * PY_AMOUNT_BITS) {
        const uint64_t balance = le_load_u64(sender_leaves + PY_LEAF_LEN * item + 64), amount = le_load_u64(msg + 2);
        const uint64_t v = e < PY_AMOUNT_BITS ? balance : balance - amount;
        bit = (unsigned)(v >> (e & 63)) & 1u;
        at = A.balance_at + e;  // diff follows balance
        if (e == 0) {
            flags[item] = (uint8_t)((sig_ok[item] ? 1u : 0u) | (amount <= balance ? 2u : 0u));
            uint32_t st = status[item];  // bit 0: the Schnorr kernel's
            const size_t words = 8 * (size_t)A.levels;
            bool canonical = true;
            for (unsigned l = 0; l < A.levels; l++) {
                if (sender_siblings) canonical &= py_canonical(sender_siblings + item * words + 8 * l);
                if (recipient_siblings) canonical &= py_canonical(recipient_siblings + item * words + 8 * l);
            }
            if (!canonical) st |= 2u;
            if (((unsigned)msg[0] | (unsigned)msg[1]) >> A.levels) st |= 4u;
            status[item] = st;
        }
    } else {
        const unsigned k = e - 2 * (unsigned)PY_AMOUNT_BITS;
        bit = (recipient_leaves[PY_LEAF_LEN * item + (k >> 3)] >> (k & 7)) & 1u;
        at = A.recipient_bits_at + k;
    }
    const Fr v = bit ? fp_one<Fr>() : fp_zero<Fr>();
    uint4* q = reinterpret_cast<uint4*>(witness + item * A.stride + at);
    q[0] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
    q[1] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
}

int payment_prep_run(swm_ctx* ctx, const uint8_t* d_msgs, const uint8_t* d_sender_leaves, size_t n, unsigned levels, uint32_t* d_keys,
                     uint64_t* d_idx_s, uint64_t* d_idx_r) {
    SWM_LAUNCH(ctx, "payment_prep", payment_prep_kernel, dim3((unsigned)((16 * n + PY_LANES - 1) / PY_LANES)), dim3(PY_LANES), 0, d_msgs,
               d_sender_leaves, n, levels, d_keys, d_idx_s, d_idx_r);
    return SWM_OK;
}

int payment_bits_run(swm_ctx* ctx, size_t n, size_t stride, size_t balance_at, size_t recipient_bits_at, unsigned levels, const uint8_t* d_msgs,
                     const uint8_t* d_sender_leaves, const uint8_t* d_recipient_leaves, const uint32_t* d_sender_sib,
                     const uint32_t* d_recipient_sib, const uint8_t* d_sig_ok, Fr* d_w, uint8_t* d_flags, uint32_t* d_status) {
    PyArgs A;
    A.count = n;
    A.stride = stride;
    A.balance_at = balance_at;
    A.recipient_bits_at = recipient_bits_at;
    A.levels = levels;
    SWM_LAUNCH(ctx, "payment_bits", payment_bits_kernel, dim3((unsigned)((PY_BIT_WITNESSES * n + PY_LANES - 1) / PY_LANES)), dim3(PY_LANES), 0, A,
               d_msgs, d_sender_leaves, d_recipient_leaves, d_sender_sib, d_recipient_sib, d_sig_ok, d_w, d_flags, d_status);
    return SWM_OK;
}

// n payments on device buffers.  d_sigs and the siblings 4-byte aligned, d_witness 16-byte aligned.  tree: may be NULL, then the
// two sibling arrays are read and d_roots_s / d_roots_r (may be NULL) take the walked roots.  d_flags, d_status: per item.
static int py_run(swm_ctx* ctx, const swm_payment_circuit* c, const swm_poseidon_tree* tree, const uint8_t* d_msgs, const uint8_t* d_sigs,
                  const uint8_t* d_sender_leaves, const uint8_t* d_recipient_leaves, const uint8_t* d_sender_sib, const uint8_t* d_recipient_sib,
                  size_t n, Fr* d_w, uint8_t* d_flags, uint32_t* d_status, uint32_t* d_roots_s, uint32_t* d_roots_r) {
    if (!n) return SWM_OK;
    if (n > 0x7FFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "payment_witness: %zu payments in one call", n);
    const PaymentShape& s = c->shape;
    uint8_t* aux = nullptr;  // keys 64 n | sender indices 8 n | recipient indices 8 n | the Schnorr verdicts n
    SWM_TRY(scratch(ctx, "payment.aux", 81 * n + 16, (void**)&aux));
    uint32_t* d_keys = reinterpret_cast<uint32_t*>(aux);
    uint64_t* d_idx_s = reinterpret_cast<uint64_t*>(aux + 64 * n);
    uint64_t* d_idx_r = d_idx_s + n;
    uint8_t* d_sig_ok = aux + 80 * n;
    SWM_TRY(payment_prep_run(ctx, d_msgs, d_sender_leaves, n, (unsigned)s.levels, d_keys, d_idx_s, d_idx_r));
    SWM_TRY(schnorr_witness_run(ctx, &c->schnorr, aux, d_msgs, d_sigs, n, d_w, s.num_witness, d_sig_ok, d_status));
    SWM_TRY(ptw_run(ctx, &c->tree, tree, d_sender_leaves, d_idx_s, d_sender_sib, n, d_w + s.sender_at, s.num_witness, d_roots_s));
    SWM_TRY(ptw_run(ctx, &c->tree, tree, d_recipient_leaves, d_idx_r, d_recipient_sib, n, d_w + s.recipient_at, s.num_witness, d_roots_r));
    return payment_bits_run(ctx, n, s.num_witness, s.balance_at, s.recipient_bits_at, (unsigned)s.levels, d_msgs, d_sender_leaves,
                            d_recipient_leaves, tree ? nullptr : reinterpret_cast<const uint32_t*>(d_sender_sib),
                            tree ? nullptr : reinterpret_cast<const uint32_t*>(d_recipient_sib), d_sig_ok, d_w, d_flags, d_status);
}

// the host forms' checks: what the device form reports per item
int py_check(swm_ctx* ctx, const char* what, size_t height, const uint8_t* msgs, const uint8_t* sender_leaves,
                    const uint8_t* sender_sib, const uint8_t* recipient_sib, size_t count) {
    const size_t levels = height - 1;
    uint8_t key[64];
    Fr v;
    for (size_t p = 0; p < count; p++) {
        memcpy(key, sender_leaves + PY_LEAF_LEN * p, 64);
        if (schnorr_check_keys(ctx, key, 1) != SWM_OK)
            return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: item %zu: the sender's key is not a point of ed-on-BLS12-377", what, p);
        for (int k = 0; k < 2; k++)
            if ((size_t)msgs[PY_MSG_LEN * p + k] >> levels)
                return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: item %zu: account id %u in a tree of height %zu", what, p,
                               (unsigned)msgs[PY_MSG_LEN * p + k], height);
        for (int k = 0; k < 2; k++) {
            const uint8_t* sib = k ? recipient_sib : sender_sib;
            for (size_t l = 0; sib && l < levels; l++)
                if (!ps_load_std(sib + 32 * (p * levels + l), &v))
                    return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: item %zu: sibling %zu of the %s's path is not a canonical field element", what,
                                   p, l, k ? "recipient" : "sender");
        }
    }
    return SWM_OK;
}

int ledger_check_tree(swm_ctx* ctx, const char* what, const swm_poseidon* params, size_t height, const swm_poseidon_tree* t) {
    if (t->params != params || t->height != height || t->leaf_len != PY_LEAF_LEN)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: a tree of height %zu with %zu-byte leaves for a circuit of height %zu with %zu-byte leaves, "
                       "or other parameters", what, t->height, t->leaf_len, height, (size_t)PY_LEAF_LEN);
    return SWM_OK;
}

// signatures | sender leaves | recipient leaves | the two sibling arrays | messages of n payments into "stage.a": all but the
// messages stay word-aligned
int py_stage(swm_ctx* ctx, size_t levels, const uint8_t* msgs, const uint8_t* sigs, const uint8_t* sender_leaves,
                    const uint8_t* recipient_leaves, const uint8_t* sender_sib, const uint8_t* recipient_sib, size_t n, PyStaged* out) {
    const size_t sib = sender_sib ? n * levels * 32 : 0;
    uint8_t* d = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", n * (64 + 2 * PY_LEAF_LEN + PY_MSG_LEN) + 2 * sib + 16, (void**)&d));
    out->sigs = d;
    out->sender_leaves = d + 64 * n;
    out->recipient_leaves = out->sender_leaves + PY_LEAF_LEN * n;
    out->sender_sib = out->recipient_leaves + PY_LEAF_LEN * n;
    out->recipient_sib = out->sender_sib + sib;
    out->msgs = out->recipient_sib + sib;
    SWM_HIP(ctx, hipMemcpyAsync(d, sigs, 64 * n, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync((void*)out->sender_leaves, sender_leaves, PY_LEAF_LEN * n, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync((void*)out->recipient_leaves, recipient_leaves, PY_LEAF_LEN * n, hipMemcpyHostToDevice, ctx->stream));
    if (sib) {
        SWM_HIP(ctx, hipMemcpyAsync((void*)out->sender_sib, sender_sib, sib, hipMemcpyHostToDevice, ctx->stream));
        SWM_HIP(ctx, hipMemcpyAsync((void*)out->recipient_sib, recipient_sib, sib, hipMemcpyHostToDevice, ctx->stream));
    } else {
        out->sender_sib = out->recipient_sib = nullptr;
    }
    SWM_HIP(ctx, hipMemcpyAsync((void*)out->msgs, msgs, PY_MSG_LEN * n, hipMemcpyHostToDevice, ctx->stream));
    return SWM_OK;
}

// "payment.w" laid out for n payments of num_witness elements
int py_out(swm_ctx* ctx, size_t num_witness, size_t n, PyOut* out) {
    const size_t item = num_witness * sizeof(Fr);
    uint8_t* d_out = nullptr;
    SWM_TRY(scratch(ctx, "payment.w", n * (item + 64 + 4 + 1) + 16, (void**)&d_out));
    out->w = reinterpret_cast<Fr*>(d_out);
    out->roots_s = reinterpret_cast<uint32_t*>(d_out + n * item);
    out->roots_r = out->roots_s + 8 * n;
    out->status = out->roots_r + 8 * n;
    out->flags = reinterpret_cast<uint8_t*>(out->status + n);
    return SWM_OK;
}

// the prover over item `i` of a chunk's device witnesses; public input one, root, sender, recipient, amount
int py_prove_item(swm_ctx* ctx, const swm_pk* pk, size_t num_witness, size_t num_constraints, const Fr& root_mont, const uint8_t* msg,
                  const Fr* d_w, swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len) {
    uint64_t amount = 0;
    for (int k = 0; k < 8; k++) amount |= (uint64_t)msg[2 + k] << (8 * k);
    const Fr inst[5] = {fp_one<Fr>(), root_mont, fp_from_u64<Fr>(msg[0]), fp_from_u64<Fr>(msg[1]), fp_from_u64<Fr>(amount)};
    return prove_device_witness(ctx, pk, 5, num_witness, num_constraints, inst, d_w, rng, flags, proof_out, cap, len);
}

// the root of a resident tree (its last node, d_root) in Montgomery form; synchronises the stream
int py_root_mont(swm_ctx* ctx, const uint8_t* d_root, Fr* root_mont) {
    uint8_t root[32];
    SWM_HIP(ctx, hipMemcpyAsync(root, d_root, 32, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    Fr r;
    (void)ps_load_std(root, &r);  // a node of the tree is canonical
    *root_mont = fp_from_std(r);
    return SWM_OK;
}

struct PaymentUnit {  // what ledger_witness_host.h drives
    using Circuit = swm_payment_circuit;
    using Tree = swm_poseidon_tree;
    static constexpr const char* name = "payment";
    static constexpr auto run = py_run;
    static int check_tree(swm_ctx* ctx, const char* what, const Circuit* c, const Tree* t) {
        return ledger_check_tree(ctx, what, c->tree.params, c->shape.height, t);
    }
    static const uint8_t* root_node(const Tree* t) { return t->d_nodes + 32 * (t->num_nodes() - 1); }
};

}  // namespace swm

using namespace swm;

extern "C" {

int swm_payment_circuit_create(swm_ctx* ctx, const swm_schnorr* schnorr, const swm_poseidon* poseidon, size_t height, swm_payment_circuit** out) {
    if (!ctx || !schnorr || !poseidon || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "payment_circuit_create: bad arguments");
    PaymentShape shape;
    if (!payment_shape(poseidon->full_rounds, poseidon->partial_rounds, poseidon->alpha, height, schnorr->has_salt, &shape))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "payment_circuit_create: height %zu (%zu <= height <= %zu)", height, (size_t)PY_MIN_HEIGHT,
                       (size_t)PY_MAX_HEIGHT);
    std::unique_ptr<swm_payment_circuit> c(new swm_payment_circuit);
    c->schnorr.params = schnorr;
    c->schnorr.shape = shape.schnorr;
    c->tree.params = poseidon;
    c->tree.shape = shape.tree;
    c->shape = shape;
    *out = c.release();
    return SWM_OK;
}

void swm_payment_circuit_destroy(swm_ctx* ctx, swm_payment_circuit* c) { destroy_circuit(ctx, c); }

int swm_payment_witness(swm_ctx* ctx, const swm_payment_circuit* c, const uint8_t* messages, const uint8_t* signatures,
                        const uint8_t* sender_leaves, const uint8_t* recipient_leaves, const uint8_t* sender_siblings,
                        const uint8_t* recipient_siblings, size_t count, uint64_t* witness, uint8_t* flags, uint8_t* sender_roots,
                        uint8_t* recipient_roots) {
    return payment_witness<PaymentUnit>(ctx, c, messages, signatures, sender_leaves, recipient_leaves, sender_siblings, recipient_siblings, count,
                                        witness, flags, sender_roots, recipient_roots);
}

int swm_payment_witness_at(swm_ctx* ctx, const swm_payment_circuit* c, const swm_poseidon_tree* tree, const uint8_t* messages,
                           const uint8_t* signatures, const uint8_t* sender_leaves, const uint8_t* recipient_leaves, size_t count,
                           uint64_t* witness, uint8_t* flags) {
    return payment_witness_at<PaymentUnit>(ctx, c, tree, messages, signatures, sender_leaves, recipient_leaves, count, witness, flags);
}

int swm_payment_witness_dev(swm_ctx* ctx, const swm_payment_circuit* c, const swm_poseidon_tree* tree, const void* d_messages,
                            const void* d_signatures, const void* d_sender_leaves, const void* d_recipient_leaves,
                            const void* d_sender_siblings, const void* d_recipient_siblings, size_t count, void* d_witness, void* d_flags,
                            void* d_status, void* d_sender_roots, void* d_recipient_roots) {
    return payment_witness_dev<PaymentUnit>(ctx, c, tree, d_messages, d_signatures, d_sender_leaves, d_recipient_leaves, d_sender_siblings,
                                            d_recipient_siblings, count, d_witness, d_flags, d_status, d_sender_roots, d_recipient_roots);
}

int swm_payment_prove_at(swm_ctx* ctx, const swm_pk* pk, const swm_payment_circuit* c, const swm_poseidon_tree* tree, const uint8_t message[10],
                         const uint8_t signature[64], const uint8_t sender_leaf[72], const uint8_t recipient_leaf[72], swm_rng* rng,
                         unsigned flags, uint8_t* proof_out, size_t cap, size_t* len) {
    return payment_prove_at<PaymentUnit>(ctx, pk, c, tree, message, signature, sender_leaf, recipient_leaf, rng, flags, proof_out, cap, len);
}

int swm_payment_prove_many_at(swm_ctx* ctx, const swm_pk* pk, const swm_payment_circuit* c, const swm_poseidon_tree* tree,
                              const uint8_t* messages, const uint8_t* signatures, const uint8_t* sender_leaves, const uint8_t* recipient_leaves,
                              size_t count, swm_rng* rng, unsigned flags, uint8_t* proofs_out, size_t proof_cap, size_t* lens,
                              uint8_t* item_flags) {
    return payment_prove_many_at<PaymentUnit>(ctx, pk, c, tree, messages, signatures, sender_leaves, recipient_leaves, count, rng, flags,
                                              proofs_out, proof_cap, lens, item_flags);
}

}  // extern "C"

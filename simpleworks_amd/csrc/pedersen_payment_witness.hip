// pedersen_payment_witness.hip — the witness of the payment circuit over a PEDERSEN account tree, synthesised on the GPU, and the
// proof entries on top of it.  The statement is Transaction::validate of examples/simple-payments (transaction.rs:148-185) as one
// system over the reference's own tree (ledger.rs:54-88: a leaf CRH of 144 windows of 4 bits, one 72-byte AccountInformation
// exactly, and a two-to-one CRH of 128): both leaves hash to the public root at the indices `sender` and `recipient`, the
// signature verifies under the sender leaf's key over sender || recipient || amount, and amount <= balance.  Order and values are
// those of simpleworks_amd/workloads.py, build_pedersen_payment: that function is the specification,
// host/pedersen_payment_shape.h the counts and offsets.
//
// A path's hashes only look sequential: once the running digests cur_0 .. cur_L are known, the leaf hash and the L level hashes
// are independent of each other, and against a resident tree every cur_l already sits in the tree's nodes.  So a membership
// section is "digests, then record":
//   digests   with a resident tree a gather: cur_l = node[l][index >> l], sibling_l = node[l][(index >> l) ^ 1], no hash;
//             without one the walk of Path::verify (pedersen.cuh, as merkle_tree.hip walks), storing every level's digest.
//   record    ONE hash stage (merkle_stage.cuh) per workgroup, its input read from memory, never from the stage below: the leaf
//             stages at 192 lanes (144 windows, three waves), the level stages at 128 (128 windows, two waves), a launch each, so
//             that no level stage idles a third wave.
// A block of n payments is
//   prep      payment_prep_kernel     (payment_witness.hip) the key array of the Schnorr kernel, the two masked leaf indices
//   schnorr   schnorr_witness_kernel  the Schnorr block, and whether the signature verifies
//   digests   pp_gather | pp_walk     both sides of every payment in one launch
//   leaves    pp_record_leaf_kernel   2 n workgroups: the leaf hash of each side
//   levels    pp_record_level_kernel  2 n L workgroups: dir | sibling | left | 512 bits | the level's hash
//   bits      payment_bits_kernel     (payment_witness.hip) the 704 bit witnesses, the flag byte, the refusals
// six launches, whatever n.  No atomics, no cooperative launch; stream order is the only ordering.  The two record kernels take
// their sections as arguments (witness_runs.h: PpArgs, pp_record_run): two per payment here, four per transfer in
// pedersen_transfer_witness.hip, whose update sections are the level stage's update flavour.
// flag byte, status: those of payment_witness.hip.  With a resident tree nothing compares the leaves with the tree: a leaf that is
// not the tree's records a satisfied leaf hash and a level 0 whose `left` is the tree's digest, so that level's select row fails:
// the honest witness of a false statement, which the prover reports.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>

#include "context.h"
#include "ff.cuh"
#include "host/pedersen_payment_shape.h"
#include "merkle_nodes.cuh"
#include "merkle_stage.cuh"
#include "merkle_tree.h"
#include "pedersen.cuh"
#include "pedersen.h"
#include "schnorr.h"
#include "swmarlin.h"
#include "ledger_witness_host.h"
#include "witness_runs.h"

struct swm_pedersen_payment_circuit {
    swm_schnorr_circuit schnorr;  // over PP_MSG_LEN bytes
    const swm_pedersen* leaf = nullptr;
    const swm_pedersen* inner = nullptr;
    swm::PedersenPaymentShape shape;
};

namespace swm {

static constexpr unsigned PP_LEAF_LANES = 192, PP_LEVEL_LANES = 128;

// Path q = 2 item + side (side 1: the recipient).  digests: cur_0 .. cur_L of path q at 8 (q (L + 1) + l); siblings: the
// sender's n x L x 8 words, then the recipient's.  The indices are masked to L bits (payment_prep_kernel): every read is a node.
__global__ void __launch_bounds__(256) pp_gather_kernel(const uint32_t* __restrict__ nodes, unsigned levels, const uint64_t* __restrict__ idx_s,
                                                        const uint64_t* __restrict__ idx_r, size_t count, uint32_t* __restrict__ digests,
                                                        uint32_t* __restrict__ siblings) {
    const size_t dig_words = 2 * count * (levels + 1) * 8, side_words = count * levels * 8, words = dig_words + 2 * side_words;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
        const bool sib = i >= dig_words;
        const size_t k = sib ? i - dig_words : i;
        size_t item;
        unsigned side, l;
        if (sib) {
            side = k >= side_words ? 1u : 0u;
            const size_t s = (k - side * side_words) >> 3;
            item = s / levels;
            l = (unsigned)(s % levels);
        } else {
            const size_t s = k >> 3, q = s / (levels + 1);
            item = q >> 1;
            side = (unsigned)(q & 1);
            l = (unsigned)(s % (levels + 1));
        }
        const uint64_t at = ((side ? idx_r : idx_s)[item] >> l) ^ (sib ? 1u : 0u);
        const uint32_t v = nodes[8 * (mt_level_offset(levels, l) + at) + (k & 7)];
        if (sib) siblings[k] = v;
        else digests[k] = v;
    }
}

// Path::verify's walk for the 2 n paths of n payments, `lanes` lanes each, every level's digest stored.  roots_s / roots_r (may
// be NULL): cur_L of each side.
__global__ void __launch_bounds__(256) pp_walk_kernel(const EdRow* __restrict__ leaf_table, unsigned leaf_windows, const EdRow* __restrict__ inner_table,
                                                      unsigned inner_windows, unsigned levels, const uint8_t* __restrict__ sender_leaves,
                                                      const uint8_t* __restrict__ recipient_leaves, const uint64_t* __restrict__ idx_s,
                                                      const uint64_t* __restrict__ idx_r, const uint32_t* __restrict__ sib_s,
                                                      const uint32_t* __restrict__ sib_r, size_t count, unsigned lanes, Fr k2d,
                                                      uint32_t* __restrict__ digests, uint32_t* __restrict__ roots_s,
                                                      uint32_t* __restrict__ roots_r) {
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t q = gid / lanes;
    const unsigned lane = (unsigned)(gid % lanes);
    const int head = (int)((threadIdx.x & 63u) & ~(lanes - 1u));  // the group's lane 0 within the wave
    const bool live = q < 2 * count;
    const size_t item = live ? q >> 1 : 0;
    const bool side = q & 1;
    const uint64_t index = (side ? idx_r : idx_s)[item];
    const uint32_t* sib = (side ? sib_r : sib_s) + item * (size_t)levels * 8;

    EdExt acc = ed_identity();
    if (live) {
        const uint8_t* msg = (side ? recipient_leaves : sender_leaves) + item * PP_LEAF_LEN;
        acc = ped_partial(leaf_table, leaf_windows, 4, [msg](size_t i) { return (unsigned)msg[i]; }, PP_LEAF_LEN, lanes, lane);
    }
    uint32_t cur[8];
#pragma unroll 1
    for (unsigned l = 0;; l++) {
        acc = ped_join(acc, lanes, k2d);
        Fr x = fp_zero<Fr>();
        if (lane == 0) {
            x = ped_digest(acc);
            if (live) {
                uint32_t* o = digests + 8 * (q * (levels + 1) + l);
#pragma unroll
                for (int i = 0; i < 8; i++) o[i] = x.v[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 8; i++) cur[i] = (uint32_t)__shfl((int)x.v[i], head, 64);
        if (l == levels) break;
        const bool right = (index >> l) & 1u;  // the running digest is the right child
        MtMsg64 m;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t s = live ? sib[8 * l + i] : 0u;
            m.w[i] = right ? s : cur[i];
            m.w[8 + i] = right ? cur[i] : s;
        }
        acc = ped_partial(inner_table, inner_windows, 4, m, 64, lanes, lane);
    }
    uint32_t* roots = side ? roots_r : roots_s;
    if (live && lane == 0 && roots) {
#pragma unroll
        for (int i = 0; i < 8; i++) roots[8 * item + i] = cur[i];
    }
}

// Workgroup item x sections + k: the leaf hash of section k of that item (witness_runs.h: PpArgs), 144 windows on 192 lanes.
__global__ void __launch_bounds__(PP_LEAF_LANES) pp_record_leaf_kernel(const EdRow* __restrict__ leaf_table, PpArgs A, Fr* __restrict__ witness,
                                                                       Fr k2d, Fr half) {
    __shared__ MwStage<3> sh;
    const unsigned tid = threadIdx.x;
    const size_t item = blockIdx.x / A.sections;
    const PpSection& S = A.s[blockIdx.x % A.sections];
    const uint8_t* leaf = S.leaves + item * PP_LEAF_LEN;
    const unsigned nib = tid < PP_LEAF_WINDOWS ? (leaf[tid >> 1] >> (4 * (tid & 1))) & 15u : 0u;
    mw_hash_stage<3>(leaf_table, nib, (unsigned)PP_LEAF_BITS, witness + item * A.stride + S.at, k2d, half, sh);
}

// Workgroup (item x sections + k) L + l: level l of section k of that item, 128 windows on 128 lanes.  dir | sibling | left | the
// 512 bits of left || right | the hash's witnesses, from cur_l and the sibling as they stand in memory.  An update section's level
// has no dir and no sibling of its own: left, the bits and the hash's witnesses sit two elements earlier.
__global__ void __launch_bounds__(PP_LEVEL_LANES) pp_record_level_kernel(const EdRow* __restrict__ inner_table, PpArgs A, Fr* __restrict__ witness,
                                                                         Fr k2d, Fr half) {
    __shared__ MwStage<2> sh;
    __shared__ uint32_t bits[16];  // left || right, canonical little-endian words
    const unsigned tid = threadIdx.x;
    const size_t q = blockIdx.x / A.levels, item = q / A.sections;
    const unsigned l = blockIdx.x % A.levels;
    const PpSection& S = A.s[q % A.sections];
    const unsigned dir = (unsigned)(S.idx[item] >> l) & 1u;
    const uint32_t* sib = S.sib + 8 * (item * A.levels + l);
    const uint32_t* cur = S.dig + item * A.dig_stride + 8 * l;
    if (tid < 8) {  // left = dir ? sibling : cur, right = the other one
        const uint32_t s = sib[tid], c = cur[tid];
        bits[tid] = dir ? s : c;
        bits[8 + tid] = dir ? c : s;
    }
    __syncthreads();
    const Fr one = fp_one<Fr>(), zero = fp_zero<Fr>();
    const bool update = S.update != 0;
    // lw: where this level's dir would be; an update level starts at its left, lw + 2
    Fr* lw = witness + item * A.stride + S.at + PP_LEAF_WITNESSES + (update ? MW_LEVEL_WITNESSES - 2 : MW_LEVEL_WITNESSES) * (size_t)l -
             (update ? 2 : 0);
    if (tid == 0) {
        Fr s, left;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            s.v[i] = sib[i];
            left.v[i] = bits[i];
        }
        if (!update) {
            lw[0] = dir ? one : zero;
            lw[1] = fp_from_std(s);
        }
        lw[2] = fp_from_std(left);
    }
    for (unsigned i = tid; i < 2 * MW_DIGEST_BITS; i += PP_LEVEL_LANES) lw[MW_LEVEL_BITS_AT + i] = (bits[i >> 5] >> (i & 31)) & 1u ? one : zero;
    const unsigned nib = (bits[tid >> 3] >> (4 * (tid & 7))) & 15u;
    mw_hash_stage<2>(inner_table, nib, 2 * (unsigned)MW_DIGEST_BITS, lw + MW_LEVEL_ADDS_AT, k2d, half, sh);
}

static const EdRow* pp_rows(const swm_pedersen* p) { return reinterpret_cast<const EdRow*>(p->d_table); }

int pp_record_run(swm_ctx* ctx, const swm_pedersen* leaf, const swm_pedersen* inner, const PpArgs& A, size_t n, Fr* d_w) {
    const Fr k2d = fp_from_u64<Fr>(2 * ED_D), half = fp_inv(fp_from_u64<Fr>(2));
    SWM_LAUNCH(ctx, "pedersen_payment_leaves", pp_record_leaf_kernel, dim3((unsigned)(A.sections * n)), dim3(PP_LEAF_LANES), 0, pp_rows(leaf), A,
               d_w, k2d, half);
    SWM_LAUNCH(ctx, "pedersen_payment_levels", pp_record_level_kernel, dim3((unsigned)(A.sections * n * A.levels)), dim3(PP_LEVEL_LANES), 0,
               pp_rows(inner), A, d_w, k2d, half);
    return SWM_OK;
}

// n payments on device buffers.  d_sigs and the siblings 4-byte aligned, d_witness 16-byte aligned.  tree: may be NULL, then the
// two sibling arrays are read and d_roots_s / d_roots_r (may be NULL) take the walked roots.  d_flags, d_status: per item.
static int pp_run(swm_ctx* ctx, const swm_pedersen_payment_circuit* c, const swm_merkle_tree* tree, const uint8_t* d_msgs, const uint8_t* d_sigs,
                  const uint8_t* d_sender_leaves, const uint8_t* d_recipient_leaves, const uint8_t* d_sender_sib, const uint8_t* d_recipient_sib,
                  size_t n, Fr* d_w, uint8_t* d_flags, uint32_t* d_status, uint32_t* d_roots_s, uint32_t* d_roots_r) {
    if (!n) return SWM_OK;
    if (n > 0x7FFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "pedersen_payment_witness: %zu payments in one call", n);
    const PedersenPaymentShape& s = c->shape;
    const unsigned levels = (unsigned)s.levels;
    uint8_t* aux = nullptr;  // keys 64 n | sender indices 8 n | recipient indices 8 n | the Schnorr verdicts n
    SWM_TRY(scratch(ctx, "payment.aux", 81 * n + 16, (void**)&aux));
    uint32_t* d_keys = reinterpret_cast<uint32_t*>(aux);
    uint64_t* d_idx_s = reinterpret_cast<uint64_t*>(aux + 64 * n);
    uint64_t* d_idx_r = d_idx_s + n;
    uint8_t* d_sig_ok = aux + 80 * n;
    const size_t dig_words = 2 * n * (levels + 1) * 8, side_words = n * levels * 8;
    uint32_t* d_dig = nullptr;  // the digests of both sides | with a tree, the sender's and the recipient's siblings
    SWM_TRY(scratch(ctx, "ptree.digests", (dig_words + 2 * side_words) * 4, (void**)&d_dig));
    SWM_TRY(payment_prep_run(ctx, d_msgs, d_sender_leaves, n, levels, d_keys, d_idx_s, d_idx_r));
    SWM_TRY(schnorr_witness_run(ctx, &c->schnorr, aux, d_msgs, d_sigs, n, d_w, s.num_witness, d_sig_ok, d_status));
    const uint32_t *d_sib_s = reinterpret_cast<const uint32_t*>(d_sender_sib), *d_sib_r = reinterpret_cast<const uint32_t*>(d_recipient_sib);
    if (tree) {
        const size_t words = dig_words + 2 * side_words;
        const unsigned blocks = (unsigned)std::min<size_t>((words + 255) / 256, 1u << 16);
        SWM_LAUNCH(ctx, "pedersen_payment_gather", pp_gather_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<const uint32_t*>(tree->d_nodes),
                   levels, (const uint64_t*)d_idx_s, (const uint64_t*)d_idx_r, n, d_dig, d_dig + dig_words);
        d_sib_s = d_dig + dig_words;
        d_sib_r = d_sib_s + side_words;
    } else {
        const unsigned lanes = lanes_for(2 * n);
        SWM_LAUNCH(ctx, "pedersen_payment_walk", pp_walk_kernel, dim3((unsigned)((2 * n * lanes + 255) / 256)), dim3(256), 0, pp_rows(c->leaf),
                   c->leaf->num_windows, pp_rows(c->inner), c->inner->num_windows, levels, d_sender_leaves, d_recipient_leaves,
                   (const uint64_t*)d_idx_s, (const uint64_t*)d_idx_r, d_sib_s, d_sib_r, n, lanes, fp_from_u64<Fr>(2 * ED_D), d_dig, d_roots_s,
                   d_roots_r);
    }
    PpArgs A = {};
    A.stride = s.num_witness;
    A.dig_stride = 2 * (size_t)(levels + 1) * 8;  // path q = 2 item + side
    A.levels = levels;
    A.sections = 2;
    A.s[0] = {d_sender_leaves, d_dig, d_sib_s, d_idx_s, s.sender_at, 0u};
    A.s[1] = {d_recipient_leaves, d_dig + (size_t)(levels + 1) * 8, d_sib_r, d_idx_r, s.recipient_at, 0u};
    SWM_TRY(pp_record_run(ctx, c->leaf, c->inner, A, n, d_w));
    return payment_bits_run(ctx, n, s.num_witness, s.balance_at, s.recipient_bits_at, levels, d_msgs, d_sender_leaves, d_recipient_leaves,
                            tree ? nullptr : d_sib_s, tree ? nullptr : d_sib_r, d_sig_ok, d_w, d_flags, d_status);
}

int ledger_check_tree(swm_ctx* ctx, const char* what, const swm_pedersen* leaf, const swm_pedersen* inner, size_t height, const swm_merkle_tree* t) {
    if (t->leaf != leaf || t->inner != inner || t->height != height || t->leaf_len != PP_LEAF_LEN)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: a tree of height %zu with %zu-byte leaves for a circuit of height %zu with %zu-byte leaves, "
                       "or other parameters", what, t->height, t->leaf_len, height, (size_t)PP_LEAF_LEN);
    return SWM_OK;
}

int pedersen_tree_crh_check(swm_ctx* ctx, const char* what, const swm_pedersen* leaf, const swm_pedersen* inner) {
    if (leaf->window_size != 4 || inner->window_size != 4)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: windows of %u and %u bits (4 is required)", what, leaf->window_size, inner->window_size);
    if (leaf->num_windows < PP_LEAF_WINDOWS || inner->num_windows < PP_INNER_WINDOWS)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: %u leaf and %u two-to-one windows (at least %zu and %zu are required)", what,
                       leaf->num_windows, inner->num_windows, (size_t)PP_LEAF_WINDOWS, (size_t)PP_INNER_WINDOWS);
    return SWM_OK;
}

static_assert(PP_MSG_LEN == PY_MSG_LEN && PP_LEAF_LEN == PY_LEAF_LEN, "the payment driver's message and leaf");

struct PedersenPaymentUnit {  // what ledger_witness_host.h drives
    using Circuit = swm_pedersen_payment_circuit;
    using Tree = swm_merkle_tree;
    static constexpr const char* name = "pedersen_payment";
    static constexpr auto run = pp_run;
    static int check_tree(swm_ctx* ctx, const char* what, const Circuit* c, const Tree* t) {
        return ledger_check_tree(ctx, what, c->leaf, c->inner, c->shape.height, t);
    }
    static const uint8_t* root_node(const Tree* t) { return t->d_nodes + 32 * (t->num_nodes() - 1); }
};

}  // namespace swm

using namespace swm;

extern "C" {

int swm_pedersen_payment_circuit_create(swm_ctx* ctx, const swm_schnorr* schnorr, const swm_pedersen* leaf, const swm_pedersen* inner,
                                        size_t height, swm_pedersen_payment_circuit** out) {
    if (!ctx || !schnorr || !leaf || !inner || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "pedersen_payment_circuit_create: bad arguments");
    PedersenPaymentShape shape;
    if (!pedersen_payment_shape(height, schnorr->has_salt, &shape))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "pedersen_payment_circuit_create: height %zu (%zu <= height <= %zu)", height,
                       (size_t)PP_MIN_HEIGHT, (size_t)PP_MAX_HEIGHT);
    SWM_TRY(pedersen_tree_crh_check(ctx, "pedersen_payment_circuit_create", leaf, inner));
    std::unique_ptr<swm_pedersen_payment_circuit> c(new swm_pedersen_payment_circuit);
    c->schnorr.params = schnorr;
    c->schnorr.shape = shape.schnorr;
    c->leaf = leaf;
    c->inner = inner;
    c->shape = shape;
    *out = c.release();
    return SWM_OK;
}

void swm_pedersen_payment_circuit_destroy(swm_ctx* ctx, swm_pedersen_payment_circuit* c) { destroy_circuit(ctx, c); }

int swm_pedersen_payment_witness(swm_ctx* ctx, const swm_pedersen_payment_circuit* c, const uint8_t* messages, const uint8_t* signatures,
                                 const uint8_t* sender_leaves, const uint8_t* sender_siblings, const uint8_t* recipient_leaves,
                                 const uint8_t* recipient_siblings, size_t count, uint64_t* witness, uint8_t* flags, uint8_t* sender_roots,
                                 uint8_t* recipient_roots) {
    return payment_witness<PedersenPaymentUnit>(ctx, c, messages, signatures, sender_leaves, recipient_leaves, sender_siblings, recipient_siblings,
                                                count, witness, flags, sender_roots, recipient_roots);
}

int swm_pedersen_payment_witness_at(swm_ctx* ctx, const swm_pedersen_payment_circuit* c, const swm_merkle_tree* tree, const uint8_t* messages,
                                    const uint8_t* signatures, const uint8_t* sender_leaves, const uint8_t* recipient_leaves, size_t count,
                                    uint64_t* witness, uint8_t* flags) {
    return payment_witness_at<PedersenPaymentUnit>(ctx, c, tree, messages, signatures, sender_leaves, recipient_leaves, count, witness, flags);
}

int swm_pedersen_payment_witness_dev(swm_ctx* ctx, const swm_pedersen_payment_circuit* c, const swm_merkle_tree* tree, const void* d_messages,
                                     const void* d_signatures, const void* d_sender_leaves, const void* d_recipient_leaves,
                                     const void* d_sender_siblings, const void* d_recipient_siblings, size_t count, void* d_witness,
                                     void* d_flags, void* d_status, void* d_sender_roots, void* d_recipient_roots) {
    return payment_witness_dev<PedersenPaymentUnit>(ctx, c, tree, d_messages, d_signatures, d_sender_leaves, d_recipient_leaves, d_sender_siblings,
                                                    d_recipient_siblings, count, d_witness, d_flags, d_status, d_sender_roots,
                                                    d_recipient_roots);
}

int swm_pedersen_payment_prove_at(swm_ctx* ctx, const swm_pk* pk, const swm_pedersen_payment_circuit* c, const swm_merkle_tree* tree,
                                  const uint8_t message[10], const uint8_t signature[64], const uint8_t sender_leaf[72],
                                  const uint8_t recipient_leaf[72], swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len) {
    return payment_prove_at<PedersenPaymentUnit>(ctx, pk, c, tree, message, signature, sender_leaf, recipient_leaf, rng, flags, proof_out, cap,
                                                 len);
}

int swm_pedersen_payment_prove_many_at(swm_ctx* ctx, const swm_pk* pk, const swm_pedersen_payment_circuit* c, const swm_merkle_tree* tree,
                                       const uint8_t* messages, const uint8_t* signatures, const uint8_t* sender_leaves,
                                       const uint8_t* recipient_leaves, size_t count, swm_rng* rng, unsigned flags, uint8_t* proofs_out,
                                       size_t proof_cap, size_t* lens, uint8_t* item_flags) {
    return payment_prove_many_at<PedersenPaymentUnit>(ctx, pk, c, tree, messages, signatures, sender_leaves, recipient_leaves, count, rng, flags,
                                                      proofs_out, proof_cap, lens, item_flags);
}

}  // extern "C"

// transfer_witness.hip — the witness of the transfer circuit for a block of transfers applied in order, the tree and the account
// table advanced on the GPU, and the proof entries on top of it.  The statement is State::apply_transaction of
// examples/simple-payments (ledger.rs:176-193) read sequentially over a Poseidon account tree: validate holds against old_root,
// debiting the sender gives R1, crediting the recipient in the tree of R1 gives new_root.  Order and values are those of
// simpleworks_amd/workloads.py, build_transfer: that function is the specification, host/transfer_shape.h the counts and offsets.
//
// Transfer i + 1 is witnessed against the tree as transfer i left it, so the path digests are produced in order; recording the
// permutations is independent once they are known (poseidon_tree_witness.hip).  A block of n transfers is
//   prep      transfer_prep_kernel     the senders' keys out of the account table for the Schnorr kernel (a transfer changes
//                                      balances only, so the table before the block serves)
//   schnorr   schnorr_witness_kernel   the Schnorr block, and whether the signature verifies
//   advance   transfer_advance_kernel  ONE workgroup: the table against the tree, then the transfers in order on one wave; per
//                                      transfer four paths as (digests | siblings), four leaves, the root pair, flag and status;
//                                      at the end the nodes and the table
//   record    poseidon_tree_record_kernel x 4 (ptw_record): the two membership blocks and the two update blocks
//   bits      transfer_bits_kernel     balance, diff, sum, the recipient's bits, R1
// eight launches, whatever n.  The flag byte is the advance kernel's: it decides whether the transfer is applied.
//
// The advance kernel's schedule for one transfer, sender index s, recipient index r, d = the top bit of s ^ r (the level at which
// the two paths' nodes are siblings).  Lane 0 walks the debited leaf, lane 1 the credited leaf, in lockstep, so the dependence
// chain is P_leaf + L permutations:
//   below d the walks are independent: both read siblings of the old tree;
//   at d the recipient's sibling IS the sender's new digest of level d: a shuffle, the one place where the intermediate tree's
//   path differs from the old tree's;
//   above d both walk over the same nodes, the sender lane carries the intermediate tree (R1 at the top), the recipient lane the
//   final one (new_root); the recipient's path IN THE TREE OF R1 needs no hashing: old nodes up to d, the sender lane's above.
// An applied transfer writes its digests into the nodes (in LDS) as it walks: the recipient lane at every level, the sender lane up
// to d.  A refused one walks the same way, for its witness, and writes nothing.  s == r has no d: the recipient lane's path in
// the tree of R1 is the sender lane's throughout (the sequential no-op); it is never applied.
//
// The host layer (chunks, the verdict-first results step, the block loop, the entries) is ledger_witness_host.h's over TransferUnit,
// which is transfer_units.h's PoseidonTransfers (circuit, tree, scratch names, tree check, transfer_run_strided) and a name.
#include <hip/hip_runtime.h>

#include <string.h>

#include <memory>
#include <vector>

#include "context.h"
#include "ff.cuh"
#include "host/transfer_shape.h"
#include "ledger_bytes.cuh"
#include "merkle_nodes.cuh"
#include "poseidon.h"
#include "poseidon_tree.h"
#include "schnorr.h"
#include "swmarlin.h"
#include "ledger_witness_host.h"
#include "transfer_units.h"
#include "witness_runs.h"

namespace swm {

static constexpr unsigned TR_LANES = 256;                                      // phase 0: a lane per leaf, ids are one byte
static constexpr unsigned TR_MAX_LEAVES = 1u << (PY_MAX_HEIGHT - 1);           // 256
static constexpr unsigned TR_FLAG_SIG = 1, TR_FLAG_BALANCE = 2, TR_FLAG_SUM = 4, TR_FLAG_ACCOUNTS = 8, TR_FLAG_APPLIED = 16;
static constexpr unsigned TR_ST_KEY = 1, TR_ST_ID = 4, TR_ST_SELF = 8;

// word i of the key array: 16 words per item out of the first 64 bytes of the sender's leaf in the table
__global__ void __launch_bounds__(TR_LANES) transfer_prep_kernel(const uint8_t* __restrict__ msgs, const uint8_t* __restrict__ accounts,
                                                                 size_t count, unsigned levels, uint32_t* __restrict__ keys) {
    const size_t i = blockIdx.x * (size_t)TR_LANES + threadIdx.x;
    if (i >= 16 * count) return;
    const size_t item = i >> 4;
    const unsigned word = (unsigned)(i & 15);
    const unsigned sender = msgs[PY_MSG_LEN * item] & ((1u << levels) - 1);
    const uint8_t* b = accounts + PY_LEAF_LEN * sender + 4 * word;
    keys[i] = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}

__device__ __forceinline__ bool tr_blank(const uint8_t* leaf) {
    unsigned any = 0;
    for (unsigned k = 0; k < PY_LEAF_LEN; k++) any |= leaf[k];
    return any == 0;
}

__device__ __forceinline__ Fr tr_select(bool c, const Fr& a, const Fr& b) {
    Fr x;
#pragma unroll
    for (int w = 0; w < 8; w++) x.v[w] = c ? a.v[w] : b.v[w];
    return x;
}

struct TrOut {              // what the advance kernel leaves for the record launches and the bits kernel, n = count
    uint32_t* dig;          // 4 x n x (L + 1) x 8 words: sender old | sender new | recipient in the tree of R1 | recipient new
    uint32_t* sib;          // 2 x n x L x 8 words: the sender's siblings | the recipient's in the tree of R1
    uint8_t* leaves;        // 4 x n x 72 bytes, in the order of dig
    uint64_t* idx;          // 2 x n: sender, recipient, masked to the tree
    uint32_t* roots;        // 2 x n x 8 words: old roots | new roots
    uint8_t* flags;         // n
    uint32_t* status;       // n, bit 0 is the Schnorr kernel's
    uint32_t* verdict;      // 1: nonzero when the table is not the tree's
};

// One workgroup.  nodes, accounts: read, and written back at the end unless the call is refused.
__global__ void __launch_bounds__(TR_LANES) transfer_advance_kernel(const uint4* __restrict__ table, PtParams P, unsigned levels, size_t count,
                                                                    uint32_t* __restrict__ nodes, uint8_t* __restrict__ accounts,
                                                                    const uint8_t* __restrict__ msgs, const uint8_t* __restrict__ sig_ok,
                                                                    TrOut O) {
    extern __shared__ __align__(16) uint32_t ps_tab[];
    __shared__ uint32_t s_nodes[(2 * TR_MAX_LEAVES - 1) * 8];
    __shared__ uint8_t s_acc[TR_MAX_LEAVES * PY_LEAF_LEN];
    __shared__ uint8_t s_new[PS_LANES * PY_LEAF_LEN];  // a lane's own new leaf, for the sponge
    __shared__ unsigned s_bad;
    const unsigned tid = threadIdx.x, n_leaves = 1u << levels, n_nodes = 2 * n_leaves - 1;
    if (tid == 0) s_bad = 0;
    for (unsigned i = tid; i < n_nodes * 8; i += TR_LANES) s_nodes[i] = nodes[i];
    for (unsigned i = tid; i < n_leaves * (unsigned)PY_LEAF_LEN; i += TR_LANES) s_acc[i] = accounts[i];
    pt_load_table(ps_tab, table, P.rows);  // its barrier covers the three loops above
    // phase 0: the table is the tree's leaf level
    if (tid < n_leaves) {
        Fr want = fp_zero<Fr>();
        if (!tr_blank(s_acc + PY_LEAF_LEN * tid)) want = pt_hash_leaf(ps_tab, P, s_acc, tid, PY_LEAF_LEN);
        unsigned diff = 0;
#pragma unroll
        for (int w = 0; w < 8; w++) diff |= want.v[w] ^ s_nodes[8 * tid + w];
        if (diff) s_bad = 1;  // every writer stores the same value
    }
    __syncthreads();
    if (s_bad) {
        if (tid == 0) *O.verdict = 1;
        return;
    }
    if (tid >= PS_LANES) return;  // phase 1 is one wave: no barrier from here on
    if (tid == 0) *O.verdict = 0;
    const unsigned me = tid & 1;  // 0: the sender's walk, 1: the recipient's; the lanes above 1 repeat these two and store nothing
    const bool store = tid < 2;
    const unsigned mask = n_leaves - 1;
    const size_t dig_stride = count * (levels + 1) * 8, sib_stride = count * levels * 8;
    uint8_t* my_new = s_new + PY_LEAF_LEN * tid;
#pragma unroll 1
    for (size_t t = 0; t < count; t++) {
        const uint8_t* msg = msgs + PY_MSG_LEN * t;
        const unsigned sid = msg[0], rid = msg[1], s = sid & mask, r = rid & mask;
        const uint64_t amount = le_load_u64(msg + 2);
        const uint8_t* s_leaf = s_acc + PY_LEAF_LEN * s;
        const uint64_t balance = le_load_u64(s_leaf + 64), diff = balance - amount;
        // the recipient's leaf in the tree of R1: the table's, or the debited leaf when it pays itself
        const uint8_t* r_leaf = s_acc + PY_LEAF_LEN * r;
        const uint64_t rbalance = s == r ? diff : le_load_u64(r_leaf + 64), sum = rbalance + amount;
        unsigned flag = (sig_ok[t] ? TR_FLAG_SIG : 0u) | (amount <= balance ? TR_FLAG_BALANCE : 0u) | (sum >= rbalance ? TR_FLAG_SUM : 0u) |
                        (!tr_blank(s_leaf) && !tr_blank(r_leaf) ? TR_FLAG_ACCOUNTS : 0u);
        const unsigned st = (O.status[t] & TR_ST_KEY) | ((sid | rid) >> levels ? TR_ST_ID : 0u) | (sid == rid ? TR_ST_SELF : 0u);
        const bool applied = flag == 15u && st == 0;
        if (applied) flag |= TR_FLAG_APPLIED;
        const int d = s == r ? -1 : 31 - __clz((int)(s ^ r));
        const unsigned mine = me ? r : s;
        // my two leaves: as they are in the tree this lane starts from, and as this lane leaves them
        const uint8_t* old_leaf = me ? r_leaf : s_leaf;
        const uint64_t old_value = me ? rbalance : balance, new_value = me ? sum : diff;
        uint8_t* out_old = O.leaves + PY_LEAF_LEN * ((size_t)(2 * me) * count + t);
        uint8_t* out_new = O.leaves + PY_LEAF_LEN * ((size_t)(2 * me + 1) * count + t);
        for (unsigned k = 0; k < PY_LEAF_LEN; k++) {
            const uint8_t key = old_leaf[k];
            const uint8_t o = k < 64 ? key : (uint8_t)(old_value >> (8 * (k - 64))), n = k < 64 ? key : (uint8_t)(new_value >> (8 * (k - 64)));
            my_new[k] = n;
            if (store) {
                out_old[k] = o;
                out_new[k] = n;
            }
        }
        uint32_t* dig_old = O.dig + (size_t)(2 * me) * dig_stride + t * (levels + 1) * 8;
        uint32_t* dig_new = O.dig + (size_t)(2 * me + 1) * dig_stride + t * (levels + 1) * 8;
        uint32_t* sib_out = O.sib + (size_t)me * sib_stride + t * levels * 8;
        if (store) {
            O.idx[(size_t)me * count + t] = mine;
            if (me == 0) pt_store(O.roots + 8 * t, pt_load(s_nodes + 8 * (n_nodes - 1)));
        }
        Fr cur = pt_hash_leaf(ps_tab, P, s_new, tid, PY_LEAF_LEN);
#pragma unroll 1
        for (unsigned l = 0; l <= levels; l++) {
            const size_t at = mt_level_offset(levels, l);
            Fr other;  // the neighbour lane's running digest
#pragma unroll
            for (int w = 0; w < 8; w++) other.v[w] = (uint32_t)__shfl_xor((int)cur.v[w], 1);
            const bool above = (int)l > d;  // the two walks are over the same node
            // the digest of my node in the tree this lane starts from
            const Fr before = me && above ? other : pt_load(s_nodes + 8 * (at + (mine >> l)));
            Fr sibling = fp_zero<Fr>();
            if (l < levels) sibling = me && (int)l == d ? other : pt_load(s_nodes + 8 * (at + ((mine >> l) ^ 1)));
            if (store) {
                pt_store(dig_old + 8 * l, before);
                pt_store(dig_new + 8 * l, cur);
                if (l < levels) pt_store(sib_out + 8 * l, sibling);
            }
            if (applied && store && (me || !above)) pt_store(s_nodes + 8 * (at + (mine >> l)), cur);
            if (l < levels) {
                const bool right = (mine >> l) & 1u;
                cur = pt_hash2(ps_tab, P, tr_select(right, sibling, cur), tr_select(right, cur, sibling));
            }
        }
        if (store) {
            if (applied) {
                uint8_t* leaf = s_acc + PY_LEAF_LEN * mine + 64;
                for (unsigned k = 0; k < 8; k++) leaf[k] = (uint8_t)(new_value >> (8 * k));
            }
            if (me == 0) {
                O.flags[t] = (uint8_t)flag;
                O.status[t] = st;
            }
        }
        // the next transfer's loads see these stores: one wave, LDS in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (store && me == 0) pt_store(O.roots + 8 * (count + t), pt_load(s_nodes + 8 * (n_nodes - 1)));
    }
    for (unsigned i = tid; i < n_nodes * 8; i += PS_LANES) nodes[i] = s_nodes[i];
    for (unsigned i = tid; i < n_leaves * (unsigned)PY_LEAF_LEN; i += PS_LANES) accounts[i] = s_acc[i];
}

struct TrBitsArgs {
    size_t count, stride, balance_at, sum_at, r1_at, recipient_bits_at;
    unsigned levels;
};

// Element e (0 .. 768) of item p: 64 balance bits, 64 diff bits (adjacent in the witness), 64 sum bits, 576 recipient leaf bits,
// R1.  Adjacent lanes write adjacent elements, two 16-byte stores each.
__global__ void __launch_bounds__(TR_LANES) transfer_bits_kernel(TrBitsArgs A, const uint8_t* __restrict__ leaves,
                                                                 const uint32_t* __restrict__ sender_new_dig, Fr* __restrict__ witness) {
    const size_t i = blockIdx.x * (size_t)TR_LANES + threadIdx.x;
    if (i >= TR_BIT_WITNESSES * A.count) return;
    const size_t item = i / TR_BIT_WITNESSES;
    const unsigned e = (unsigned)(i % TR_BIT_WITNESSES);
    const size_t n = A.count;
    Fr v;
    size_t at;
    if (e < 3 * PY_AMOUNT_BITS) {
        // balance: the sender's old leaf; diff: its new one; sum: the recipient's new one
        const unsigned which = e / (unsigned)PY_AMOUNT_BITS, k = e % (unsigned)PY_AMOUNT_BITS;
        const size_t leaf = which == 0 ? 0 : which == 1 ? 1 : 3;
        const unsigned bit = (leaves[PY_LEAF_LEN * (leaf * n + item) + 64 + (k >> 3)] >> (k & 7)) & 1u;
        v = bit ? fp_one<Fr>() : fp_zero<Fr>();
        at = which == 2 ? A.sum_at + k : A.balance_at + e;
    } else if (e < TR_BIT_WITNESSES - 1) {
        const unsigned k = e - 3 * (unsigned)PY_AMOUNT_BITS;
        const unsigned bit = (leaves[PY_LEAF_LEN * (2 * n + item) + (k >> 3)] >> (k & 7)) & 1u;
        v = bit ? fp_one<Fr>() : fp_zero<Fr>();
        at = A.recipient_bits_at + k;
    } else {
        v = fp_from_std(pt_load(sender_new_dig + 8 * (item * (A.levels + 1) + A.levels)));  // a digest is canonical
        at = A.r1_at;
    }
    uint4* q = reinterpret_cast<uint4*>(witness + item * A.stride + at);
    q[0] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
    q[1] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
}

int transfer_prep_run(swm_ctx* ctx, const uint8_t* d_msgs, const uint8_t* d_accounts, size_t n, unsigned levels, uint32_t* d_keys) {
    SWM_LAUNCH(ctx, "transfer_prep", transfer_prep_kernel, dim3((unsigned)((16 * n + TR_LANES - 1) / TR_LANES)), dim3(TR_LANES), 0, d_msgs,
               d_accounts, n, levels, d_keys);
    return SWM_OK;
}

int transfer_bits_run(swm_ctx* ctx, size_t n, size_t stride, size_t balance_at, size_t sum_at, size_t r1_at, size_t recipient_bits_at,
                      unsigned levels, const uint8_t* d_leaves, const uint32_t* d_sender_new_dig, Fr* d_w) {
    TrBitsArgs A;
    A.count = n;
    A.stride = stride;
    A.balance_at = balance_at;
    A.sum_at = sum_at;
    A.r1_at = r1_at;
    A.recipient_bits_at = recipient_bits_at;
    A.levels = levels;
    SWM_LAUNCH(ctx, "transfer_bits", transfer_bits_kernel, dim3((unsigned)((TR_BIT_WITNESSES * n + TR_LANES - 1) / TR_LANES)), dim3(TR_LANES), 0, A,
               d_leaves, d_sender_new_dig, d_w);
    return SWM_OK;
}

// "transfer.aux" for n transfers: every piece a multiple of 8 bytes but the last two
static size_t tr_aux_bytes(size_t n, size_t levels) {
    return 64 * n + 4 * (4 * n * (levels + 1) * 8 + 2 * n * levels * 8) + 16 * n + 64 * n + 4 * n + 8 + 4 * PY_LEAF_LEN * n + 2 * n + 64;
}

// n transfers on device buffers, in order: d_accounts and the tree's nodes are advanced.  d_w 16-byte aligned; item i's witnesses
// from d_w + i * stride (stride >= the shape's num_witness: a block's own driver passes that, the rollup's one more).
int transfer_run_strided(swm_ctx* ctx, const swm_transfer_circuit* c, swm_poseidon_tree* tree, uint8_t* d_accounts, const uint8_t* d_msgs,
                         const uint8_t* d_sigs, size_t n, Fr* d_w, size_t stride, BlockRunOut* out) {
    const TransferShape& s = c->shape;
    const swm_poseidon* p = c->tree.params;
    const unsigned levels = (unsigned)s.levels;
    uint8_t* aux = nullptr;
    SWM_TRY(scratch(ctx, "transfer.aux", tr_aux_bytes(n, levels), (void**)&aux));
    TrOut O;
    uint32_t* d_keys = reinterpret_cast<uint32_t*>(aux);
    O.dig = d_keys + 16 * n;
    O.sib = O.dig + 4 * n * (levels + 1) * 8;
    O.idx = reinterpret_cast<uint64_t*>(O.sib + 2 * n * levels * 8);
    O.roots = reinterpret_cast<uint32_t*>(O.idx + 2 * n);
    O.status = O.roots + 16 * n;
    O.verdict = O.status + n;
    O.leaves = reinterpret_cast<uint8_t*>(O.verdict + 2);
    O.flags = O.leaves + 4 * PY_LEAF_LEN * n;
    uint8_t* d_sig_ok = O.flags + n;
    SWM_TRY(transfer_prep_run(ctx, d_msgs, d_accounts, n, levels, d_keys));
    SWM_TRY(schnorr_witness_run(ctx, &c->schnorr, aux, d_msgs, d_sigs, n, d_w, stride, d_sig_ok, O.status));
    SWM_LAUNCH(ctx, "transfer_advance", transfer_advance_kernel, dim3(1), dim3(TR_LANES), pt_lds(p), pt_table(p), pt_params(p), levels, n,
               reinterpret_cast<uint32_t*>(tree->d_nodes), d_accounts, d_msgs, (const uint8_t*)d_sig_ok, O);
    const size_t dig = n * (levels + 1) * 8, sib = n * levels * 8, leaves = PY_LEAF_LEN * n;
    const size_t at[4] = {s.sender_at, s.sender_update_at, s.recipient_at, s.recipient_update_at};
    for (int k = 0; k < 4; k++)
        SWM_TRY(ptw_record(ctx, &c->tree, O.leaves + k * leaves, O.idx + (k / 2) * n, O.dig + k * dig, O.sib + (k / 2) * sib, n, d_w + at[k],
                           stride, k % 2 == 0));
    SWM_TRY(transfer_bits_run(ctx, n, stride, s.balance_at, s.sum_at, s.r1_at, s.recipient_bits_at, levels, O.leaves, O.dig + dig, d_w));
    *out = BlockRunOut{O.roots, O.flags, O.status, O.verdict};
    return SWM_OK;
}

// the prover over one item of a chunk's device witnesses; public input one, old_root, new_root, sender, recipient, amount
int transfer_prove_item(swm_ctx* ctx, const swm_pk* pk, size_t num_witness, size_t num_constraints, const uint8_t* old_root, const uint8_t* new_root,
                        const uint8_t* msg, const Fr* d_w, swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len) {
    uint64_t amount = 0;
    for (int k = 0; k < 8; k++) amount |= (uint64_t)msg[2 + k] << (8 * k);
    Fr r0, r1;
    (void)ps_load_std(old_root, &r0);  // nodes of the tree: canonical
    (void)ps_load_std(new_root, &r1);
    const Fr inst[6] = {fp_one<Fr>(), fp_from_std(r0), fp_from_std(r1), fp_from_u64<Fr>(msg[0]), fp_from_u64<Fr>(msg[1]), fp_from_u64<Fr>(amount)};
    return prove_device_witness(ctx, pk, TR_INSTANCE, num_witness, num_constraints, inst, d_w, rng, flags, proof_out, cap, len);
}

static_assert(TR_FLAG_APPLIED == TRANSFER_FLAG_APPLIED, "the block driver proves what the advance kernel applied");

struct TransferUnit : PoseidonTransfers {  // what ledger_witness_host.h drives
    static constexpr const char* name = "transfer";
};

}  // namespace swm

using namespace swm;

extern "C" {

int swm_transfer_circuit_create(swm_ctx* ctx, const swm_schnorr* schnorr, const swm_poseidon* poseidon, size_t height, swm_transfer_circuit** out) {
    if (!ctx || !schnorr || !poseidon || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "transfer_circuit_create: bad arguments");
    TransferShape shape;
    if (!transfer_shape(poseidon->full_rounds, poseidon->partial_rounds, poseidon->alpha, height, schnorr->has_salt, &shape))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "transfer_circuit_create: height %zu (%zu <= height <= %zu)", height, (size_t)PY_MIN_HEIGHT,
                       (size_t)PY_MAX_HEIGHT);
    std::unique_ptr<swm_transfer_circuit> c(new swm_transfer_circuit);
    c->schnorr.params = schnorr;
    c->schnorr.shape = shape.payment.schnorr;
    c->tree.params = poseidon;
    c->tree.shape = shape.payment.tree;
    c->shape = shape;
    *out = c.release();
    return SWM_OK;
}

void swm_transfer_circuit_destroy(swm_ctx* ctx, swm_transfer_circuit* c) { destroy_circuit(ctx, c); }

int swm_transfer_witness_at(swm_ctx* ctx, const swm_transfer_circuit* c, swm_poseidon_tree* tree, uint8_t* accounts_inout, const uint8_t* messages,
                            const uint8_t* signatures, size_t count, uint64_t* witnesses_out, uint8_t* old_roots, uint8_t* new_roots,
                            uint8_t* flags, uint32_t* status) {
    return transfer_witness_at<TransferUnit>(ctx, c, tree, accounts_inout, messages, signatures, count, witnesses_out, old_roots, new_roots, flags,
                                             status);
}

int swm_transfer_prove_many_at(swm_ctx* ctx, const swm_pk* pk, const swm_transfer_circuit* c, swm_poseidon_tree* tree, uint8_t* accounts_inout,
                               const uint8_t* messages, const uint8_t* signatures, size_t count, swm_rng* rng, unsigned prove_flags,
                               uint8_t* proofs_out, size_t proof_cap, size_t* lens, uint8_t* old_roots, uint8_t* new_roots, uint8_t* flags,
                               uint32_t* status) {
    return transfer_prove_many_at<TransferUnit>(ctx, pk, c, tree, accounts_inout, messages, signatures, count, rng, prove_flags, proofs_out,
                                                proof_cap, lens, old_roots, new_roots, flags, status);
}

int swm_transfer_prove_at(swm_ctx* ctx, const swm_pk* pk, const swm_transfer_circuit* c, swm_poseidon_tree* tree, uint8_t* accounts_inout,
                          const uint8_t message[10], const uint8_t signature[64], swm_rng* rng, unsigned prove_flags, uint8_t* proof_out,
                          size_t cap, size_t* len, uint8_t old_root[32], uint8_t new_root[32], uint8_t* flag, uint32_t* status) {
    if (!message || !signature || !proof_out || !len || !old_root || !new_root || !flag || !status)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "transfer_prove_at: bad arguments");
    return swm_transfer_prove_many_at(ctx, pk, c, tree, accounts_inout, message, signature, 1, rng, prove_flags, proof_out, cap, len, old_root,
                                      new_root, flag, status);
}

}  // extern "C"

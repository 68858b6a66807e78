// pedersen_account_update_witness.hip — the witness of the account-update circuit over a PEDERSEN account tree for a block of
// registrations and balance updates applied in order, the resident tree (swm_merkle_tree, 72-byte leaves) and the account table
// advanced on the GPU, and the proof entries on top of it.  The statement is account_update_witness.hip's (State::register and
// State::update_balance: the leaf at `id` becomes key || new_balance, every other leaf stays) over the sections of
// pedersen_payment_witness.hip.  Order and values are those of simpleworks_amd/workloads.py, build_pedersen_account_update: that
// function is the specification, host/pedersen_account_update_shape.h the counts and offsets.  Over this tree the blank leaf is a
// member (the hash of 72 zero bytes is the identity's x = 0), so a registration's old leaf is 72 zero bytes and its section is a
// membership section like any other: no cur_0, no masked digest.
//
// A block of n operations is
//   check     pedersen_transfer_check_kernel  (pedersen_transfer_witness.hip, witness_runs.h) the table against the tree's leaf level
//   advance   pedersen_account_update_advance_kernel  ONE workgroup of ONE wave: the operations in order; per operation two paths
//                                             as (digests | siblings, one sibling array for both), two leaves, the masked id, the root
//                                             pair, flag and status; at the end the nodes and the table.  It reads the verdict word
//                                             first and leaves when it is set.
//   leaves    pp_record_leaf_kernel           2 n leaf stages    } pedersen_payment_witness.hip (witness_runs.h: pp_record_run): the
//   levels    pp_record_level_kernel          2 n L level stages } membership section and the update section
//   bits      pedersen_account_update_bits_kernel  the 648 booleans and the 512 masked bits; a refused operation's vector cleared
// five launches and one 4-byte memset (the verdict word), whatever n.  No atomics; stream order is the only cross-launch ordering.
//
// The advance kernel's schedule for one operation on leaf m: the old path is a gather — cur_0 .. cur_L and the L siblings are read
// from the nodes before anything is written, the old side hashes nothing.  An applied operation hashes the new leaf (144 windows
// over the wave's 64 lanes) and walks it to the root (128 windows per level): 1 + L dependent hashes, each level's node written
// after a barrier that follows that level's reads.  A refused one hashes nothing, writes neither nodes nor table, and leaves the
// gathered old path in both digest arrays, so that the record launches read initialised memory.
//
// The host layer (chunks, the verdict-first results step, the block loop, the entries, the prover call) is ledger_witness_host.h's
// over PedersenAccountUpdateUnit, with the vocabulary (AuIn, AuOut, flag, status and kind constants) account_update_witness.hip uses.
#include <hip/hip_runtime.h>

#include <string.h>

#include <memory>
#include <vector>

#include "context.h"
#include "ff.cuh"
#include "host/pedersen_account_update_shape.h"
#include "ledger_bytes.cuh"
#include "ledger_witness_host.h"
#include "merkle_nodes.cuh"
#include "merkle_tree.h"
#include "pedersen.cuh"
#include "pedersen.h"
#include "swmarlin.h"
#include "witness_runs.h"

struct swm_pedersen_account_update_circuit {
    const swm_pedersen* leaf = nullptr;
    const swm_pedersen* inner = nullptr;
    swm::PedersenAccountUpdateShape shape;
};

namespace swm {

static constexpr unsigned PAU_LANES = 64;                                  // one wave: a Pedersen hash takes it whole
static constexpr unsigned PAU_BITS_LANES = 256;
static constexpr unsigned PAU_MAX_LEAVES = 1u << (PP_MAX_HEIGHT - 1);      // 256
static_assert(PP_LEAF_LEN == PY_LEAF_LEN && PAU_INSTANCE == 9, "the block driver's leaf, the prover's public input");

// One workgroup, one wave.  nodes, accounts: read, and written back at the end unless the call is refused.  O.leaves: the old leaf
// (72 zero bytes for a registration) | key || new_balance; O.verdict is the check kernel's.
__global__ void __launch_bounds__(PAU_LANES) pedersen_account_update_advance_kernel(const EdRow* __restrict__ leaf_table, unsigned leaf_windows,
                                                                                    const EdRow* __restrict__ inner_table, unsigned inner_windows,
                                                                                    unsigned levels, size_t count, uint32_t* __restrict__ nodes,
                                                                                    uint8_t* __restrict__ accounts, AuIn I, Fr k2d, AuOut O) {
    __shared__ uint32_t s_nodes[(2 * PAU_MAX_LEAVES - 1) * 8];
    __shared__ uint8_t s_acc[PAU_MAX_LEAVES * PP_LEAF_LEN];
    __shared__ uint32_t s_msg[16];           // left || right of the level's hash
    __shared__ uint8_t s_leaf[PP_LEAF_LEN];  // the new leaf
    __shared__ uint32_t s_cur[8];            // the running digest
    if (*O.verdict) return;                  // the table is not the tree's: nothing is written
    const unsigned lane = threadIdx.x;
    const unsigned n_leaves = 1u << levels, n_nodes = 2 * n_leaves - 1, mask = n_leaves - 1;
    for (unsigned i = lane; i < n_nodes * 8; i += PAU_LANES) s_nodes[i] = nodes[i];
    for (unsigned i = lane; i < n_leaves * (unsigned)PP_LEAF_LEN; i += PAU_LANES) s_acc[i] = accounts[i];
    __syncthreads();
    const size_t dig_stride = count * (levels + 1) * 8;
#pragma unroll 1
    for (size_t t = 0; t < count; t++) {
        const unsigned id = I.ids[t], kind = I.kinds[t], m = id & mask;
        const bool reg = kind == AU_KIND_REGISTER;
        const uint8_t* leaf = s_acc + PP_LEAF_LEN * m;
        const uint8_t* key = reg ? I.keys + 64 * t : leaf;
        const uint64_t new_value = le_load_u64(I.balances + 8 * t);
        // the decision: every lane reads the same bytes and takes the same one
        unsigned held = 0, any = 0;
        for (unsigned k = 0; k < PP_LEAF_LEN; k++) held |= leaf[k];
        for (unsigned k = 0; k < 64; k++) any |= key[k];
        any |= new_value != 0;
        unsigned st = 0;
        if (id >> levels) st = AU_ST_ID;  // there is no leaf to say more about
        else if (reg)
            st = (le_below_r(key) && le_below_r(key + 32) ? 0u : AU_ST_KEY) | (held ? AU_ST_OCCUPIED : 0u) | (any ? 0u : AU_ST_ZERO);
        else
            st = held ? 0u : AU_ST_BLANK;
        const bool applied = st == 0;
        for (unsigned k = lane; k < PP_LEAF_LEN; k += PAU_LANES) {
            const uint8_t o = reg ? (uint8_t)0 : leaf[k], n = k < 64 ? key[k] : (uint8_t)(new_value >> (8 * (k - 64)));
            s_leaf[k] = n;
            O.leaves[PP_LEAF_LEN * t + k] = o;
            O.leaves[PP_LEAF_LEN * (count + t) + k] = n;
        }
        uint32_t* dig_old = O.dig + t * (levels + 1) * 8;
        uint32_t* dig_new = O.dig + dig_stride + t * (levels + 1) * 8;
        uint32_t* sib_out = O.sib + t * levels * 8;
        // the old path, gathered: nothing of this operation is written yet
        for (unsigned i = lane; i < (levels + 1) * 8; i += PAU_LANES) {
            const unsigned l = i >> 3;
            const uint32_t v = s_nodes[8 * (mt_level_offset(levels, l) + (m >> l)) + (i & 7)];
            dig_old[i] = v;
            if (!applied) dig_new[i] = v;
        }
        for (unsigned i = lane; i < levels * 8; i += PAU_LANES) {
            const unsigned l = i >> 3;
            sib_out[i] = s_nodes[8 * (mt_level_offset(levels, l) + ((m >> l) ^ 1)) + (i & 7)];
        }
        if (lane == 0) O.idx[t] = m;
        if (lane < 8) O.roots[8 * t + lane] = s_nodes[8 * (n_nodes - 1) + lane];
        __syncthreads();  // s_leaf is whole, the gather is done
        if (applied) {    // the same in every lane
            {
                const uint8_t* b = s_leaf;
                EdExt acc = ped_partial(leaf_table, leaf_windows, 4, [b](size_t i) { return (unsigned)b[i]; }, PP_LEAF_LEN, PAU_LANES, lane);
                acc = ped_join(acc, PAU_LANES, k2d);
                if (lane == 0) {
                    const Fr x = ped_digest(acc);
#pragma unroll
                    for (int i = 0; i < 8; i++) s_cur[i] = x.v[i];
                }
            }
            __syncthreads();
#pragma unroll 1
            for (unsigned l = 0; l <= levels; l++) {
                const size_t at = mt_level_offset(levels, l);
                const unsigned word = lane & 7;
                const uint32_t cur = s_cur[word];
                uint32_t sibling = 0;
                if (l < levels) sibling = s_nodes[8 * (at + ((m >> l) ^ 1)) + word];
                if (lane < 8) dig_new[8 * l + lane] = cur;
                if (l < levels && lane < 16) {
                    const bool right = (m >> l) & 1u;  // the running digest is the right child
                    s_msg[lane] = (lane < 8) == right ? sibling : cur;
                }
                __syncthreads();  // every read of this level is done
                if (lane < 8) s_nodes[8 * (at + (m >> l)) + lane] = cur;
                if (l < levels) {
                    const uint32_t* w = s_msg;
                    EdExt acc = ped_partial(inner_table, inner_windows, 4, [w](size_t i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xFFu; }, 64,
                                            PAU_LANES, lane);
                    acc = ped_join(acc, PAU_LANES, k2d);
                    if (lane == 0) {
                        const Fr x = ped_digest(acc);
#pragma unroll
                        for (int i = 0; i < 8; i++) s_cur[i] = x.v[i];
                    }
                }
                __syncthreads();  // the next level reads these writes
            }
            for (unsigned k = lane; k < PP_LEAF_LEN; k += PAU_LANES) s_acc[PP_LEAF_LEN * m + k] = s_leaf[k];
        }
        if (lane == 0) {
            O.flags[t] = applied ? (uint8_t)AU_FLAG_APPLIED : (uint8_t)0;
            O.status[t] = st;
        }
        __syncthreads();  // the root and the table as this operation leaves them
        if (lane < 8) O.roots[8 * (count + t) + lane] = s_nodes[8 * (n_nodes - 1) + lane];
        __syncthreads();  // the next operation writes s_leaf
    }
    for (unsigned i = lane; i < n_nodes * 8; i += PAU_LANES) nodes[i] = s_nodes[i];
    for (unsigned i = lane; i < n_leaves * (unsigned)PP_LEAF_LEN; i += PAU_LANES) accounts[i] = s_acc[i];
}

struct PauBitsArgs {
    size_t count, stride, num_witness;
};

// Lane i writes 16 bytes: half (i & 1) of element e = (i / 2) % num_witness of item (i / 2) / num_witness.  An applied item: e < 1160
// is a boolean or a masked key bit, in storage order (512 key bits, 64 bits of the old balance, 64 of the new one, 8 id bits, 512
// masked key bits: the old leaf's key bytes, zero for a registration), the others are the record launches'.  A refused item: every
// element is cleared.
__global__ void __launch_bounds__(PAU_BITS_LANES) pedersen_account_update_bits_kernel(PauBitsArgs A, const uint8_t* __restrict__ ids,
                                                                                      const uint8_t* __restrict__ leaves,
                                                                                      const uint8_t* __restrict__ flags, Fr* __restrict__ witness) {
    const size_t i = blockIdx.x * (size_t)PAU_BITS_LANES + threadIdx.x;
    if (i >= 2 * A.num_witness * A.count) return;
    const size_t item = (i >> 1) / A.num_witness;
    const unsigned e = (unsigned)((i >> 1) % A.num_witness), half = (unsigned)(i & 1);
    bool set = false;
    if (flags[item] & AU_FLAG_APPLIED) {
        if (e >= PAU_LOOSE_WITNESSES) return;
        const uint8_t* old_leaf = leaves + PP_LEAF_LEN * item;
        const uint8_t* new_leaf = leaves + PP_LEAF_LEN * (A.count + item);
        unsigned byte;
        if (e < PAU_KEY_BITS) byte = new_leaf[e >> 3];
        else if (e < PAU_KEY_BITS + PP_AMOUNT_BITS) byte = old_leaf[64 + ((e - PAU_KEY_BITS) >> 3)];
        else if (e < PAU_KEY_BITS + 2 * PP_AMOUNT_BITS) byte = new_leaf[64 + ((e - PAU_KEY_BITS - PP_AMOUNT_BITS) >> 3)];
        else if (e < PAU_BOOLEANS) byte = ids[item];
        else byte = old_leaf[(e - PAU_BOOLEANS) >> 3];
        set = (byte >> (e & 7)) & 1u;  // every group starts at a multiple of 8
    }
    const Fr one = fp_one<Fr>();
    const uint4 v = half ? make_uint4(one.v[4], one.v[5], one.v[6], one.v[7]) : make_uint4(one.v[0], one.v[1], one.v[2], one.v[3]);
    reinterpret_cast<uint4*>(witness + item * A.stride + e)[half] = set ? v : make_uint4(0, 0, 0, 0);
}

static const EdRow* pau_rows(const swm_pedersen* p) { return reinterpret_cast<const EdRow*>(p->d_table); }

// n operations on device buffers, in order: d_accounts and the tree's nodes are advanced.  d_w 16-byte aligned; item i's witnesses
// from d_w + i * stride (stride >= the shape's num_witness).
static int pau_run(swm_ctx* ctx, const swm_pedersen_account_update_circuit* c, swm_merkle_tree* tree, uint8_t* d_accounts, const AuIn& in,
                   size_t n, Fr* d_w, size_t stride, AuOut* out) {
    const PedersenAccountUpdateShape& s = c->shape;
    const unsigned levels = (unsigned)s.levels, n_leaves = 1u << levels;
    AuOut O;
    SWM_TRY(account_update_aux(ctx, "paccount_update.aux", n, levels, &O));
    uint32_t* d_nodes = reinterpret_cast<uint32_t*>(tree->d_nodes);
    SWM_HIP(ctx, hipMemsetAsync(O.verdict, 0, 4, ctx->stream));
    SWM_TRY(pedersen_transfer_check_run(ctx, c->leaf, d_nodes, d_accounts, n_leaves, O.verdict));
    SWM_LAUNCH(ctx, "pedersen_account_update_advance", pedersen_account_update_advance_kernel, dim3(1), dim3(PAU_LANES), 0, pau_rows(c->leaf),
               c->leaf->num_windows, pau_rows(c->inner), c->inner->num_windows, levels, n, d_nodes, d_accounts, in, fp_from_u64<Fr>(2 * ED_D), O);
    // (After a refused table the advance kernel has written nothing: the launches below then read whatever the scratch holds — every
    // read and write within its buffer, an index is used for its direction bits alone — and the caller drops the chunk.)
    const size_t dig = n * (levels + 1) * 8, leaves = PP_LEAF_LEN * n;
    PpArgs A = {};
    A.stride = stride;
    A.dig_stride = (size_t)(levels + 1) * 8;
    A.levels = levels;
    A.sections = 2;
    A.s[0] = {O.leaves, O.dig, O.sib, O.idx, s.old_at, 0u};
    A.s[1] = {O.leaves + leaves, O.dig + dig, O.sib, O.idx, s.new_at, 1u};
    SWM_TRY(pp_record_run(ctx, c->leaf, c->inner, A, n, d_w));
    PauBitsArgs B;
    B.count = n;
    B.stride = stride;
    B.num_witness = s.num_witness;
    SWM_LAUNCH(ctx, "pedersen_account_update_bits", pedersen_account_update_bits_kernel,
               dim3((unsigned)((2 * s.num_witness * n + PAU_BITS_LANES - 1) / PAU_BITS_LANES)), dim3(PAU_BITS_LANES), 0, B, in.ids,
               (const uint8_t*)O.leaves, (const uint8_t*)O.flags, d_w);
    *out = O;
    return SWM_OK;
}

struct PedersenAccountUpdateUnit {  // what ledger_witness_host.h drives
    using Circuit = swm_pedersen_account_update_circuit;
    using Tree = swm_merkle_tree;
    static constexpr const char* name = "pedersen_account_update";
    static constexpr const char* accounts_scratch = "paccount_update.accounts";
    static constexpr const char* witness_scratch = "paccount_update.w";
    static constexpr auto run = pau_run;
    static int check_tree(swm_ctx* ctx, const char* what, const Circuit* c, const Tree* t) {
        return ledger_check_tree(ctx, what, c->leaf, c->inner, c->shape.height, t);
    }
};

}  // namespace swm

using namespace swm;

extern "C" {

int swm_pedersen_account_update_circuit_create(swm_ctx* ctx, const swm_pedersen* leaf, const swm_pedersen* inner, size_t height,
                                               swm_pedersen_account_update_circuit** out) {
    if (!ctx || !leaf || !inner || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "pedersen_account_update_circuit_create: bad arguments");
    PedersenAccountUpdateShape shape;
    if (!pedersen_account_update_shape(height, &shape))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "pedersen_account_update_circuit_create: height %zu (%zu <= height <= %zu)", height,
                       (size_t)PP_MIN_HEIGHT, (size_t)PP_MAX_HEIGHT);
    SWM_TRY(pedersen_tree_crh_check(ctx, "pedersen_account_update_circuit_create", leaf, inner));
    std::unique_ptr<swm_pedersen_account_update_circuit> c(new swm_pedersen_account_update_circuit);
    c->leaf = leaf;
    c->inner = inner;
    c->shape = shape;
    *out = c.release();
    return SWM_OK;
}

void swm_pedersen_account_update_circuit_destroy(swm_ctx* ctx, swm_pedersen_account_update_circuit* c) { destroy_circuit(ctx, c); }

int swm_pedersen_account_update_witness_at(swm_ctx* ctx, const swm_pedersen_account_update_circuit* c, swm_merkle_tree* tree,
                                           uint8_t* accounts_inout, const uint8_t* ids, const uint8_t* kinds, const uint8_t* keys_xy,
                                           const uint8_t* balances, size_t count, uint64_t* witnesses_out, uint8_t* old_roots,
                                           uint8_t* new_roots, uint8_t* flags, uint32_t* status) {
    return account_update_witness_at<PedersenAccountUpdateUnit>(ctx, c, tree, accounts_inout, ids, kinds, keys_xy, balances, count, witnesses_out,
                                                                old_roots, new_roots, flags, status);
}

int swm_pedersen_account_update_prove_many_at(swm_ctx* ctx, const swm_pk* pk, const swm_pedersen_account_update_circuit* c,
                                              swm_merkle_tree* tree, uint8_t* accounts_inout, const uint8_t* ids, const uint8_t* kinds,
                                              const uint8_t* keys_xy, const uint8_t* balances, size_t count, swm_rng* rng,
                                              unsigned prove_flags, uint8_t* proofs_out, size_t proof_cap, size_t* lens, uint8_t* old_roots,
                                              uint8_t* new_roots, uint8_t* flags, uint32_t* status) {
    return account_update_prove_many_at<PedersenAccountUpdateUnit>(ctx, pk, c, tree, accounts_inout, ids, kinds, keys_xy, balances, count, rng,
                                                                   prove_flags, proofs_out, proof_cap, lens, old_roots, new_roots, flags, status);
}

int swm_pedersen_account_update_prove_at(swm_ctx* ctx, const swm_pk* pk, const swm_pedersen_account_update_circuit* c, swm_merkle_tree* tree,
                                         uint8_t* accounts_inout, uint8_t id, uint8_t kind, const uint8_t key_xy[64], uint64_t balance,
                                         swm_rng* rng, unsigned prove_flags, uint8_t* proof_out, size_t cap, size_t* len,
                                         uint8_t old_root[32], uint8_t new_root[32], uint8_t* flag, uint32_t* status) {
    return account_update_prove_at<PedersenAccountUpdateUnit>(ctx, pk, c, tree, accounts_inout, id, kind, key_xy, balance, rng, prove_flags,
                                                              proof_out, cap, len, old_root, new_root, flag, status);
}

}  // extern "C"

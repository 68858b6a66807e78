// account_update_witness.hip — the witness of the account-update circuit for a block of registrations and balance updates applied in
// order, the tree and the account table advanced on the GPU, and the proof entries on top of it.  The statement is State::register
// (examples/simple-payments, ledger.rs:131-150) and State::update_balance (:166-173) over a Poseidon account tree: the leaf at `id`
// becomes key || new_balance, every other leaf stays; the old leaf is key || old_balance, or the blank leaf (level-0 node: the zero
// digest) for a registration.  Order and values are those of simpleworks_amd/workloads.py, build_account_update: that function is the
// specification, host/account_update_shape.h the counts and offsets.  The key is packed unreduced, with no strict-canonical check
// in the circuit (the caveat of the Schnorr block's `dec` bits): a registration whose coordinate is >= r is refused here.
//
// Operation i + 1 is witnessed against the tree as operation i left it, so the path digests are produced in order; recording the
// permutations is independent once they are known (poseidon_tree_witness.hip).  A block of n operations is
//   advance   account_update_advance_kernel  ONE workgroup: the table against the tree, then the operations in order on one wave;
//                                            per operation two paths as (digests | siblings, one sibling array for both), two
//                                            leaves, the masked index, the root pair, flag and status; at the end the nodes and
//                                            the table
//   record    poseidon_tree_record_kernel x 2 (ptw_record, unchanged): the old leaf's membership block — its leaf unit records the
//                                            honest h = HL(key || old_balance), its level units walk the gathered digests, whose
//                                            first is cur_0 = the node (zero for a blank leaf) — and the update block (own_path 0)
//   bits      account_update_bits_kernel     the 648 booleans and cur_0; a refused operation's whole vector cleared
// four launches, whatever n.
//
// The advance kernel's schedule for one operation on leaf m: the old path is a gather — digests and siblings are read from the nodes
// before anything is written, the old side hashes nothing (the masked leaf hash is the record kernel's).  An applied operation
// hashes the new leaf and walks it to the root, P_leaf + L dependent permutations, writing each digest into the nodes (in LDS) after
// the level's loads.  A refused one hashes nothing, writes nothing and leaves zero digests for the update block.  Every lane of the
// wave computes the same; lane 0 stores.
//
// The host layer (chunks, the verdict-first results step, the block loop, the entries) is ledger_witness_host.h's over
// AccountUpdateUnit; this unit also defines account_update_prove_item, the prover call of both trees' units.
#include <hip/hip_runtime.h>

#include <string.h>

#include <memory>
#include <vector>

#include "context.h"
#include "ff.cuh"
#include "host/account_update_shape.h"
#include "ledger_bytes.cuh"
#include "ledger_witness_host.h"
#include "merkle_nodes.cuh"
#include "poseidon.h"
#include "poseidon_tree.h"
#include "swmarlin.h"
#include "witness_runs.h"

struct swm_account_update_circuit {
    swm_poseidon_tree_circuit tree;  // over PY_LEAF_LEN bytes
    swm::AccountUpdateShape shape;
};

namespace swm {

static constexpr unsigned AU_LANES = 256;                              // phase 0: a lane per leaf, ids are one byte
static constexpr unsigned AU_MAX_LEAVES = 1u << (PY_MAX_HEIGHT - 1);   // 256

__device__ __forceinline__ bool au_blank(const uint8_t* leaf) {
    unsigned any = 0;
    for (unsigned k = 0; k < PY_LEAF_LEN; k++) any |= leaf[k];
    return any == 0;
}

__device__ __forceinline__ Fr au_select(bool c, const Fr& a, const Fr& b) {
    Fr x;
#pragma unroll
    for (int w = 0; w < 8; w++) x.v[w] = c ? a.v[w] : b.v[w];
    return x;
}

// One workgroup.  nodes, accounts: read, and written back at the end unless the call is refused.  O.leaves: key || old_balance |
// key || new_balance.
__global__ void __launch_bounds__(AU_LANES) account_update_advance_kernel(const uint4* __restrict__ table, PtParams P, unsigned levels,
                                                                          size_t count, uint32_t* __restrict__ nodes,
                                                                          uint8_t* __restrict__ accounts, AuIn I, AuOut O) {
    extern __shared__ __align__(16) uint32_t ps_tab[];
    __shared__ uint32_t s_nodes[(2 * AU_MAX_LEAVES - 1) * 8];
    __shared__ uint8_t s_acc[AU_MAX_LEAVES * PY_LEAF_LEN];
    __shared__ uint8_t s_new[PS_LANES * PY_LEAF_LEN];  // a lane's own new leaf, for the sponge
    __shared__ unsigned s_bad;
    const unsigned tid = threadIdx.x, n_leaves = 1u << levels, n_nodes = 2 * n_leaves - 1;
    if (tid == 0) s_bad = 0;
    for (unsigned i = tid; i < n_nodes * 8; i += AU_LANES) s_nodes[i] = nodes[i];
    for (unsigned i = tid; i < n_leaves * (unsigned)PY_LEAF_LEN; i += AU_LANES) s_acc[i] = accounts[i];
    pt_load_table(ps_tab, table, P.rows);  // its barrier covers the three loops above
    // phase 0: the table is the tree's leaf level
    if (tid < n_leaves) {
        Fr want = fp_zero<Fr>();
        if (!au_blank(s_acc + PY_LEAF_LEN * tid)) want = pt_hash_leaf(ps_tab, P, s_acc, tid, PY_LEAF_LEN);
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
    const bool store = tid == 0;
    const unsigned mask = n_leaves - 1;
    const size_t dig_stride = count * (levels + 1) * 8;
    uint8_t* my_new = s_new + PY_LEAF_LEN * tid;
#pragma unroll 1
    for (size_t t = 0; t < count; t++) {
        const unsigned id = I.ids[t], kind = I.kinds[t], m = id & mask;
        const uint8_t* leaf = s_acc + PY_LEAF_LEN * m;
        const uint8_t* key = kind == AU_KIND_REGISTER ? I.keys + 64 * t : leaf;
        const bool blank = au_blank(leaf);
        const uint64_t old_value = kind == AU_KIND_REGISTER ? 0 : le_load_u64(leaf + 64), new_value = le_load_u64(I.balances + 8 * t);
        uint8_t* out_old = O.leaves + PY_LEAF_LEN * t;
        uint8_t* out_new = O.leaves + PY_LEAF_LEN * (count + t);
        unsigned any = 0;
        for (unsigned k = 0; k < PY_LEAF_LEN; k++) {
            const uint8_t kb = k < 64 ? key[k] : 0;
            const uint8_t o = k < 64 ? kb : (uint8_t)(old_value >> (8 * (k - 64))), n = k < 64 ? kb : (uint8_t)(new_value >> (8 * (k - 64)));
            any |= n;
            my_new[k] = n;
            if (store) {
                out_old[k] = o;
                out_new[k] = n;
            }
        }
        unsigned st = 0;
        if (id >> levels) st = AU_ST_ID;  // there is no leaf to say more about
        else if (kind == AU_KIND_REGISTER)
            st = (le_below_r(key) && le_below_r(key + 32) ? 0u : AU_ST_KEY) | (blank ? 0u : AU_ST_OCCUPIED) | (any ? 0u : AU_ST_ZERO);
        else
            st = blank ? AU_ST_BLANK : 0u;
        const bool applied = st == 0;  // the same in every lane
        uint32_t* dig_old = O.dig + t * (levels + 1) * 8;
        uint32_t* dig_new = O.dig + dig_stride + t * (levels + 1) * 8;
        uint32_t* sib_out = O.sib + t * levels * 8;
        if (store) {
            O.idx[t] = m;
            pt_store(O.roots + 8 * t, pt_load(s_nodes + 8 * (n_nodes - 1)));
        }
        Fr cur = fp_zero<Fr>();
        if (applied) cur = pt_hash_leaf(ps_tab, P, s_new, tid, PY_LEAF_LEN);
#pragma unroll 1
        for (unsigned l = 0; l <= levels; l++) {
            const size_t at = mt_level_offset(levels, l);
            // this level's loads, then its one store
            const Fr before = pt_load(s_nodes + 8 * (at + (m >> l)));
            Fr sibling = fp_zero<Fr>();
            if (l < levels) sibling = pt_load(s_nodes + 8 * (at + ((m >> l) ^ 1)));
            if (store) {
                pt_store(dig_old + 8 * l, before);
                pt_store(dig_new + 8 * l, cur);
                if (l < levels) pt_store(sib_out + 8 * l, sibling);
                if (applied) pt_store(s_nodes + 8 * (at + (m >> l)), cur);
            }
            if (applied && l < levels) {
                const bool right = (m >> l) & 1u;
                cur = pt_hash2(ps_tab, P, au_select(right, sibling, cur), au_select(right, cur, sibling));
            }
        }
        if (store) {
            if (applied) {
                uint8_t* dst = s_acc + PY_LEAF_LEN * m;
                for (unsigned k = 0; k < PY_LEAF_LEN; k++) dst[k] = my_new[k];
            }
            O.flags[t] = applied ? (uint8_t)AU_FLAG_APPLIED : (uint8_t)0;
            O.status[t] = st;
        }
        // the next operation's loads see these stores: one wave, LDS in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (store) pt_store(O.roots + 8 * (count + t), pt_load(s_nodes + 8 * (n_nodes - 1)));
    }
    for (unsigned i = tid; i < n_nodes * 8; i += PS_LANES) nodes[i] = s_nodes[i];
    for (unsigned i = tid; i < n_leaves * (unsigned)PY_LEAF_LEN; i += PS_LANES) accounts[i] = s_acc[i];
}

struct AuBitsArgs {
    size_t count, stride, num_witness;
    unsigned levels;
};

// Element e (0 .. num_witness) of item p.  An applied item: e < 649 is a boolean or cur_0, in storage order (512 key bits, 64 bits
// of the old balance, 64 of the new one, 8 id bits, cur_0), the others are the record launches'.  A refused item: every element is
// cleared.  Adjacent lanes write adjacent elements, two 16-byte stores each.
__global__ void __launch_bounds__(AU_LANES) account_update_bits_kernel(AuBitsArgs A, const uint8_t* __restrict__ ids,
                                                                       const uint8_t* __restrict__ leaves, const uint32_t* __restrict__ dig_old,
                                                                       const uint8_t* __restrict__ flags, Fr* __restrict__ witness) {
    const size_t i = blockIdx.x * (size_t)AU_LANES + threadIdx.x;
    if (i >= A.num_witness * A.count) return;
    const size_t item = i / A.num_witness;
    const unsigned e = (unsigned)(i % A.num_witness);
    Fr v = fp_zero<Fr>();
    if (flags[item] & AU_FLAG_APPLIED) {
        if (e >= AU_BIT_WITNESSES) return;
        if (e < AU_BOOLEANS) {
            const uint8_t* old_leaf = leaves + PY_LEAF_LEN * item;
            const uint8_t* new_leaf = leaves + PY_LEAF_LEN * (A.count + item);
            unsigned byte;
            if (e < AU_KEY_BITS) byte = new_leaf[e >> 3];
            else if (e < AU_KEY_BITS + PY_AMOUNT_BITS) byte = old_leaf[64 + ((e - AU_KEY_BITS) >> 3)];
            else if (e < AU_KEY_BITS + 2 * PY_AMOUNT_BITS) byte = new_leaf[64 + ((e - AU_KEY_BITS - PY_AMOUNT_BITS) >> 3)];
            else byte = ids[item];
            if ((byte >> (e & 7)) & 1u) v = fp_one<Fr>();  // every group starts at a multiple of 8
        } else {
            v = fp_from_std(pt_load(dig_old + 8 * (item * (A.levels + 1))));  // a node: canonical
        }
    }
    uint4* q = reinterpret_cast<uint4*>(witness + item * A.stride + e);
    q[0] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
    q[1] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
}

// n operations on device buffers, in order: d_accounts and the tree's nodes are advanced.  d_w 16-byte aligned; item i's witnesses
// from d_w + i * stride (stride >= the shape's num_witness).
static int au_run(swm_ctx* ctx, const swm_account_update_circuit* c, swm_poseidon_tree* tree, uint8_t* d_accounts, const AuIn& in, size_t n,
                  Fr* d_w, size_t stride, AuOut* out) {
    const AccountUpdateShape& s = c->shape;
    const swm_poseidon* p = c->tree.params;
    const unsigned levels = (unsigned)s.levels;
    AuOut O;
    SWM_TRY(account_update_aux(ctx, "account_update.aux", n, levels, &O));
    SWM_LAUNCH(ctx, "account_update_advance", account_update_advance_kernel, dim3(1), dim3(AU_LANES), pt_lds(p), pt_table(p), pt_params(p),
               levels, n, reinterpret_cast<uint32_t*>(tree->d_nodes), d_accounts, in, O);
    const size_t dig = n * (levels + 1) * 8, leaves = PY_LEAF_LEN * n;
    SWM_TRY(ptw_record(ctx, &c->tree, O.leaves, O.idx, O.dig, O.sib, n, d_w + s.old_at, stride, true));
    SWM_TRY(ptw_record(ctx, &c->tree, O.leaves + leaves, O.idx, O.dig + dig, O.sib, n, d_w + s.new_at, stride, false));
    AuBitsArgs A;
    A.count = n;
    A.stride = stride;
    A.num_witness = s.num_witness;
    A.levels = levels;
    SWM_LAUNCH(ctx, "account_update_bits", account_update_bits_kernel, dim3((unsigned)((s.num_witness * n + AU_LANES - 1) / AU_LANES)),
               dim3(AU_LANES), 0, A, in.ids, (const uint8_t*)O.leaves, (const uint32_t*)O.dig, (const uint8_t*)O.flags, d_w);
    *out = O;
    return SWM_OK;
}

// 32 little-endian bytes as a field element: whatever they hold, reduced (the circuit packs the key's bits unreduced)
static Fr au_key_mont(const uint8_t* b) {
    Fr s, r;
    for (int i = 0; i < 8; i++) r.v[i] = FrParams::P[i];
    (void)ps_load_std(b, &s);
    while (fp_cmp_std(s, r) >= 0) {  // at most 2^256 / r = 13 rounds
        uint64_t borrow = 0;
        for (int i = 0; i < 8; i++) {
            const uint64_t d = (uint64_t)s.v[i] - r.v[i] - borrow;
            s.v[i] = (uint32_t)d;
            borrow = (d >> 32) & 1;
        }
    }
    return fp_from_std(s);
}

// the prover over one item's device witnesses, for both trees; public input one, old_root, new_root, id, key_x, key_y, old_balance,
// new_balance, fresh
int account_update_prove_item(swm_ctx* ctx, const swm_pk* pk, size_t num_witness, size_t num_constraints, const uint8_t* old_root,
                              const uint8_t* new_root, unsigned id, unsigned kind, const uint8_t* old_leaf, const uint8_t* new_leaf, const Fr* d_w,
                              swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len) {
    uint64_t old_balance = 0, new_balance = 0;
    for (int k = 0; k < 8; k++) {
        old_balance |= (uint64_t)old_leaf[64 + k] << (8 * k);
        new_balance |= (uint64_t)new_leaf[64 + k] << (8 * k);
    }
    Fr r0, r1;
    (void)ps_load_std(old_root, &r0);  // nodes of the tree: canonical
    (void)ps_load_std(new_root, &r1);
    const Fr inst[AU_INSTANCE] = {fp_one<Fr>(), fp_from_std(r0), fp_from_std(r1), fp_from_u64<Fr>(id), au_key_mont(new_leaf),
                                  au_key_mont(new_leaf + 32), fp_from_u64<Fr>(old_balance), fp_from_u64<Fr>(new_balance),
                                  fp_from_u64<Fr>(kind)};
    return prove_device_witness(ctx, pk, AU_INSTANCE, num_witness, num_constraints, inst, d_w, rng, flags, proof_out, cap, len);
}

struct AccountUpdateUnit {  // what ledger_witness_host.h drives
    using Circuit = swm_account_update_circuit;
    using Tree = swm_poseidon_tree;
    static constexpr const char* name = "account_update";
    static constexpr const char* accounts_scratch = "account_update.accounts";
    static constexpr const char* witness_scratch = "account_update.w";
    static constexpr auto run = au_run;
    static int check_tree(swm_ctx* ctx, const char* what, const Circuit* c, const Tree* t) {
        return ledger_check_tree(ctx, what, c->tree.params, c->shape.height, t);
    }
};

}  // namespace swm

using namespace swm;

extern "C" {

int swm_account_update_circuit_create(swm_ctx* ctx, const swm_poseidon* poseidon, size_t height, swm_account_update_circuit** out) {
    if (!ctx || !poseidon || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "account_update_circuit_create: bad arguments");
    AccountUpdateShape shape;
    if (!account_update_shape(poseidon->full_rounds, poseidon->partial_rounds, poseidon->alpha, height, &shape))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "account_update_circuit_create: height %zu (%zu <= height <= %zu)", height,
                       (size_t)PY_MIN_HEIGHT, (size_t)PY_MAX_HEIGHT);
    std::unique_ptr<swm_account_update_circuit> c(new swm_account_update_circuit);
    c->tree.params = poseidon;
    c->tree.shape = shape.tree;
    c->shape = shape;
    *out = c.release();
    return SWM_OK;
}

void swm_account_update_circuit_destroy(swm_ctx* ctx, swm_account_update_circuit* c) { destroy_circuit(ctx, c); }

int swm_account_update_witness_at(swm_ctx* ctx, const swm_account_update_circuit* c, swm_poseidon_tree* tree, uint8_t* accounts_inout,
                                  const uint8_t* ids, const uint8_t* kinds, const uint8_t* keys_xy, const uint8_t* balances, size_t count,
                                  uint64_t* witnesses_out, uint8_t* old_roots, uint8_t* new_roots, uint8_t* flags, uint32_t* status) {
    return account_update_witness_at<AccountUpdateUnit>(ctx, c, tree, accounts_inout, ids, kinds, keys_xy, balances, count, witnesses_out, old_roots,
                                                        new_roots, flags, status);
}

int swm_account_update_prove_many_at(swm_ctx* ctx, const swm_pk* pk, const swm_account_update_circuit* c, swm_poseidon_tree* tree,
                                     uint8_t* accounts_inout, const uint8_t* ids, const uint8_t* kinds, const uint8_t* keys_xy,
                                     const uint8_t* balances, size_t count, swm_rng* rng, unsigned prove_flags, uint8_t* proofs_out,
                                     size_t proof_cap, size_t* lens, uint8_t* old_roots, uint8_t* new_roots, uint8_t* flags, uint32_t* status) {
    return account_update_prove_many_at<AccountUpdateUnit>(ctx, pk, c, tree, accounts_inout, ids, kinds, keys_xy, balances, count, rng, prove_flags,
                                                           proofs_out, proof_cap, lens, old_roots, new_roots, flags, status);
}

int swm_account_update_prove_at(swm_ctx* ctx, const swm_pk* pk, const swm_account_update_circuit* c, swm_poseidon_tree* tree,
                                uint8_t* accounts_inout, uint8_t id, uint8_t kind, const uint8_t key_xy[64], uint64_t balance, swm_rng* rng,
                                unsigned prove_flags, uint8_t* proof_out, size_t cap, size_t* len, uint8_t old_root[32], uint8_t new_root[32],
                                uint8_t* flag, uint32_t* status) {
    return account_update_prove_at<AccountUpdateUnit>(ctx, pk, c, tree, accounts_inout, id, kind, key_xy, balance, rng, prove_flags, proof_out,
                                                      cap, len, old_root, new_root, flag, status);
}

}  // extern "C"

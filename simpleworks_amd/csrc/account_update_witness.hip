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
#include <hip/hip_runtime.h>

#include <string.h>

#include <memory>
#include <vector>

#include "context.h"
#include "ff.cuh"
#include "host/account_update_shape.h"
#include "merkle_nodes.cuh"
#include "poseidon.h"
#include "poseidon_tree.h"
#include "swmarlin.h"
#include "witness_host.h"
#include "witness_runs.h"

struct swm_account_update_circuit {
    swm_poseidon_tree_circuit tree;  // over PY_LEAF_LEN bytes
    swm::AccountUpdateShape shape;
};

namespace swm {

static constexpr unsigned AU_LANES = 256;                              // phase 0: a lane per leaf, ids are one byte
static constexpr unsigned AU_MAX_LEAVES = 1u << (PY_MAX_HEIGHT - 1);   // 256
static constexpr unsigned AU_FLAG_APPLIED = 1;
static constexpr unsigned AU_ST_KEY = 1, AU_ST_ID = 2, AU_ST_OCCUPIED = 4, AU_ST_BLANK = 8, AU_ST_ZERO = 16;
static constexpr unsigned AU_KIND_REGISTER = 1;  // kinds[i]: 0 = set balance, 1 = register

__device__ __forceinline__ uint64_t au_load_u64(const uint8_t* b) {
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) v |= (uint64_t)b[k] << (8 * k);
    return v;
}

__device__ __forceinline__ bool au_blank(const uint8_t* leaf) {
    unsigned any = 0;
    for (unsigned k = 0; k < PY_LEAF_LEN; k++) any |= leaf[k];
    return any == 0;
}

__device__ __forceinline__ bool au_canonical(const uint8_t* b) {  // 32 little-endian bytes below r
    Fr x;
#pragma unroll
    for (int w = 0; w < 8; w++)
        x.v[w] = (uint32_t)b[4 * w] | (uint32_t)b[4 * w + 1] << 8 | (uint32_t)b[4 * w + 2] << 16 | (uint32_t)b[4 * w + 3] << 24;
    return pt_canonical(x);
}

__device__ __forceinline__ Fr au_select(bool c, const Fr& a, const Fr& b) {
    Fr x;
#pragma unroll
    for (int w = 0; w < 8; w++) x.v[w] = c ? a.v[w] : b.v[w];
    return x;
}

struct AuIn {  // the block on the device, n = count
    const uint8_t *ids, *kinds, *keys, *balances;  // n | n | 64 n | 8 n bytes
};

struct AuOut {              // what the advance kernel leaves for the record launches and the bits kernel
    uint32_t* dig;          // 2 x n x (L + 1) x 8 words: the old path's nodes | the new leaf's walk
    uint32_t* sib;          // n x L x 8 words: one sibling array, it serves both
    uint8_t* leaves;        // 2 x n x 72 bytes: key || old_balance | key || new_balance
    uint64_t* idx;          // n: the id masked to the tree
    uint32_t* roots;        // 2 x n x 8 words: old roots | new roots
    uint8_t* flags;         // n
    uint32_t* status;       // n
    uint32_t* verdict;      // 1: nonzero when the table is not the tree's
};

// One workgroup.  nodes, accounts: read, and written back at the end unless the call is refused.
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
        const uint64_t old_value = kind == AU_KIND_REGISTER ? 0 : au_load_u64(leaf + 64), new_value = au_load_u64(I.balances + 8 * t);
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
            st = (au_canonical(key) && au_canonical(key + 32) ? 0u : AU_ST_KEY) | (blank ? 0u : AU_ST_OCCUPIED) | (any ? 0u : AU_ST_ZERO);
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

// "account_update.aux" for n operations: every piece a multiple of 8 bytes but the last two
static size_t au_aux_bytes(size_t n, size_t levels) {
    return 4 * (2 * n * (levels + 1) * 8 + n * levels * 8) + 8 * n + 64 * n + 4 * n + 8 + 2 * PY_LEAF_LEN * n + n + 64;
}

// n operations on device buffers, in order: d_accounts and the tree's nodes are advanced.  d_w 16-byte aligned; item i's witnesses
// from d_w + i * stride (stride >= the shape's num_witness).
static int au_run(swm_ctx* ctx, const swm_account_update_circuit* c, swm_poseidon_tree* tree, uint8_t* d_accounts, const AuIn& in, size_t n,
                  Fr* d_w, size_t stride, AuOut* out) {
    const AccountUpdateShape& s = c->shape;
    const swm_poseidon* p = c->tree.params;
    const unsigned levels = (unsigned)s.levels;
    uint8_t* aux = nullptr;
    SWM_TRY(scratch(ctx, "account_update.aux", au_aux_bytes(n, levels), (void**)&aux));
    AuOut O;
    O.dig = reinterpret_cast<uint32_t*>(aux);
    O.sib = O.dig + 2 * n * (levels + 1) * 8;
    O.idx = reinterpret_cast<uint64_t*>(O.sib + n * levels * 8);
    O.roots = reinterpret_cast<uint32_t*>(O.idx + n);
    O.status = O.roots + 16 * n;
    O.verdict = O.status + n;
    O.leaves = reinterpret_cast<uint8_t*>(O.verdict + 2);
    O.flags = O.leaves + 2 * PY_LEAF_LEN * n;
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

static int au_check_tree(swm_ctx* ctx, const char* what, const swm_account_update_circuit* c, const swm_poseidon_tree* t) {
    if (t->params != c->tree.params || t->height != c->shape.height || t->leaf_len != PY_LEAF_LEN)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: a tree of height %zu with %zu-byte leaves for a circuit of height %zu with %zu-byte leaves, "
                       "or other parameters", what, t->height, t->leaf_len, c->shape.height, (size_t)PY_LEAF_LEN);
    return SWM_OK;
}

struct AuBlock {  // the caller's arrays of a whole block; roots may be NULL
    const uint8_t *ids, *kinds, *keys, *balances;
    uint8_t *old_roots, *new_roots, *flags;
    uint32_t* status;
};

// Chunk [base, base + n) of a block: staged, run, its small results copied out and waited for.  The witnesses stay in
// "account_update.w" (*d_w).  leaves (may be NULL): the chunk's 2 x n x 72 leaf bytes, for the prover's public input.
static int au_chunk(swm_ctx* ctx, const char* what, const swm_account_update_circuit* c, swm_poseidon_tree* tree, uint8_t* d_accounts,
                    const AuBlock& b, size_t base, size_t n, Fr** d_w, uint8_t* leaves) {
    const size_t item = c->shape.num_witness * sizeof(Fr);
    uint8_t *d_in = nullptr, *d_out = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", n * (64 + 8 + 2) + 16, (void**)&d_in));
    AuIn in;
    in.keys = d_in;
    in.balances = d_in + 64 * n;
    in.ids = d_in + 72 * n;
    in.kinds = d_in + 73 * n;
    SWM_HIP(ctx, hipMemcpyAsync(d_in, b.keys + 64 * base, 64 * n, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(d_in + 64 * n, b.balances + 8 * base, 8 * n, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(d_in + 72 * n, b.ids + base, n, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(d_in + 73 * n, b.kinds + base, n, hipMemcpyHostToDevice, ctx->stream));
    SWM_TRY(scratch(ctx, "account_update.w", n * item + 16, (void**)&d_out));
    AuOut O;
    SWM_TRY(au_run(ctx, c, tree, d_accounts, in, n, (Fr*)d_out, c->shape.num_witness, &O));
    uint32_t verdict = 0;
    SWM_HIP(ctx, hipMemcpyAsync(&verdict, O.verdict, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (b.old_roots) SWM_HIP(ctx, hipMemcpyAsync(b.old_roots + 32 * base, O.roots, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
    if (b.new_roots) SWM_HIP(ctx, hipMemcpyAsync(b.new_roots + 32 * base, O.roots + 8 * n, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
    if (leaves) SWM_HIP(ctx, hipMemcpyAsync(leaves, O.leaves, 2 * PY_LEAF_LEN * n, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(b.flags + base, O.flags, n, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(b.status + base, O.status, 4 * n, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (verdict) return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: the account table is not the tree's leaf level", what);
    *d_w = (Fr*)d_out;
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

// the prover over one item's device witnesses; public input one, old_root, new_root, id, key_x, key_y, old_balance, new_balance, fresh
static int au_prove_item(swm_ctx* ctx, const swm_pk* pk, const AccountUpdateShape& s, const uint8_t* old_root, const uint8_t* new_root,
                         unsigned id, unsigned kind, const uint8_t* old_leaf, const uint8_t* new_leaf, const Fr* d_w, swm_rng* rng,
                         unsigned flags, uint8_t* proof_out, size_t cap, size_t* len) {
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
    return prove_device_witness(ctx, pk, AU_INSTANCE, s.num_witness, s.num_constraints, inst, d_w, rng, flags, proof_out, cap, len);
}

// the account table (2^levels leaves of 72 bytes) into the unit's scratch buffer
static int au_upload_accounts(swm_ctx* ctx, const uint8_t* accounts, size_t bytes, uint8_t** d_accounts) {
    SWM_TRY(scratch(ctx, "account_update.accounts", bytes + 16, (void**)d_accounts));
    SWM_HIP(ctx, hipMemcpyAsync(*d_accounts, accounts, bytes, hipMemcpyHostToDevice, ctx->stream));
    return SWM_OK;
}

// the table after a chunk and (witness not NULL) the chunk's witnesses back to the host, waited for
static int au_download(swm_ctx* ctx, uint8_t* accounts, const uint8_t* d_accounts, size_t table_bytes, uint8_t* witness, const Fr* d_w,
                       size_t witness_bytes) {
    SWM_HIP(ctx, hipMemcpyAsync(accounts, d_accounts, table_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (witness) SWM_HIP(ctx, hipMemcpyAsync(witness, d_w, witness_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWM_OK;
}

// The block in chunks.  witness (may be NULL): the host copy of every item; pk (may be NULL): one proof per applied operation.
static int au_block(swm_ctx* ctx, const char* what, const swm_pk* pk, const swm_account_update_circuit* c, swm_poseidon_tree* tree,
                    uint8_t* accounts, const AuBlock& b, size_t count, uint64_t* witness, swm_rng* rng, unsigned prove_flags,
                    uint8_t* proofs_out, size_t proof_cap, size_t* lens) {
    const AccountUpdateShape& s = c->shape;
    const size_t num_witness = s.num_witness, item = num_witness * sizeof(Fr), table_bytes = PY_LEAF_LEN << s.levels;
    std::vector<uint8_t> roots, leaves;  // the prover needs the root pairs whether the caller asked for them or not
    AuBlock blk = b;
    if (pk && (!b.old_roots || !b.new_roots)) {
        roots.resize(64 * count);
        if (!b.old_roots) blk.old_roots = roots.data();
        if (!b.new_roots) blk.new_roots = roots.data() + 32 * count;
    }
    uint8_t* d_accounts = nullptr;
    {
        SWM_ON_DEVICE(ctx);
        SWM_TRY(drained(ctx, au_upload_accounts(ctx, accounts, table_bytes, &d_accounts)));
    }
    for (const WitnessChunk ch : WitnessChunks(witness_stage_items(ctx, item), count)) {
        Fr* d_w = nullptr;
        if (pk) leaves.resize(2 * PY_LEAF_LEN * ch.count);
        {
            SWM_ON_DEVICE(ctx);
            SWM_TRY(drained(ctx, au_chunk(ctx, what, c, tree, d_accounts, blk, ch.base, ch.count, &d_w, pk ? leaves.data() : nullptr)));
            // the tree is advanced from here on: the table goes back with it, whatever the prover does below
            SWM_TRY(drained(ctx, au_download(ctx, accounts, d_accounts, table_bytes,
                                             witness ? reinterpret_cast<uint8_t*>(witness) + ch.base * item : nullptr, d_w, ch.count * item)));
        }
        for (size_t i = ch.base; pk && i < ch.base + ch.count; i++) {
            if (!(blk.flags[i] & AU_FLAG_APPLIED)) continue;
            const size_t k = i - ch.base;
            size_t len = 0;
            SWM_TRY(au_prove_item(ctx, pk, s, blk.old_roots + 32 * i, blk.new_roots + 32 * i, b.ids[i], b.kinds[i], leaves.data() + PY_LEAF_LEN * k,
                                  leaves.data() + PY_LEAF_LEN * (ch.count + k), d_w + k * num_witness, rng, prove_flags,
                                  proofs_out + i * proof_cap, proof_cap, &len));
            lens[i] = len;
        }
    }
    return SWM_OK;
}

// what both block entries refuse before anything runs
static int au_check_block(swm_ctx* ctx, const char* what, const swm_account_update_circuit* c, const swm_poseidon_tree* tree,
                          const uint8_t* kinds, size_t count) {
    SWM_TRY(au_check_tree(ctx, what, c, tree));
    if (count > 0x7FFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: %zu operations in one call", what, count);
    for (size_t i = 0; i < count; i++)
        if (kinds[i] > AU_KIND_REGISTER)
            return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: operation %zu: kind %u (0 = set balance, 1 = register)", what, i, (unsigned)kinds[i]);
    return SWM_OK;
}

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
    const char* what = "account_update_witness_at";
    if (!ctx || !c || !tree || !accounts_inout ||
        (count && (!ids || !kinds || !keys_xy || !balances || !witnesses_out || !old_roots || !new_roots || !flags || !status)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what);
    SWM_TRY(au_check_block(ctx, what, c, tree, kinds, count));
    if (!count) return SWM_OK;
    const AuBlock b = {ids, kinds, keys_xy, balances, old_roots, new_roots, flags, status};
    return au_block(ctx, what, nullptr, c, tree, accounts_inout, b, count, witnesses_out, nullptr, 0, nullptr, 0, nullptr);
}

int swm_account_update_prove_many_at(swm_ctx* ctx, const swm_pk* pk, const swm_account_update_circuit* c, swm_poseidon_tree* tree,
                                     uint8_t* accounts_inout, const uint8_t* ids, const uint8_t* kinds, const uint8_t* keys_xy,
                                     const uint8_t* balances, size_t count, swm_rng* rng, unsigned prove_flags, uint8_t* proofs_out,
                                     size_t proof_cap, size_t* lens, uint8_t* old_roots, uint8_t* new_roots, uint8_t* flags, uint32_t* status) {
    const char* what = "account_update_prove_many_at";
    if (!ctx || !pk || !c || !tree || !accounts_inout || !rng ||
        (count && (!ids || !kinds || !keys_xy || !balances || !proofs_out || !lens || !flags || !status)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what);
    SWM_TRY(au_check_block(ctx, what, c, tree, kinds, count));
    // the tree is advanced before the proofs are made: a key of another shape is refused while nothing has changed
    if (!pk_takes_shape(pk, c->shape.num_instance, c->shape.num_witness, c->shape.num_constraints))
        return set_err(ctx, SWM_ERR_MISMATCH, "%s: the proving key is not that of this circuit", what);
    if (!count) return SWM_OK;
    for (size_t i = 0; i < count; i++) {  // whatever ends the call, every entry has been written
        lens[i] = 0;
        flags[i] = 0;
        status[i] = 0;
    }
    const AuBlock b = {ids, kinds, keys_xy, balances, old_roots, new_roots, flags, status};
    return au_block(ctx, what, pk, c, tree, accounts_inout, b, count, nullptr, rng, prove_flags, proofs_out, proof_cap, lens);
}

int swm_account_update_prove_at(swm_ctx* ctx, const swm_pk* pk, const swm_account_update_circuit* c, swm_poseidon_tree* tree,
                                uint8_t* accounts_inout, uint8_t id, uint8_t kind, const uint8_t key_xy[64], uint64_t balance, swm_rng* rng,
                                unsigned prove_flags, uint8_t* proof_out, size_t cap, size_t* len, uint8_t old_root[32], uint8_t new_root[32],
                                uint8_t* flag, uint32_t* status) {
    if (!key_xy || !proof_out || !len || !old_root || !new_root || !flag || !status)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "account_update_prove_at: bad arguments");
    uint8_t b[8];
    for (int k = 0; k < 8; k++) b[k] = (uint8_t)(balance >> (8 * k));
    return swm_account_update_prove_many_at(ctx, pk, c, tree, accounts_inout, &id, &kind, key_xy, b, 1, rng, prove_flags, proof_out, cap, len,
                                            old_root, new_root, flag, status);
}

}  // extern "C"

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
#include <hip/hip_runtime.h>

#include <string.h>

#include <memory>
#include <vector>

#include "context.h"
#include "ff.cuh"
#include "host/pedersen_account_update_shape.h"
#include "merkle_nodes.cuh"
#include "merkle_tree.h"
#include "pedersen.cuh"
#include "pedersen.h"
#include "swmarlin.h"
#include "witness_host.h"
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
static constexpr unsigned PAU_FLAG_APPLIED = 1;
static constexpr unsigned PAU_ST_KEY = 1, PAU_ST_ID = 2, PAU_ST_OCCUPIED = 4, PAU_ST_BLANK = 8, PAU_ST_ZERO = 16;
static constexpr unsigned PAU_KIND_REGISTER = 1;  // kinds[i]: 0 = set balance, 1 = register

__device__ __forceinline__ uint64_t pau_load_u64(const uint8_t* b) {
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) v |= (uint64_t)b[k] << (8 * k);
    return v;
}

__device__ __forceinline__ bool pau_canonical(const uint8_t* b) {  // 32 little-endian bytes below r
    Fr x, r;
#pragma unroll
    for (int w = 0; w < 8; w++) {
        x.v[w] = (uint32_t)b[4 * w] | (uint32_t)b[4 * w + 1] << 8 | (uint32_t)b[4 * w + 2] << 16 | (uint32_t)b[4 * w + 3] << 24;
        r.v[w] = FrParams::P[w];
    }
    return fp_cmp_std(x, r) < 0;
}

struct PauIn {  // the block on the device, n = count
    const uint8_t *ids, *kinds, *keys, *balances;  // n | n | 64 n | 8 n bytes
};

struct PauOut {             // what the advance kernel leaves for the record launches and the bits kernel
    uint32_t* dig;          // 2 x n x (L + 1) x 8 words: the old path's nodes | the new leaf's walk
    uint32_t* sib;          // n x L x 8 words: one sibling array, it serves both
    uint8_t* leaves;        // 2 x n x 72 bytes: the old leaf (72 zero bytes for a registration) | key || new_balance
    uint64_t* idx;          // n: the id masked to the tree
    uint32_t* roots;        // 2 x n x 8 words: old roots | new roots
    uint8_t* flags;         // n
    uint32_t* status;       // n
    uint32_t* verdict;      // 1: nonzero when the table is not the tree's (the check kernel's)
};

// One workgroup, one wave.  nodes, accounts: read, and written back at the end unless the call is refused.
__global__ void __launch_bounds__(PAU_LANES) pedersen_account_update_advance_kernel(const EdRow* __restrict__ leaf_table, unsigned leaf_windows,
                                                                                    const EdRow* __restrict__ inner_table, unsigned inner_windows,
                                                                                    unsigned levels, size_t count, uint32_t* __restrict__ nodes,
                                                                                    uint8_t* __restrict__ accounts, PauIn I, Fr k2d, PauOut O) {
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
        const bool reg = kind == PAU_KIND_REGISTER;
        const uint8_t* leaf = s_acc + PP_LEAF_LEN * m;
        const uint8_t* key = reg ? I.keys + 64 * t : leaf;
        const uint64_t new_value = pau_load_u64(I.balances + 8 * t);
        // the decision: every lane reads the same bytes and takes the same one
        unsigned held = 0, any = 0;
        for (unsigned k = 0; k < PP_LEAF_LEN; k++) held |= leaf[k];
        for (unsigned k = 0; k < 64; k++) any |= key[k];
        any |= new_value != 0;
        unsigned st = 0;
        if (id >> levels) st = PAU_ST_ID;  // there is no leaf to say more about
        else if (reg)
            st = (pau_canonical(key) && pau_canonical(key + 32) ? 0u : PAU_ST_KEY) | (held ? PAU_ST_OCCUPIED : 0u) | (any ? 0u : PAU_ST_ZERO);
        else
            st = held ? 0u : PAU_ST_BLANK;
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
            O.flags[t] = applied ? (uint8_t)PAU_FLAG_APPLIED : (uint8_t)0;
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
    if (flags[item] & PAU_FLAG_APPLIED) {
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

// "paccount_update.aux" for n operations: every piece a multiple of 8 bytes but the last two
static size_t pau_aux_bytes(size_t n, size_t levels) {
    return 4 * (2 * n * (levels + 1) * 8 + n * levels * 8) + 8 * n + 64 * n + 4 * n + 8 + 2 * PP_LEAF_LEN * n + n + 64;
}

// n operations on device buffers, in order: d_accounts and the tree's nodes are advanced.  d_w 16-byte aligned; item i's witnesses
// from d_w + i * stride (stride >= the shape's num_witness).
static int pau_run(swm_ctx* ctx, const swm_pedersen_account_update_circuit* c, swm_merkle_tree* tree, uint8_t* d_accounts, const PauIn& in,
                   size_t n, Fr* d_w, size_t stride, PauOut* out) {
    const PedersenAccountUpdateShape& s = c->shape;
    const unsigned levels = (unsigned)s.levels, n_leaves = 1u << levels;
    uint8_t* aux = nullptr;
    SWM_TRY(scratch(ctx, "paccount_update.aux", pau_aux_bytes(n, levels), (void**)&aux));
    PauOut O;
    O.dig = reinterpret_cast<uint32_t*>(aux);
    O.sib = O.dig + 2 * n * (levels + 1) * 8;
    O.idx = reinterpret_cast<uint64_t*>(O.sib + n * levels * 8);
    O.roots = reinterpret_cast<uint32_t*>(O.idx + n);
    O.status = O.roots + 16 * n;
    O.verdict = O.status + n;
    O.leaves = reinterpret_cast<uint8_t*>(O.verdict + 2);
    O.flags = O.leaves + 2 * PP_LEAF_LEN * n;
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

static int pau_check_tree(swm_ctx* ctx, const char* what, const swm_pedersen_account_update_circuit* c, const swm_merkle_tree* t) {
    if (t->leaf != c->leaf || t->inner != c->inner || t->height != c->shape.height || t->leaf_len != PP_LEAF_LEN)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: a tree of height %zu with %zu-byte leaves for a circuit of height %zu with %zu-byte leaves, "
                       "or other parameters", what, t->height, t->leaf_len, c->shape.height, (size_t)PP_LEAF_LEN);
    return SWM_OK;
}

struct PauBlock {  // the caller's arrays of a whole block; roots may be NULL
    const uint8_t *ids, *kinds, *keys, *balances;
    uint8_t *old_roots, *new_roots, *flags;
    uint32_t* status;
};

// Chunk [base, base + n) of a block: staged, run, its small results copied out and waited for.  The witnesses stay in
// "paccount_update.w" (*d_w).  leaves (may be NULL): the chunk's 2 x n x 72 leaf bytes, for the prover's public input.
static int pau_chunk(swm_ctx* ctx, const char* what, const swm_pedersen_account_update_circuit* c, swm_merkle_tree* tree, uint8_t* d_accounts,
                     const PauBlock& b, size_t base, size_t n, Fr** d_w, uint8_t* leaves) {
    const size_t item = c->shape.num_witness * sizeof(Fr);
    uint8_t *d_in = nullptr, *d_out = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", n * (64 + 8 + 2) + 16, (void**)&d_in));
    PauIn in;
    in.keys = d_in;
    in.balances = d_in + 64 * n;
    in.ids = d_in + 72 * n;
    in.kinds = d_in + 73 * n;
    SWM_HIP(ctx, hipMemcpyAsync(d_in, b.keys + 64 * base, 64 * n, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(d_in + 64 * n, b.balances + 8 * base, 8 * n, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(d_in + 72 * n, b.ids + base, n, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(d_in + 73 * n, b.kinds + base, n, hipMemcpyHostToDevice, ctx->stream));
    SWM_TRY(scratch(ctx, "paccount_update.w", n * item + 16, (void**)&d_out));
    PauOut O;
    SWM_TRY(pau_run(ctx, c, tree, d_accounts, in, n, (Fr*)d_out, c->shape.num_witness, &O));
    uint32_t verdict = 0;
    SWM_HIP(ctx, hipMemcpyAsync(&verdict, O.verdict, 4, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (verdict) return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: the account table is not the tree's leaf level", what);
    if (b.old_roots) SWM_HIP(ctx, hipMemcpyAsync(b.old_roots + 32 * base, O.roots, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
    if (b.new_roots) SWM_HIP(ctx, hipMemcpyAsync(b.new_roots + 32 * base, O.roots + 8 * n, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
    if (leaves) SWM_HIP(ctx, hipMemcpyAsync(leaves, O.leaves, 2 * PP_LEAF_LEN * n, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(b.flags + base, O.flags, n, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(b.status + base, O.status, 4 * n, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *d_w = (Fr*)d_out;
    return SWM_OK;
}

// 32 little-endian bytes as a field element: whatever they hold, reduced (the circuit packs the key's bits unreduced)
static Fr pau_key_mont(const uint8_t* b) {
    Fr s, r;
    for (int i = 0; i < 8; i++) {
        s.v[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
        r.v[i] = FrParams::P[i];
    }
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

static Fr pau_root_mont(const uint8_t* b) {  // a node of the tree: canonical
    Fr s;
    for (int i = 0; i < 8; i++) s.v[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
    return fp_from_std(s);
}

// the prover over one item's device witnesses; public input one, old_root, new_root, id, key_x, key_y, old_balance, new_balance, fresh
static int pau_prove_item(swm_ctx* ctx, const swm_pk* pk, const PedersenAccountUpdateShape& s, const uint8_t* old_root, const uint8_t* new_root,
                          unsigned id, unsigned kind, const uint8_t* old_leaf, const uint8_t* new_leaf, const Fr* d_w, swm_rng* rng,
                          unsigned flags, uint8_t* proof_out, size_t cap, size_t* len) {
    uint64_t old_balance = 0, new_balance = 0;
    for (int k = 0; k < 8; k++) {
        old_balance |= (uint64_t)old_leaf[64 + k] << (8 * k);
        new_balance |= (uint64_t)new_leaf[64 + k] << (8 * k);
    }
    const Fr inst[PAU_INSTANCE] = {fp_one<Fr>(), pau_root_mont(old_root), pau_root_mont(new_root), fp_from_u64<Fr>(id), pau_key_mont(new_leaf),
                                   pau_key_mont(new_leaf + 32), fp_from_u64<Fr>(old_balance), fp_from_u64<Fr>(new_balance),
                                   fp_from_u64<Fr>(kind)};
    return prove_device_witness(ctx, pk, PAU_INSTANCE, s.num_witness, s.num_constraints, inst, d_w, rng, flags, proof_out, cap, len);
}

// the account table (2^levels leaves of 72 bytes) into the unit's scratch buffer
static int pau_upload_accounts(swm_ctx* ctx, const uint8_t* accounts, size_t bytes, uint8_t** d_accounts) {
    SWM_TRY(scratch(ctx, "paccount_update.accounts", bytes + 16, (void**)d_accounts));
    SWM_HIP(ctx, hipMemcpyAsync(*d_accounts, accounts, bytes, hipMemcpyHostToDevice, ctx->stream));
    return SWM_OK;
}

// the table after a chunk and (witness not NULL) the chunk's witnesses back to the host, waited for
static int pau_download(swm_ctx* ctx, uint8_t* accounts, const uint8_t* d_accounts, size_t table_bytes, uint8_t* witness, const Fr* d_w,
                        size_t witness_bytes) {
    SWM_HIP(ctx, hipMemcpyAsync(accounts, d_accounts, table_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (witness) SWM_HIP(ctx, hipMemcpyAsync(witness, d_w, witness_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWM_OK;
}

// The block in chunks.  witness (may be NULL): the host copy of every item; pk (may be NULL): one proof per applied operation.
static int pau_block(swm_ctx* ctx, const char* what, const swm_pk* pk, const swm_pedersen_account_update_circuit* c, swm_merkle_tree* tree,
                     uint8_t* accounts, const PauBlock& b, size_t count, uint64_t* witness, swm_rng* rng, unsigned prove_flags,
                     uint8_t* proofs_out, size_t proof_cap, size_t* lens) {
    const PedersenAccountUpdateShape& s = c->shape;
    const size_t num_witness = s.num_witness, item = num_witness * sizeof(Fr), table_bytes = PP_LEAF_LEN << s.levels;
    std::vector<uint8_t> roots, leaves;  // the prover needs the root pairs whether the caller asked for them or not
    PauBlock blk = b;
    if (pk && (!b.old_roots || !b.new_roots)) {
        roots.resize(64 * count);
        if (!b.old_roots) blk.old_roots = roots.data();
        if (!b.new_roots) blk.new_roots = roots.data() + 32 * count;
    }
    uint8_t* d_accounts = nullptr;
    {
        SWM_ON_DEVICE(ctx);
        SWM_TRY(drained(ctx, pau_upload_accounts(ctx, accounts, table_bytes, &d_accounts)));
    }
    for (const WitnessChunk ch : WitnessChunks(witness_stage_items(ctx, item), count)) {
        Fr* d_w = nullptr;
        if (pk) leaves.resize(2 * PP_LEAF_LEN * ch.count);
        {
            SWM_ON_DEVICE(ctx);
            SWM_TRY(drained(ctx, pau_chunk(ctx, what, c, tree, d_accounts, blk, ch.base, ch.count, &d_w, pk ? leaves.data() : nullptr)));
            // the tree is advanced from here on: the table goes back with it, whatever the prover does below
            SWM_TRY(drained(ctx, pau_download(ctx, accounts, d_accounts, table_bytes,
                                              witness ? reinterpret_cast<uint8_t*>(witness) + ch.base * item : nullptr, d_w, ch.count * item)));
        }
        for (size_t i = ch.base; pk && i < ch.base + ch.count; i++) {
            if (!(blk.flags[i] & PAU_FLAG_APPLIED)) continue;
            const size_t k = i - ch.base;
            size_t len = 0;
            SWM_TRY(pau_prove_item(ctx, pk, s, blk.old_roots + 32 * i, blk.new_roots + 32 * i, b.ids[i], b.kinds[i], leaves.data() + PP_LEAF_LEN * k,
                                   leaves.data() + PP_LEAF_LEN * (ch.count + k), d_w + k * num_witness, rng, prove_flags,
                                   proofs_out + i * proof_cap, proof_cap, &len));
            lens[i] = len;
        }
    }
    return SWM_OK;
}

// what both block entries refuse before anything runs
static int pau_check_block(swm_ctx* ctx, const char* what, const swm_pedersen_account_update_circuit* c, const swm_merkle_tree* tree,
                           const uint8_t* kinds, size_t count) {
    SWM_TRY(pau_check_tree(ctx, what, c, tree));
    if (count > 0x7FFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: %zu operations in one call", what, count);
    for (size_t i = 0; i < count; i++)
        if (kinds[i] > PAU_KIND_REGISTER)
            return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: operation %zu: kind %u (0 = set balance, 1 = register)", what, i, (unsigned)kinds[i]);
    return SWM_OK;
}

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
    if (leaf->window_size != 4 || inner->window_size != 4)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "pedersen_account_update_circuit_create: windows of %u and %u bits (4 is required)",
                       leaf->window_size, inner->window_size);
    if (leaf->num_windows < PP_LEAF_WINDOWS || inner->num_windows < PP_INNER_WINDOWS)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "pedersen_account_update_circuit_create: %u leaf and %u two-to-one windows (at least %zu and "
                       "%zu are required)", leaf->num_windows, inner->num_windows, (size_t)PP_LEAF_WINDOWS, (size_t)PP_INNER_WINDOWS);
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
    const char* what = "pedersen_account_update_witness_at";
    if (!ctx || !c || !tree || !accounts_inout ||
        (count && (!ids || !kinds || !keys_xy || !balances || !witnesses_out || !old_roots || !new_roots || !flags || !status)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what);
    SWM_TRY(pau_check_block(ctx, what, c, tree, kinds, count));
    if (!count) return SWM_OK;
    const PauBlock b = {ids, kinds, keys_xy, balances, old_roots, new_roots, flags, status};
    return pau_block(ctx, what, nullptr, c, tree, accounts_inout, b, count, witnesses_out, nullptr, 0, nullptr, 0, nullptr);
}

int swm_pedersen_account_update_prove_many_at(swm_ctx* ctx, const swm_pk* pk, const swm_pedersen_account_update_circuit* c,
                                              swm_merkle_tree* tree, uint8_t* accounts_inout, const uint8_t* ids, const uint8_t* kinds,
                                              const uint8_t* keys_xy, const uint8_t* balances, size_t count, swm_rng* rng,
                                              unsigned prove_flags, uint8_t* proofs_out, size_t proof_cap, size_t* lens, uint8_t* old_roots,
                                              uint8_t* new_roots, uint8_t* flags, uint32_t* status) {
    const char* what = "pedersen_account_update_prove_many_at";
    if (!ctx || !pk || !c || !tree || !accounts_inout || !rng ||
        (count && (!ids || !kinds || !keys_xy || !balances || !proofs_out || !lens || !flags || !status)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what);
    SWM_TRY(pau_check_block(ctx, what, c, tree, kinds, count));
    // the tree is advanced before the proofs are made: a key of another shape is refused while nothing has changed
    if (!pk_takes_shape(pk, c->shape.num_instance, c->shape.num_witness, c->shape.num_constraints))
        return set_err(ctx, SWM_ERR_MISMATCH, "%s: the proving key is not that of this circuit", what);
    if (!count) return SWM_OK;
    for (size_t i = 0; i < count; i++) {  // whatever ends the call, every entry has been written
        lens[i] = 0;
        flags[i] = 0;
        status[i] = 0;
    }
    const PauBlock b = {ids, kinds, keys_xy, balances, old_roots, new_roots, flags, status};
    return pau_block(ctx, what, pk, c, tree, accounts_inout, b, count, nullptr, rng, prove_flags, proofs_out, proof_cap, lens);
}

int swm_pedersen_account_update_prove_at(swm_ctx* ctx, const swm_pk* pk, const swm_pedersen_account_update_circuit* c, swm_merkle_tree* tree,
                                         uint8_t* accounts_inout, uint8_t id, uint8_t kind, const uint8_t key_xy[64], uint64_t balance,
                                         swm_rng* rng, unsigned prove_flags, uint8_t* proof_out, size_t cap, size_t* len,
                                         uint8_t old_root[32], uint8_t new_root[32], uint8_t* flag, uint32_t* status) {
    if (!key_xy || !proof_out || !len || !old_root || !new_root || !flag || !status)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "pedersen_account_update_prove_at: bad arguments");
    uint8_t b[8];
    for (int k = 0; k < 8; k++) b[k] = (uint8_t)(balance >> (8 * k));
    return swm_pedersen_account_update_prove_many_at(ctx, pk, c, tree, accounts_inout, &id, &kind, key_xy, b, 1, rng, prove_flags, proof_out, cap,
                                                     len, old_root, new_root, flag, status);
}

}  // extern "C"

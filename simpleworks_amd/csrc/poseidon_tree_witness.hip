// poseidon_tree_witness.hip — the witness of the membership circuit over a Poseidon Merkle tree, synthesised on the GPU, and the
// proof entries on top of it.  The statement: "the public leaf bytes hash to a leaf of the tree with public root"; index and path
// are the witness.  Order and values are those of simpleworks_amd/workloads.py, build_poseidon_membership: that function is the
// specification, host/poseidon_tree_shape.h the counts and offsets.
//
// A path's permutations only look sequential: once the running digests cur_0 .. cur_L are known, the leaf sponge and the L level
// permutations are independent of each other.  Two phases:
//   digests   with a resident tree a gather: cur_l = node[l][index >> l], sibling_l = node[l][(index >> l) ^ 1];
//             without one the walk of swm_poseidon_verify_paths (pt_walk, the same device function), one lane per path, storing
//             every level's digest to scratch.
//   record    one lane per (path, unit), one wave per workgroup, the table in LDS.  Unit 0 is the leaf sponge, its P_leaf
//             permutations in sequence; unit l + 1 is level l: d_l = b_l (s_l - cur_l) in ff.cuh arithmetic, then b_l, s_l, d_l
//             are stored, (cur_l + d_l, s_l - d_l) — the two digests in hashing order — enter as absorbed elements and
//             pw_permute records at the level's offset.  The first ceil(count / 64) workgroups take the leaf units, the others
//             the level units, so a workgroup holds one kind.
// The recording arithmetic and its bounds are those of poseidon_witness.hip; the inputs' bounds those of poseidon_tree.h.
// With a resident tree nothing checks that the leaf bytes are the tree's leaf: the leaf sponge then records another digest than
// the gathered cur_0 and the system is unsatisfied, which the prover reports.
#include <hip/hip_runtime.h>

#include <string.h>

#include <memory>
#include <vector>

#include "context.h"
#include "ff.cuh"
#include "fr29.cuh"
#include "host/poseidon_tree_shape.h"
#include "poseidon.h"
#include "poseidon_record.cuh"
#include "poseidon_tree.h"
#include "merkle_nodes.cuh"
#include "swmarlin.h"
#include "witness_runs.h"
#include "witness_host.h"

namespace swm {

// digests: count x (L + 1) x 8 words, cur_0 .. cur_L of every path; roots (may be NULL): cur_L
__global__ void __launch_bounds__(PS_LANES) poseidon_tree_walk_kernel(const uint4* __restrict__ table, PtParams P, unsigned levels,
                                                                      const uint8_t* __restrict__ leaves, size_t leaf_len,
                                                                      const uint64_t* __restrict__ indices, const uint8_t* __restrict__ siblings,
                                                                      size_t count, uint32_t* __restrict__ digests, uint32_t* __restrict__ roots) {
    SWM_LIGHT_KERNEL();
    extern __shared__ __align__(16) uint32_t ps_tab[];
    pt_load_table(ps_tab, table, P.rows);
    const size_t p = blockIdx.x * (size_t)PS_LANES + threadIdx.x;
    if (p >= count) return;
    unsigned bad = 0;
    const Fr top = pt_walk(ps_tab, P, leaves, p, leaf_len, indices[p], reinterpret_cast<const uint32_t*>(siblings + p * (size_t)levels * 32),
                           levels, digests + 8 * p * (levels + 1), bad);
    if (roots) pt_store(roots + 8 * p, top);
}

// word i of (digests | siblings): from the nodes of a resident tree.  The caller has checked index < 2^L.
__global__ void __launch_bounds__(256) poseidon_tree_gather_kernel(const uint32_t* __restrict__ nodes, unsigned levels,
                                                                   const uint64_t* __restrict__ indices, size_t count,
                                                                   uint32_t* __restrict__ digests, uint32_t* __restrict__ siblings) {
    const size_t dig_words = count * (levels + 1) * 8, words = dig_words + count * levels * 8;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
        const bool sib = i >= dig_words;
        const size_t k = sib ? i - dig_words : i, per = sib ? levels : levels + 1;
        const size_t s = k >> 3, p = s / per;
        const unsigned l = (unsigned)(s % per);
        const uint64_t at = (indices[p] >> l) ^ (sib ? 1u : 0u);
        const uint32_t v = nodes[8 * (mt_level_offset(levels, l) + at) + (k & 7)];
        if (sib) siblings[k] = v;
        else digests[k] = v;
    }
}

struct PtwArgs {
    unsigned levels, leaf_blocks, own_path;
    size_t leaf_len, n_elems, count, stride, bits_at, siblings_at, deltas_at, leaf_at, levels_at, perm_values;
};

__device__ __forceinline__ void ptw_store(Fr* dst, const Fr& v) {
    uint4* q = reinterpret_cast<uint4*>(dst);
    q[0] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
    q[1] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
}

__global__ void __launch_bounds__(PS_LANES) poseidon_tree_record_kernel(const uint4* __restrict__ table, PwArgs A, PtwArgs T,
                                                                        const uint8_t* __restrict__ leaves, const uint64_t* __restrict__ indices,
                                                                        const uint32_t* __restrict__ siblings,
                                                                        const uint32_t* __restrict__ digests, Fr* __restrict__ witness) {
    SWM_LIGHT_KERNEL();
    extern __shared__ __align__(16) uint32_t ps_tab[];
    pt_load_table(ps_tab, table, A.rows);
    const int alpha_top = 31 - __clz((int)A.alpha);
    const Fr29 to_mont = ps_row(ps_tab, 0);
    Fr29 s0, s1, s2;
#pragma unroll
    for (int i = 0; i < 9; i++) s0.l[i] = s1.l[i] = s2.l[i] = 0;
    if (blockIdx.x < T.leaf_blocks) {
        // unit 0: the leaf sponge.  An idle lane recomputes the last path's and stores nothing.
        const size_t lane_item = blockIdx.x * (size_t)PS_LANES + threadIdx.x;
        const bool act = lane_item < T.count;
        const size_t item = act ? lane_item : T.count - 1;
        Fr* wp = witness + item * T.stride + T.leaf_at;
        bool unused = false;
#pragma unroll 1
        for (size_t e = 0; e < T.n_elems; e += 2) {
            if (e) pw_permute(ps_tab, A, alpha_top, s0, s1, s2, wp, act, 0xFFFFFFFFu);
            s0 = fr29_add(s0, fr29_mul_fenced(fr29_unpack(ps_fetch<true>(leaves, item, T.leaf_len, e, unused)), to_mont));
            if (e + 1 < T.n_elems)
                s1 = fr29_add(s1, fr29_mul_fenced(fr29_unpack(ps_fetch<true>(leaves, item, T.leaf_len, e + 1, unused)), to_mont));
        }
        pw_permute(ps_tab, A, alpha_top, s0, s1, s2, wp, act, 0xFFFFFFFFu);
        return;
    }
    // unit l + 1: level l of path p
    const size_t units = T.count * T.levels, lane_unit = (blockIdx.x - T.leaf_blocks) * (size_t)PS_LANES + threadIdx.x;
    const bool act = lane_unit < units;
    const size_t unit = act ? lane_unit : units - 1;
    const size_t p = unit / T.levels;
    const unsigned l = (unsigned)(unit % T.levels);
    const Fr cur = pt_load(digests + 8 * (p * (T.levels + 1) + l)), s = pt_load(siblings + 8 * (p * T.levels + l));
    const bool right = (indices[p] >> l) & 1u;
    const Fr d = right ? fp_sub(s, cur) : fp_zero<Fr>();  // both < r: the difference mod r, in standard form as they are
    Fr* w = witness + p * T.stride;
    if (act) {
        if (T.own_path) {
            ptw_store(w + T.bits_at + l, right ? fp_one<Fr>() : fp_zero<Fr>());
            ptw_store(w + T.siblings_at + l, fp_from_std(s));
        }
        ptw_store(w + T.deltas_at + l, fp_from_std(d));
    }
    s0 = fr29_mul_fenced(fr29_unpack(right ? s : cur), to_mont);  // cur_l + d_l
    s1 = fr29_mul_fenced(fr29_unpack(right ? cur : s), to_mont);  // s_l - d_l
    Fr* wp = w + T.levels_at + (size_t)l * T.perm_values;
    pw_permute(ps_tab, A, alpha_top, s0, s1, s2, wp, act, 0xFFFFFFFFu);
}

// The record half: `count` blocks from given digests (count x (L + 1) x 8 words, cur_0 .. cur_L) and siblings (count x L x 8 words).
// own_path false: an update block, which walks another block's path again: no b_l and s_l are stored and its groups start 2 L
// elements earlier (deltas | leaf chain | levels).
int ptw_record(swm_ctx* ctx, const swm_poseidon_tree_circuit* c, const uint8_t* d_leaves, const uint64_t* d_indices, const uint32_t* d_dig,
               const uint32_t* d_sib, size_t count, Fr* d_witness, size_t stride, bool own_path) {
    if (!count) return SWM_OK;
    const PoseidonTreeShape& s = c->shape;
    const swm_poseidon* p = c->params;
    const unsigned levels = (unsigned)s.levels;
    PwArgs A = {};
    A.rows = (unsigned)p->rows;
    A.half_full = p->full_rounds / 2;
    A.partial = p->partial_rounds;
    A.alpha = p->alpha;
    A.chain = (unsigned)s.chain;
    pw_std_limbs(fp_one<Fr>(), &A.to_std);  // the words of Montgomery(1) ARE 2^256 mod r
    PtwArgs T = {};
    T.levels = levels;
    T.leaf_blocks = pt_blocks(count);
    T.leaf_len = s.leaf_len;
    T.n_elems = s.elems;
    T.count = count;
    T.stride = stride;
    const size_t skip = own_path ? 0 : 2 * s.levels;
    T.own_path = own_path ? 1u : 0u;
    T.bits_at = s.bits_at;
    T.siblings_at = s.siblings_at;
    T.deltas_at = s.deltas_at - skip;
    T.leaf_at = s.leaf_at - skip;
    T.levels_at = s.levels_at - skip;
    T.perm_values = s.perm_values;
    SWM_LAUNCH(ctx, "poseidon_tree_record", poseidon_tree_record_kernel, dim3(T.leaf_blocks + pt_blocks(count * levels)), dim3(PS_LANES),
               pt_lds(p), pt_table(p), A, T, d_leaves, d_indices, d_sib, d_dig, d_witness);
    return SWM_OK;
}

// `count` witnesses into d_witness (item i at d_witness + i * stride, 16-byte aligned).  With a tree the digests and the siblings are
// gathered from its nodes (d_siblings is not read); without one the paths are walked and d_roots (may be NULL) takes their roots.
int ptw_run(swm_ctx* ctx, const swm_poseidon_tree_circuit* c, const swm_poseidon_tree* tree, const uint8_t* d_leaves, const uint64_t* d_indices,
            const uint8_t* d_siblings, size_t count, Fr* d_witness, size_t stride, uint32_t* d_roots) {
    if (!count) return SWM_OK;
    const PoseidonTreeShape& s = c->shape;
    const swm_poseidon* p = c->params;
    const unsigned levels = (unsigned)s.levels;
    const size_t dig_words = count * (levels + 1) * 8;
    uint32_t* d_dig = nullptr;
    SWM_TRY(scratch(ctx, "ptree.digests", (dig_words + count * levels * 8) * 4, (void**)&d_dig));
    const uint32_t* d_sib = reinterpret_cast<const uint32_t*>(d_siblings);
    if (tree) {
        const size_t words = dig_words + count * levels * 8;
        const unsigned blocks = (unsigned)std::min<size_t>((words + 255) / 256, 1u << 16);
        SWM_LAUNCH(ctx, "poseidon_tree_gather", poseidon_tree_gather_kernel, dim3(blocks), dim3(256), 0,
                   reinterpret_cast<const uint32_t*>(tree->d_nodes), levels, d_indices, count, d_dig, d_dig + dig_words);
        d_sib = d_dig + dig_words;
    } else {
        SWM_LAUNCH(ctx, "poseidon_tree_walk", poseidon_tree_walk_kernel, dim3(pt_blocks(count)), dim3(PS_LANES), pt_lds(p), pt_table(p),
                   pt_params(p), levels, d_leaves, s.leaf_len, d_indices, d_siblings, count, d_dig, d_roots);
    }
    return ptw_record(ctx, c, d_leaves, d_indices, d_dig, d_sib, count, d_witness, stride, true);
}

// the host forms' checks: an index < 2^L, every sibling (may be NULL: a resident tree's) a canonical field element
static int ptw_check_paths(swm_ctx* ctx, const char* what, const PoseidonTreeShape& s, const uint64_t* indices, const uint8_t* siblings,
                           size_t count) {
    Fr v;
    for (size_t p = 0; p < count; p++) {
        if (indices[p] >> s.levels)
            return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: path %zu: leaf index %llu in a tree of height %zu", what, p,
                           (unsigned long long)indices[p], s.height);
        for (size_t l = 0; siblings && l < s.levels; l++)
            if (!ps_load_std(siblings + 32 * (p * s.levels + l), &v))
                return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: path %zu: sibling %zu is not a canonical field element", what, p, l);
    }
    return SWM_OK;
}

static int ptw_check_tree(swm_ctx* ctx, const char* what, const swm_poseidon_tree_circuit* c, const swm_poseidon_tree* t) {
    if (t->params != c->params || t->height != c->shape.height || t->leaf_len != c->shape.leaf_len)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: a tree of height %zu with %zu-byte leaves for a circuit of height %zu with %zu-byte leaves, "
                       "or other parameters", what, t->height, t->leaf_len, c->shape.height, c->shape.leaf_len);
    return SWM_OK;
}

// indices | siblings | leaves of n paths into "stage.a"
static int ptw_stage(swm_ctx* ctx, const PoseidonTreeShape& s, const uint8_t* leaves, const uint64_t* indices, const uint8_t* siblings, size_t n,
                     const uint8_t** d_leaves, const uint64_t** d_indices, const uint8_t** d_siblings) {
    const size_t sib_bytes = siblings ? n * s.levels * 32 : 0;
    uint8_t* d_in = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", 8 * n + sib_bytes + n * s.leaf_len + 32, (void**)&d_in));
    SWM_HIP(ctx, hipMemcpyAsync(d_in, indices, 8 * n, hipMemcpyHostToDevice, ctx->stream));
    if (sib_bytes) SWM_HIP(ctx, hipMemcpyAsync(d_in + 8 * n, siblings, sib_bytes, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(d_in + 8 * n + sib_bytes, leaves, n * s.leaf_len, hipMemcpyHostToDevice, ctx->stream));
    *d_indices = reinterpret_cast<const uint64_t*>(d_in);
    *d_siblings = d_in + 8 * n;
    *d_leaves = d_in + 8 * n + sib_bytes;
    return SWM_OK;
}

static int ptw_host(swm_ctx* ctx, const swm_poseidon_tree_circuit* c, const swm_poseidon_tree* tree, const uint8_t* leaves,
                    const uint64_t* indices, const uint8_t* siblings, size_t count, uint64_t* witness, uint8_t* roots) {
    const PoseidonTreeShape& s = c->shape;
    const size_t item = s.num_witness * sizeof(Fr);
    for (const WitnessChunk ch : WitnessChunks(witness_stage_items(ctx, item), count)) {
        const size_t base = ch.base, n = ch.count;
        const uint8_t *d_leaves, *d_siblings;
        const uint64_t* d_indices;
        uint8_t* d_out = nullptr;
        SWM_TRY(ptw_stage(ctx, s, leaves + base * s.leaf_len, indices + base, siblings ? siblings + base * s.levels * 32 : nullptr, n, &d_leaves,
                          &d_indices, &d_siblings));
        SWM_TRY(scratch(ctx, "ptree.w", n * item + 32 * n, (void**)&d_out));
        SWM_TRY(ptw_run(ctx, c, tree, d_leaves, d_indices, d_siblings, n, (Fr*)d_out, s.num_witness, roots ? (uint32_t*)(d_out + n * item) : nullptr));
        SWM_HIP(ctx, hipMemcpyAsync(reinterpret_cast<uint8_t*>(witness) + base * item, d_out, n * item, hipMemcpyDeviceToHost, ctx->stream));
        if (roots) SWM_HIP(ctx, hipMemcpyAsync(roots + 32 * base, d_out + n * item, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
        SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the staging buffers are reused by the next chunk
    }
    return SWM_OK;
}

// one witness into the scratch buffer "ptree.w"
static int ptw_one(swm_ctx* ctx, const swm_poseidon_tree_circuit* c, const swm_poseidon_tree* tree, const uint8_t* leaf, uint64_t index,
                   const uint8_t* siblings, Fr** d_w) {
    const PoseidonTreeShape& s = c->shape;
    const uint8_t *d_leaves, *d_siblings;
    const uint64_t* d_indices;
    uint8_t* d_out = nullptr;
    SWM_TRY(ptw_stage(ctx, s, leaf, &index, siblings, 1, &d_leaves, &d_indices, &d_siblings));
    SWM_TRY(scratch(ctx, "ptree.w", s.num_witness * sizeof(Fr) + 32, (void**)&d_out));
    SWM_TRY(ptw_run(ctx, c, tree, d_leaves, d_indices, d_siblings, 1, (Fr*)d_out, s.num_witness, nullptr));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `index` was staged from this frame
    *d_w = (Fr*)d_out;
    return SWM_OK;
}

// public input one, root, the leaf bits; then the prover with the device witness
static int ptw_prove(swm_ctx* ctx, const swm_pk* pk, const swm_poseidon_tree_circuit* c, const uint8_t root[32], const uint8_t* leaf, Fr* d_w,
                     swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len) {
    const PoseidonTreeShape& s = c->shape;
    std::vector<Fr> inst(s.num_instance);
    inst[0] = fp_one<Fr>();
    Fr r;
    (void)ps_load_std(root, &r);  // canonical: the caller checked it
    inst[1] = fp_from_std(r);
    for (size_t i = 0; i < 8 * s.leaf_len; i++) inst[2 + i] = (leaf[i >> 3] >> (i & 7)) & 1 ? fp_one<Fr>() : fp_zero<Fr>();
    return prove_device_witness(ctx, pk, s.num_instance, s.num_witness, s.num_constraints, inst.data(), d_w, rng, flags, proof_out, cap, len);
}

}  // namespace swm

using namespace swm;

extern "C" {

int swm_poseidon_tree_circuit_create(swm_ctx* ctx, const swm_poseidon* params, size_t height, size_t leaf_len, swm_poseidon_tree_circuit** out) {
    if (!ctx || !params || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_circuit_create: bad arguments");
    PoseidonTreeShape shape;
    if (!poseidon_tree_shape(params->full_rounds, params->partial_rounds, params->alpha, height, leaf_len, &shape))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_circuit_create: height %zu, leaves of %zu bytes (%zu <= height <= %zu, 1 .. %zu bytes)",
                       height, leaf_len, (size_t)PT_MIN_HEIGHT, (size_t)PT_MAX_HEIGHT, (size_t)PT_MAX_LEAF_LEN);
    std::unique_ptr<swm_poseidon_tree_circuit> c(new swm_poseidon_tree_circuit);
    c->params = params;
    c->shape = shape;
    *out = c.release();
    return SWM_OK;
}

void swm_poseidon_tree_circuit_destroy(swm_ctx* ctx, swm_poseidon_tree_circuit* c) {
    destroy_circuit(ctx, c);
}

int swm_poseidon_tree_witness(swm_ctx* ctx, const swm_poseidon_tree_circuit* c, const uint8_t* leaves, const uint64_t* indices,
                              const uint8_t* siblings, size_t count, uint64_t* witness, uint8_t* roots) {
    if (!ctx || !c || (count && (!leaves || !indices || !siblings || !witness)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_witness: bad arguments");
    if (!count) return SWM_OK;
    if (count > 0x7FFFFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_witness: %zu paths in one call", count);
    SWM_TRY(ptw_check_paths(ctx, "poseidon_tree_witness", c->shape, indices, siblings, count));
    SWM_ON_DEVICE(ctx);
    return drained(ctx, ptw_host(ctx, c, nullptr, leaves, indices, siblings, count, witness, roots));
}

int swm_poseidon_tree_witness_at(swm_ctx* ctx, const swm_poseidon_tree_circuit* c, const swm_poseidon_tree* tree, const uint8_t* leaves,
                                 const uint64_t* indices, size_t count, uint64_t* witness) {
    if (!ctx || !c || !tree || (count && (!leaves || !indices || !witness)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_witness_at: bad arguments");
    SWM_TRY(ptw_check_tree(ctx, "poseidon_tree_witness_at", c, tree));
    if (!count) return SWM_OK;
    if (count > 0x7FFFFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_witness_at: %zu paths in one call", count);
    SWM_TRY(ptw_check_paths(ctx, "poseidon_tree_witness_at", c->shape, indices, nullptr, count));
    SWM_ON_DEVICE(ctx);
    return drained(ctx, ptw_host(ctx, c, tree, leaves, indices, nullptr, count, witness, nullptr));
}

int swm_poseidon_tree_prove(swm_ctx* ctx, const swm_pk* pk, const swm_poseidon_tree_circuit* c, const uint8_t root[32], const uint8_t* leaf,
                            uint64_t index, const uint8_t* siblings, swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len) {
    if (!ctx || !pk || !c || !root || !leaf || !siblings || !rng || !proof_out || !len)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_prove: bad arguments");
    Fr r;
    if (!ps_load_std(root, &r)) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_prove: the root is not a canonical field element");
    SWM_TRY(ptw_check_paths(ctx, "poseidon_tree_prove", c->shape, &index, siblings, 1));
    Fr* d_w = nullptr;
    {
        SWM_ON_DEVICE(ctx);
        SWM_TRY(drained(ctx, ptw_one(ctx, c, nullptr, leaf, index, siblings, &d_w)));
    }
    return ptw_prove(ctx, pk, c, root, leaf, d_w, rng, flags, proof_out, cap, len);
}

int swm_poseidon_tree_prove_at(swm_ctx* ctx, const swm_pk* pk, const swm_poseidon_tree_circuit* c, const swm_poseidon_tree* tree,
                               const uint8_t* leaf, uint64_t index, swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len) {
    if (!ctx || !pk || !c || !tree || !leaf || !rng || !proof_out || !len)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_prove_at: bad arguments");
    SWM_TRY(ptw_check_tree(ctx, "poseidon_tree_prove_at", c, tree));
    SWM_TRY(ptw_check_paths(ctx, "poseidon_tree_prove_at", c->shape, &index, nullptr, 1));
    Fr* d_w = nullptr;
    uint8_t root[32];
    {
        SWM_ON_DEVICE(ctx);
        SWM_TRY(drained(ctx, ptw_one(ctx, c, tree, leaf, index, nullptr, &d_w)));
        SWM_HIP(ctx, hipMemcpyAsync(root, tree->d_nodes + 32 * (tree->num_nodes() - 1), 32, hipMemcpyDeviceToHost, ctx->stream));
        SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ptw_prove(ctx, pk, c, root, leaf, d_w, rng, flags, proof_out, cap, len);
}

}  // extern "C"

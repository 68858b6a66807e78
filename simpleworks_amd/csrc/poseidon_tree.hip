// poseidon_tree.hip — a Poseidon Merkle tree that STAYS on the GPU: blank, built from leaves, updated in batches, read as paths;
// and the path check that needs no tree.  The Poseidon counterpart of merkle_tree.hip, with this library's own definition of the
// tree (the reference builds no Poseidon tree): the leaf digest is the byte sponge of poseidon.hip (the reference's
// poseidon2_hash), an inner node the two-to-one form H2(a, b) = permutation of (a, b, 0), entry 0.
//
// Layout: merkle_tree.hip's — n = 2^L leaf digests | n / 2 | ... | root, 32 canonical little-endian bytes each;
// host/merkle_dirty.h and its offsets serve unchanged.
// One lane per hash, one wave per workgroup, the parameter table in LDS: the structure of poseidon_hash_kernel.  The two hashes
// and their bounds: poseidon_tree.h (every tree input enters as an absorbed element, so the bounds at the head of poseidon.hip hold
// as they stand).
// Update.  host/merkle_dirty.h turns the batch's indices into the last-writer leaf jobs and the sorted unique parents of every
// level.  The leaf jobs are one launch.  A level with more than PT_TAIL dirty nodes is one launch behind its index list.  From the
// first level with at most PT_TAIL dirty nodes ONE WAVE finishes the tree in one launch: lane j starts with dirty node j of that
// level and its digest in registers.  Going up, the lane that holds the first dirty child of a parent computes the parent; the
// other child comes from the next live lane by shuffles when it is dirty too (the list is sorted, so that lane is the next one
// still live) and from memory when it is not.  The lists are not compacted: a lane whose node was the second child goes idle.
// An update of up to PT_TAIL leaves is therefore two launches whatever the height.  Stream order between launches is the only
// cross-workgroup ordering: no cooperative launch, no grid barrier, no flag, no atomic.
// Path check.  One lane per path (pt_walk); nothing goes through memory between levels.
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "context.h"
#include "host/merkle_dirty.h"
#include "merkle_nodes.cuh"
#include "poseidon_tree.h"
#include "swmarlin.h"
#include "witness_host.h"

namespace swm {

static constexpr unsigned PT_TAIL = 64;  // dirty nodes of a level the finishing wave takes: one lane each

// Job j hashes leaf src[j] of `leaves` into leaf digest dst[j]; without lists job j is leaf j.
__global__ void __launch_bounds__(PS_LANES) poseidon_tree_leaves_kernel(const uint4* __restrict__ table, PtParams P,
                                                                        const uint8_t* __restrict__ leaves, size_t leaf_len, size_t count,
                                                                        const uint32_t* __restrict__ dst, const uint32_t* __restrict__ src,
                                                                        uint32_t* __restrict__ nodes) {
    SWM_LIGHT_KERNEL();
    extern __shared__ __align__(16) uint32_t ps_tab[];
    pt_load_table(ps_tab, table, P.rows);
    const size_t j = blockIdx.x * (size_t)PS_LANES + threadIdx.x;
    if (j >= count) return;
    const Fr x = pt_hash_leaf(ps_tab, P, leaves, src ? src[j] : j, leaf_len);
    pt_store(nodes + 8 * (dst ? (size_t)dst[j] : j), x);
}

// Job j computes parent list[j] (without a list: parent j) of the level `out` from its two children in the level `in`.
__global__ void __launch_bounds__(PS_LANES) poseidon_tree_level_kernel(const uint4* __restrict__ table, PtParams P,
                                                                       const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t count,
                                                                       const uint32_t* __restrict__ list) {
    SWM_LIGHT_KERNEL();
    extern __shared__ __align__(16) uint32_t ps_tab[];
    pt_load_table(ps_tab, table, P.rows);
    const size_t j = blockIdx.x * (size_t)PS_LANES + threadIdx.x;
    if (j >= count) return;
    const size_t p = list ? (size_t)list[j] : j;
    const Fr x = pt_hash2(ps_tab, P, pt_load(in + 16 * p), pt_load(in + 16 * p + 8));
    pt_store(out + 8 * p, x);
}

// One wave: levels first .. levels - 1.  Lane j < count starts with node list[j] (without a list: node j) of level `first`, whose
// digest the launch before this one stored.  Every lane runs every permutation; only the stores and the choice of operands depend
// on `live`.
__global__ void __launch_bounds__(PS_LANES) poseidon_tree_tail_kernel(const uint4* __restrict__ table, PtParams P, uint32_t* __restrict__ nodes,
                                                                      unsigned levels, unsigned first, unsigned count,
                                                                      const uint32_t* __restrict__ list) {
    SWM_LIGHT_KERNEL();
    extern __shared__ __align__(16) uint32_t ps_tab[];
    pt_load_table(ps_tab, table, P.rows);
    const unsigned lane = threadIdx.x;
    bool live = lane < count;
    uint32_t node = live ? (list ? list[lane] : lane) : 0u;
    Fr cur = fp_zero<Fr>();
    if (live) cur = pt_load(nodes + 8 * (mt_level_offset(levels, first) + node));
#pragma unroll 1
    for (unsigned l = first; l < levels; l++) {
        const unsigned long long mask = __ballot(live);
        const unsigned long long above = lane < 63 ? mask & ~(((unsigned long long)2 << lane) - 1) : 0ull;  // live lanes after this one
        const int next = above ? __ffsll((long long)above) - 1 : (int)lane;
        const unsigned long long below = mask & (((unsigned long long)1 << lane) - 1);
        const int prev = below ? 63 - __clzll((long long)below) : (int)lane;
        const uint32_t next_node = (uint32_t)__shfl((int)node, next, 64), prev_node = (uint32_t)__shfl((int)node, prev, 64);
        Fr other;
#pragma unroll
        for (int w = 0; w < 8; w++) other.v[w] = (uint32_t)__shfl((int)cur.v[w], next, 64);
        // the second dirty child of a parent: the lane before it computes the parent
        const bool second = live && below && (node & 1u) && prev_node == (node ^ 1u);
        const bool pair = live && above && !(node & 1u) && next_node == (node ^ 1u);  // the sibling is dirty: it is in `other`
        live = live && !second;
        if (live && !pair) other = pt_load(nodes + 8 * (mt_level_offset(levels, l) + (node ^ 1u)));
        const bool right = node & 1u;  // this lane's digest is the right child
        cur = pt_hash2(ps_tab, P, right ? other : cur, right ? cur : other);
        node >>= 1;
        if (live) pt_store(nodes + 8 * (mt_level_offset(levels, l + 1) + node), cur);
    }
}

// chain[0] = 32 zero bytes, chain[l + 1] = H2(chain[l], chain[l]).  One lane.
__global__ void __launch_bounds__(PS_LANES) poseidon_tree_blank_chain_kernel(const uint4* __restrict__ table, PtParams P, unsigned levels,
                                                                             uint32_t* __restrict__ chain) {
    extern __shared__ __align__(16) uint32_t ps_tab[];
    pt_load_table(ps_tab, table, P.rows);
    if (threadIdx.x) return;
    Fr cur = fp_zero<Fr>();
    pt_store(chain, cur);
#pragma unroll 1
    for (unsigned l = 0; l < levels; l++) {
        cur = pt_hash2(ps_tab, P, cur, cur);
        pt_store(chain + 8 * (l + 1), cur);
    }
}

// Path::verify for `count` paths, one lane each.
__global__ void __launch_bounds__(PS_LANES) poseidon_verify_paths_kernel(const uint4* __restrict__ table, PtParams P, unsigned levels,
                                                                         const uint8_t* __restrict__ roots, size_t root_stride,
                                                                         const uint8_t* __restrict__ leaves, size_t leaf_len,
                                                                         const uint64_t* __restrict__ indices, const uint8_t* __restrict__ siblings,
                                                                         size_t count, uint8_t* __restrict__ ok, uint32_t* __restrict__ status) {
    SWM_LIGHT_KERNEL();
    extern __shared__ __align__(16) uint32_t ps_tab[];
    pt_load_table(ps_tab, table, P.rows);
    const size_t p = blockIdx.x * (size_t)PS_LANES + threadIdx.x;
    if (p >= count) return;
    const uint64_t index = indices[p];
    unsigned bad = (index >> levels) ? 2u : 0u;
    const Fr top = pt_walk(ps_tab, P, leaves, p, leaf_len, index, reinterpret_cast<const uint32_t*>(siblings + p * (size_t)levels * 32), levels,
                           nullptr, bad);
    const Fr root = pt_load(reinterpret_cast<const uint32_t*>(roots + p * root_stride));
    if (!pt_canonical(root)) bad |= 1u;
    bool same = true;
#pragma unroll
    for (int w = 0; w < 8; w++) same = same && root.v[w] == top.v[w];
    ok[p] = !bad && same ? 1 : 0;
    if (status) status[p] = (bad & 1u) ? 1u : bad ? 2u : 0u;
}

static uint32_t* pt_level(const swm_poseidon_tree* t, size_t l) {
    return reinterpret_cast<uint32_t*>(t->d_nodes + 32 * merkle_level_offset(t->levels(), l));
}

static int pt_check_params(swm_ctx* ctx, const char* what, size_t height, size_t leaf_len) {
    if (!merkle_height_ok(height))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: height %zu (%zu <= height <= %zu)", what, height, (size_t)MT_MIN_HEIGHT, (size_t)MT_MAX_HEIGHT);
    if (!leaf_len || leaf_len > PS_MAX_BYTES)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: leaves of %zu bytes (1 .. %zu)", what, leaf_len, PS_MAX_BYTES);
    return SWM_OK;
}

static int pt_alloc(swm_ctx* ctx, const char* what, const swm_poseidon* params, size_t height, size_t leaf_len,
                    std::unique_ptr<swm_poseidon_tree>* out) {
    std::unique_ptr<swm_poseidon_tree> t(new swm_poseidon_tree);
    t->params = params;
    t->height = height;
    t->leaf_len = leaf_len;
    hipError_t e = hipMalloc((void**)&t->d_nodes, t->num_nodes() * 32);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(ctx, e == hipErrorOutOfMemory ? SWM_ERR_OOM : SWM_ERR_HIP, "%s: %zu nodes: %s", what, t->num_nodes(), hipGetErrorString(e));
    }
    *out = std::move(t);
    return SWM_OK;
}

static void pt_release(swm_ctx* ctx, std::unique_ptr<swm_poseidon_tree>& t) {  // a create that failed after its allocation
    drain_streams(ctx);
    (void)hipFree(t->d_nodes);
    t.reset();
}

static int pt_blank_run(swm_ctx* ctx, swm_poseidon_tree* t) {
    const unsigned levels = (unsigned)t->levels();
    uint32_t* d_chain = nullptr;
    SWM_TRY(scratch(ctx, "merkle.chain", MT_MAX_HEIGHT * 32, (void**)&d_chain));
    SWM_LAUNCH(ctx, "poseidon_tree_blank_chain", poseidon_tree_blank_chain_kernel, dim3(1), dim3(PS_LANES), pt_lds(t->params),
               pt_table(t->params), pt_params(t->params), levels, d_chain);
    const size_t halves = 2 * t->num_nodes();
    const unsigned blocks = (unsigned)std::min<size_t>((halves + 255) / 256, 1u << 16);
    SWM_LAUNCH(ctx, "merkle_blank_fill", merkle_blank_fill_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<const uint4*>(d_chain), levels,
               reinterpret_cast<uint4*>(t->d_nodes));
    return SWM_OK;
}

// The wave that finishes the tree from level `first`, whose `count` <= PT_TAIL dirty nodes are d_list (NULL: nodes 0 .. count - 1).
static int pt_tail_run(swm_ctx* ctx, swm_poseidon_tree* t, unsigned first, size_t count, const uint32_t* d_list) {
    const unsigned levels = (unsigned)t->levels();
    if (first >= levels) return SWM_OK;
    SWM_LAUNCH(ctx, "poseidon_tree_tail", poseidon_tree_tail_kernel, dim3(1), dim3(PS_LANES), pt_lds(t->params), pt_table(t->params),
               pt_params(t->params), reinterpret_cast<uint32_t*>(t->d_nodes), levels, first, (unsigned)count, d_list);
    return SWM_OK;
}

// every node from the n leaves at d_leaves
static int pt_build_run(swm_ctx* ctx, swm_poseidon_tree* t, const uint8_t* d_leaves) {
    const swm_poseidon* p = t->params;
    const size_t n = t->n(), levels = t->levels();
    SWM_LAUNCH(ctx, "poseidon_tree_leaves", poseidon_tree_leaves_kernel, dim3(pt_blocks(n)), dim3(PS_LANES), pt_lds(p), pt_table(p), pt_params(p),
               d_leaves, t->leaf_len, n, (const uint32_t*)nullptr, (const uint32_t*)nullptr, pt_level(t, 0));
    size_t l = 0;
    for (; l < levels && (n >> l) > PT_TAIL; l++)
        SWM_LAUNCH(ctx, "poseidon_tree_level", poseidon_tree_level_kernel, dim3(pt_blocks(n >> (l + 1))), dim3(PS_LANES), pt_lds(p), pt_table(p),
                   pt_params(p), pt_level(t, l), pt_level(t, l + 1), n >> (l + 1), (const uint32_t*)nullptr);
    return pt_tail_run(ctx, t, (unsigned)l, n >> l, nullptr);
}

// The launches of one batch.  `d` is the batch's dirty set, d_leaves the batch's leaf bytes on the device.  The index lists go up
// from `words` (host memory of this call): the caller waits before `words` goes out of scope.
static int pt_update_run(swm_ctx* ctx, swm_poseidon_tree* t, const MerkleDirty& d, const uint8_t* d_leaves, std::vector<uint32_t>* words) {
    const size_t jobs = d.leaves.size();
    if (!jobs) return SWM_OK;
    const swm_poseidon* p = t->params;
    const size_t levels = t->levels();
    auto dirty = [&](size_t l) { return l == 0 ? jobs : d.parents[l - 1].size(); };  // dirty nodes of level l
    // leaf jobs (dst | src), the parents of every level that gets a launch of its own, the finishing wave's nodes
    words->resize(2 * jobs);
    for (size_t j = 0; j < jobs; j++) {
        (*words)[j] = d.leaves[j].index;
        (*words)[jobs + j] = d.leaves[j].src;
    }
    std::vector<size_t> at(levels + 1, 0);
    size_t first = 0;
    for (; first < levels && dirty(first) > PT_TAIL; first++) {
        at[first] = words->size();
        words->insert(words->end(), d.parents[first].begin(), d.parents[first].end());
    }
    size_t tail_at = 0;  // the dirty nodes of level `first`
    if (first == 0) tail_at = 0;
    else tail_at = at[first - 1];
    uint32_t* d_words = nullptr;
    SWM_TRY(scratch(ctx, "merkle.jobs", words->size() * 4, (void**)&d_words));
    SWM_HIP(ctx, hipMemcpyAsync(d_words, words->data(), words->size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SWM_LAUNCH(ctx, "poseidon_tree_update_leaves", poseidon_tree_leaves_kernel, dim3(pt_blocks(jobs)), dim3(PS_LANES), pt_lds(p), pt_table(p),
               pt_params(p), d_leaves, t->leaf_len, jobs, (const uint32_t*)d_words, (const uint32_t*)(d_words + jobs), pt_level(t, 0));
    for (size_t l = 0; l < first; l++) {
        const size_t cnt = d.parents[l].size();
        SWM_LAUNCH(ctx, "poseidon_tree_update_level", poseidon_tree_level_kernel, dim3(pt_blocks(cnt)), dim3(PS_LANES), pt_lds(p), pt_table(p),
                   pt_params(p), pt_level(t, l), pt_level(t, l + 1), cnt, (const uint32_t*)(d_words + at[l]));
    }
    return pt_tail_run(ctx, t, (unsigned)first, dirty(first), d_words + tail_at);
}

static int pt_update_args(swm_ctx* ctx, const swm_poseidon_tree* t, const uint64_t* indices, const void* leaves, size_t leaf_len, size_t count,
                          MerkleDirty* d) {
    if (!ctx || !t || (count && (!indices || !leaves))) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_update: bad arguments");
    if (leaf_len != t->leaf_len)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_update: leaves of %zu bytes in a tree of %zu-byte leaves", leaf_len, t->leaf_len);
    size_t bad_at = 0;
    switch (merkle_dirty(t->height, indices, count, d, &bad_at)) {
        case MT_DIRTY_OK: return SWM_OK;
        case MT_DIRTY_BAD_INDEX:
            return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_update: update %zu: leaf index %llu in a tree of %zu leaves", bad_at,
                           (unsigned long long)indices[bad_at], t->n());
        default: return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_update: %zu updates in one call", count);
    }
}

static int pt_paths_host(swm_ctx* ctx, const swm_poseidon_tree* t, const uint64_t* indices, size_t count, uint8_t* siblings) {
    const size_t bytes = count * t->levels() * 32, words = bytes / 4;
    uint8_t *d_in = nullptr, *d_out = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", 8 * count, (void**)&d_in));
    SWM_TRY(scratch(ctx, "stage.b", bytes, (void**)&d_out));
    SWM_HIP(ctx, hipMemcpyAsync(d_in, indices, 8 * count, hipMemcpyHostToDevice, ctx->stream));
    const unsigned blocks = (unsigned)std::min<size_t>((words + 255) / 256, 1u << 16);
    SWM_LAUNCH(ctx, "merkle_paths", merkle_paths_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<const uint32_t*>(t->d_nodes),
               (unsigned)t->levels(), reinterpret_cast<const uint64_t*>(d_in), count, reinterpret_cast<uint32_t*>(d_out));
    SWM_HIP(ctx, hipMemcpyAsync(siblings, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWM_OK;
}

static int pt_verify_host(swm_ctx* ctx, const swm_poseidon* p, size_t height, const uint8_t* roots, size_t root_stride, const uint8_t* leaves,
                          size_t leaf_len, const uint64_t* indices, const uint8_t* siblings, size_t count, uint8_t* ok, uint32_t* status) {
    // indices | siblings | roots | leaves in one staging buffer; status | ok in the other
    const size_t sib_bytes = count * (height - 1) * 32, root_bytes = root_stride ? 32 * count : 32;
    uint8_t *d_in = nullptr, *d_out = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", 8 * count + sib_bytes + root_bytes + count * leaf_len + 32, (void**)&d_in));
    SWM_TRY(scratch(ctx, "stage.b", 5 * count, (void**)&d_out));
    uint8_t *d_sib = d_in + 8 * count, *d_roots = d_sib + sib_bytes, *d_leaves = d_roots + root_bytes;
    SWM_HIP(ctx, hipMemcpyAsync(d_in, indices, 8 * count, hipMemcpyHostToDevice, ctx->stream));
    if (sib_bytes) SWM_HIP(ctx, hipMemcpyAsync(d_sib, siblings, sib_bytes, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(d_roots, roots, root_bytes, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(d_leaves, leaves, count * leaf_len, hipMemcpyHostToDevice, ctx->stream));
    SWM_LAUNCH(ctx, "poseidon_verify_paths", poseidon_verify_paths_kernel, dim3(pt_blocks(count)), dim3(PS_LANES), pt_lds(p), pt_table(p),
               pt_params(p), (unsigned)(height - 1), (const uint8_t*)d_roots, root_stride, (const uint8_t*)d_leaves, leaf_len,
               reinterpret_cast<const uint64_t*>(d_in), (const uint8_t*)d_sib, count, d_out + 4 * count, reinterpret_cast<uint32_t*>(d_out));
    SWM_HIP(ctx, hipMemcpyAsync(ok, d_out + 4 * count, count, hipMemcpyDeviceToHost, ctx->stream));
    if (status) SWM_HIP(ctx, hipMemcpyAsync(status, d_out, 4 * count, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWM_OK;
}

}  // namespace swm

using namespace swm;

extern "C" {

int swm_poseidon_tree_create_blank(swm_ctx* ctx, const swm_poseidon* params, size_t height, size_t leaf_len, swm_poseidon_tree** out) {
    if (!ctx || !params || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_create_blank: bad arguments");
    SWM_TRY(pt_check_params(ctx, "poseidon_tree_create_blank", height, leaf_len));
    SWM_ON_DEVICE(ctx);
    std::unique_ptr<swm_poseidon_tree> t;
    SWM_TRY(pt_alloc(ctx, "poseidon_tree_create_blank", params, height, leaf_len, &t));
    const int rc = pt_blank_run(ctx, t.get());
    if (rc != SWM_OK) {
        pt_release(ctx, t);
        return rc;
    }
    *out = t.release();
    return SWM_OK;
}

int swm_poseidon_tree_create_from_leaves(swm_ctx* ctx, const swm_poseidon* params, const uint8_t* leaves, size_t leaf_len, size_t n_leaves,
                                         swm_poseidon_tree** out) {
    if (!ctx || !params || !leaves || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_create_from_leaves: bad arguments");
    if (n_leaves < 2 || (n_leaves & (n_leaves - 1)) || n_leaves > ((size_t)1 << (MT_MAX_HEIGHT - 1)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_create_from_leaves: %zu leaves (a power of two, 2 .. 2^%zu)", n_leaves,
                       (size_t)MT_MAX_HEIGHT - 1);
    size_t height = 1;
    while (((size_t)1 << (height - 1)) < n_leaves) height++;
    SWM_TRY(pt_check_params(ctx, "poseidon_tree_create_from_leaves", height, leaf_len));
    SWM_ON_DEVICE(ctx);
    uint8_t* d_in = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", n_leaves * leaf_len + 32, (void**)&d_in));
    std::unique_ptr<swm_poseidon_tree> t;
    SWM_TRY(pt_alloc(ctx, "poseidon_tree_create_from_leaves", params, height, leaf_len, &t));
    int rc = SWM_OK;
    hipError_t e = hipMemcpyAsync(d_in, leaves, n_leaves * leaf_len, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) rc = pt_build_run(ctx, t.get(), d_in);
    if (e == hipSuccess && rc == SWM_OK) e = hipStreamSynchronize(ctx->stream);  // `leaves` is the caller's
    if (e != hipSuccess || rc != SWM_OK) {
        pt_release(ctx, t);
        return rc != SWM_OK ? rc : set_err(ctx, SWM_ERR_HIP, "poseidon_tree_create_from_leaves: %s", hipGetErrorString(e));
    }
    *out = t.release();
    return SWM_OK;
}

void swm_poseidon_tree_destroy(swm_ctx* ctx, swm_poseidon_tree* t) {
    if (!t) return;
    DeviceGuard guard(ctx);
    if (ctx) drain_streams(ctx);
    if (t->d_nodes) (void)hipFree(t->d_nodes);
    delete t;
}

int swm_poseidon_tree_update(swm_ctx* ctx, swm_poseidon_tree* t, const uint64_t* indices, const uint8_t* leaves, size_t leaf_len, size_t count) {
    MerkleDirty d;
    SWM_TRY(pt_update_args(ctx, t, indices, leaves, leaf_len, count, &d));
    if (!count) return SWM_OK;
    SWM_ON_DEVICE(ctx);
    uint8_t* d_in = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", count * leaf_len + 32, (void**)&d_in));
    SWM_HIP(ctx, hipMemcpyAsync(d_in, leaves, count * leaf_len, hipMemcpyHostToDevice, ctx->stream));
    std::vector<uint32_t> words;
    const int rc = pt_update_run(ctx, t, d, d_in, &words);
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `leaves` is the caller's, `words` goes out of scope
    return rc;
}

int swm_poseidon_tree_root(swm_ctx* ctx, const swm_poseidon_tree* t, uint8_t root[32]) {
    if (!ctx || !t || !root) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_root: bad arguments");
    SWM_ON_DEVICE(ctx);
    SWM_HIP(ctx, hipMemcpyAsync(root, t->d_nodes + 32 * (t->num_nodes() - 1), 32, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWM_OK;
}

int swm_poseidon_tree_nodes(swm_ctx* ctx, const swm_poseidon_tree* t, uint8_t* nodes) {
    if (!ctx || !t || !nodes) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_nodes: bad arguments");
    SWM_ON_DEVICE(ctx);
    SWM_HIP(ctx, hipMemcpyAsync(nodes, t->d_nodes, t->num_nodes() * 32, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWM_OK;
}

int swm_poseidon_tree_dev_nodes(const swm_poseidon_tree* t, void** d_nodes, size_t* n_nodes) {
    if (!t || !d_nodes || !n_nodes) return set_err(nullptr, SWM_ERR_INVALID_ARG, "poseidon_tree_dev_nodes: bad arguments");
    *d_nodes = t->d_nodes;
    *n_nodes = t->num_nodes();
    return SWM_OK;
}

int swm_poseidon_tree_paths(swm_ctx* ctx, const swm_poseidon_tree* t, const uint64_t* indices, size_t count, uint8_t* siblings) {
    if (!ctx || !t || (count && (!indices || !siblings))) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_paths: bad arguments");
    for (size_t p = 0; p < count; p++)
        if (indices[p] >= t->n())
            return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_tree_paths: path %zu: leaf index %llu in a tree of %zu leaves", p,
                           (unsigned long long)indices[p], t->n());
    if (!count) return SWM_OK;
    SWM_ON_DEVICE(ctx);
    return drained(ctx, pt_paths_host(ctx, t, indices, count, siblings));
}

int swm_poseidon_verify_paths(swm_ctx* ctx, const swm_poseidon* params, size_t height, const uint8_t* roots, size_t root_stride,
                              const uint8_t* leaves, size_t leaf_len, const uint64_t* indices, const uint8_t* siblings, size_t count,
                              uint8_t* ok, uint32_t* status) {
    if (!ctx || !params || (count && (!roots || !leaves || !indices || !siblings || !ok)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_verify_paths: bad arguments");
    if (root_stride != 0 && root_stride != 32)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_verify_paths: a root stride of %zu (0: one root for all paths, 32: one per path)",
                       root_stride);
    if (count > 0x7FFFFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_verify_paths: %zu paths in one call", count);
    SWM_TRY(pt_check_params(ctx, "poseidon_verify_paths", height, leaf_len));
    if (!count) return SWM_OK;
    SWM_ON_DEVICE(ctx);
    return drained(ctx, pt_verify_host(ctx, params, height, roots, root_stride, leaves, leaf_len, indices, siblings, count, ok, status));
}

}  // extern "C"

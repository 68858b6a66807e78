// merkle_tree.hip — a Pedersen Merkle tree that STAYS on the GPU: blank, built from leaves, updated in batches, read as paths;
// and the path check that needs no tree.  What the ledger of examples/simple-payments does to its account tree:
//   examples/simple-payments/ledger.rs:106-112       MerkleTree::blank(&leaf_crh_params, &two_to_one_crh_params, height)
//   examples/simple-payments/ledger.rs:140-142, 170  tree.update(id, &account_info.to_bytes_le())
//   examples/simple-payments/transaction.rs:163-173  tree.generate_proof(sender), path.verify(.., &root, &leaf)
// swm_merkle_tree_build (pedersen.hip) is one-shot: all leaves in, all nodes out, nothing kept.  One changed balance is `height`
// dependent hashes; this unit does those and no more.
//
// Layout: pedersen.hip's — n = 2^L leaf digests | n / 2 | ... | root, 32 canonical little-endian bytes each, so the children
// 2 p and 2 p + 1 of a parent are 64 adjacent bytes: the two-to-one hash's input as it stands.
// Update.  host/merkle_dirty.h turns the batch's indices into the last-writer leaf jobs and the sorted unique parents of every
// level.  A level with more than MT_TAIL dirty nodes is the hash of pedersen.cuh behind that index list, one launch, lanes per
// hash by lanes_for.  The dirty count never grows going up: from the first level with at most MT_TAIL dirty nodes one workgroup
// (one wave per node) finishes the tree in a single launch, handing each fresh digest to the next level through LDS (and storing
// it) and reading only untouched siblings from memory.  Stream order between launches is the only cross-workgroup ordering: no
// cooperative launch, no grid barrier, no flag, no atomic.  Lists of at most MT_TAIL entries travel as kernel arguments, so the
// ledger's one or two updates upload nothing and take two launches whatever the height.
// Path check.  One group of lanes_for(count) lanes per path; the running digest lives in registers and moves by shuffles: the
// group's lane 0 normalises the sum, broadcasts the eight words, and every lane picks its windows' bits from (digest, sibling)
// held in registers.  Nothing goes through memory between levels.
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "context.h"
#include "host/merkle_dirty.h"
#include "merkle_nodes.cuh"
#include "merkle_tree.h"
#include "pedersen.cuh"
#include "pedersen.h"
#include "swmarlin.h"

namespace swm {

static constexpr unsigned MT_TAIL = 4;         // dirty nodes per level the finishing workgroup takes: one wave each
static constexpr unsigned MT_MAX_LEVELS = 30;  // MT_MAX_HEIGHT - 1

struct MtSmall {  // a job list short enough to be a kernel argument
    uint32_t dst[MT_TAIL], src[MT_TAIL];
};
struct MtTail {
    uint32_t levels, first;                // two-to-one levels of the tree; the first one this launch computes
    uint32_t count[MT_MAX_LEVELS];         // [l]: dirty nodes of level l + 1 (<= MT_TAIL for l >= first)
    uint32_t node[MT_MAX_LEVELS][MT_TAIL];
};

// Job j hashes the `len` bytes at in + src[j] * stride into the digest out + 32 dst[j].  Leaves: src = position in the batch,
// dst = leaf index.  A two-to-one level: src = dst = parent, in = the level below (stride 64), out = the parent's level.
__global__ void __launch_bounds__(256) merkle_hash_indexed_kernel(const EdRow* __restrict__ table, unsigned num_windows, unsigned ws,
                                                                  const uint8_t* __restrict__ in, size_t stride, size_t len, size_t count,
                                                                  unsigned lanes, Fr k2d, uint8_t* __restrict__ out,
                                                                  const uint32_t* __restrict__ dst, const uint32_t* __restrict__ src,
                                                                  MtSmall small) {
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t h = gid / lanes;
    const unsigned lane = (unsigned)(gid % lanes);
    const bool live = h < count;
    EdExt acc = ed_identity();
    size_t to = 0;
    if (live) {
        to = dst ? dst[h] : small.dst[h];  // (no list: count <= MT_TAIL)
        const uint8_t* msg = in + (size_t)(src ? src[h] : small.src[h]) * stride;
        acc = ped_partial(table, num_windows, ws, [msg](size_t i) { return (unsigned)msg[i]; }, len, lanes, lane);
    }
    acc = ped_join(acc, lanes, k2d);
    if (live && lane == 0) {
        const Fr x = ped_digest(acc);
        uint32_t* o = reinterpret_cast<uint32_t*>(out + 32 * to);
#pragma unroll
        for (int i = 0; i < 8; i++) o[i] = x.v[i];
    }
}

// One workgroup, wave w = dirty node w of the level: levels t.first .. t.levels - 1, a barrier between them.
__global__ void __launch_bounds__(64 * MT_TAIL) merkle_tail_kernel(const EdRow* __restrict__ table, unsigned num_windows, unsigned ws,
                                                                   uint8_t* __restrict__ nodes, MtTail t, Fr k2d) {
    __shared__ uint32_t msg[MT_TAIL][16];       // left || right of each wave's hash
    __shared__ uint32_t fresh[2][MT_TAIL][8];   // the digests of the level before (by parity of the level)
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (unsigned l = t.first; l < t.levels; l++) {
        const bool live = wave < t.count[l];
        const unsigned parent = live ? t.node[l][wave] : 0;
        if (live && lane < 16) {
            const unsigned child = 2 * parent + (lane >> 3), word = lane & 7;
            int from = -1;  // computed by this launch one level down?
            if (l > t.first)
                for (unsigned j = 0; j < t.count[l - 1]; j++)
                    if (t.node[l - 1][j] == child) from = (int)j;
            msg[wave][lane] = from >= 0 ? fresh[(l - 1) & 1][from][word]
                                        : reinterpret_cast<const uint32_t*>(nodes + 32 * (mt_level_offset(t.levels, l) + child))[word];
        }
        __syncthreads();
        EdExt acc = ed_identity();
        if (live) {
            const uint32_t* m = msg[wave];
            acc = ped_partial(table, num_windows, ws, [m](size_t i) { return (m[i >> 2] >> (8 * (i & 3))) & 0xFFu; }, 64, 64, lane);
        }
        acc = ped_join(acc, 64, k2d);
        if (live && lane == 0) {
            const Fr x = ped_digest(acc);
            uint32_t* o = reinterpret_cast<uint32_t*>(nodes + 32 * (mt_level_offset(t.levels, l + 1) + parent));
#pragma unroll
            for (int i = 0; i < 8; i++) {
                fresh[l & 1][wave][i] = x.v[i];
                o[i] = x.v[i];
            }
        }
        __syncthreads();
    }
}

// MerkleTree::blank: chain[0] = 32 zero bytes, chain[l + 1] = H(chain[l] || chain[l]).  One wave.
__global__ void __launch_bounds__(64) merkle_blank_chain_kernel(const EdRow* __restrict__ table, unsigned num_windows, unsigned ws,
                                                                unsigned levels, uint32_t* __restrict__ chain, Fr k2d) {
    __shared__ uint32_t msg[16];
    const unsigned lane = threadIdx.x;
    if (lane < 16) msg[lane] = 0;
    if (lane < 8) chain[lane] = 0;
    __syncthreads();
    for (unsigned l = 0; l < levels; l++) {
        const uint32_t* m = msg;
        EdExt acc = ped_partial(table, num_windows, ws, [m](size_t i) { return (m[i >> 2] >> (8 * (i & 3))) & 0xFFu; }, 64, 64, lane);
        acc = ped_join(acc, 64, k2d);
        __syncthreads();  // every lane has read msg
        if (lane == 0) {
            const Fr x = ped_digest(acc);
#pragma unroll
            for (int i = 0; i < 8; i++) msg[i] = msg[8 + i] = chain[8 * (l + 1) + i] = x.v[i];
        }
        __syncthreads();
    }
}

__device__ __forceinline__ bool mt_canonical(const uint32_t* v) {
    Fr s, r;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        s.v[i] = v[i];
        r.v[i] = FrParams::P[i];
    }
    return fp_cmp_std(s, r) < 0;
}

// Path::verify for `count` paths, `lanes` lanes each.
__global__ void __launch_bounds__(256) merkle_verify_paths_kernel(const EdRow* __restrict__ leaf_table, unsigned leaf_windows, unsigned leaf_ws,
                                                                  const EdRow* __restrict__ inner_table, unsigned inner_windows, unsigned inner_ws,
                                                                  unsigned levels, const uint8_t* __restrict__ roots, size_t root_stride,
                                                                  const uint8_t* __restrict__ leaves, size_t leaf_len,
                                                                  const uint64_t* __restrict__ indices, const uint8_t* __restrict__ siblings,
                                                                  size_t count, unsigned lanes, Fr k2d, uint8_t* __restrict__ ok,
                                                                  uint32_t* __restrict__ status) {
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t p = gid / lanes;
    const unsigned lane = (unsigned)(gid % lanes);
    const int head = (int)((threadIdx.x & 63u) & ~(lanes - 1u));  // the group's lane 0 within the wave
    const bool live = p < count;
    const uint64_t index = live ? indices[p] : 0;
    unsigned bad = (index >> levels) ? 2u : 0u;
    const uint32_t* sib = reinterpret_cast<const uint32_t*>(siblings + (live ? p : 0) * (size_t)levels * 32);

    EdExt acc = ed_identity();
    if (live) {
        const uint8_t* msg = leaves + p * leaf_len;
        acc = ped_partial(leaf_table, leaf_windows, leaf_ws, [msg](size_t i) { return (unsigned)msg[i]; }, leaf_len, lanes, lane);
    }
    uint32_t cur[8];
#pragma unroll 1
    for (unsigned l = 0;; l++) {
        acc = ped_join(acc, lanes, k2d);
        Fr x = fp_zero<Fr>();
        if (lane == 0) x = ped_digest(acc);
#pragma unroll
        for (int i = 0; i < 8; i++) cur[i] = (uint32_t)__shfl((int)x.v[i], head, 64);
        if (l == levels) break;
        uint32_t s[8];
#pragma unroll
        for (int i = 0; i < 8; i++) s[i] = live ? sib[8 * l + i] : 0u;
        if (!mt_canonical(s)) bad |= 1u;
        const bool right = (index >> l) & 1u;  // the running digest is the right child
        MtMsg64 m;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            m.w[i] = right ? s[i] : cur[i];
            m.w[8 + i] = right ? cur[i] : s[i];
        }
        acc = ped_partial(inner_table, inner_windows, inner_ws, m, 64, lanes, lane);
    }
    if (live && lane == 0) {
        const uint32_t* root = reinterpret_cast<const uint32_t*>(roots + p * root_stride);
        uint32_t r[8];
        bool same = true;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            r[i] = root[i];
            same = same && r[i] == cur[i];
        }
        if (!mt_canonical(r)) bad |= 1u;
        ok[p] = !bad && same ? 1 : 0;
        if (status) status[p] = (bad & 1u) ? 1u : bad ? 2u : 0u;
    }
}

static const EdRow* rows_of(const swm_pedersen* p) { return reinterpret_cast<const EdRow*>(p->d_table); }
static Fr two_d() { return fp_from_u64<Fr>(2 * ED_D); }

static int mt_check_params(swm_ctx* ctx, const char* what, const swm_pedersen* leaf, const swm_pedersen* inner, size_t height, size_t leaf_len) {
    if (!merkle_height_ok(height))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: height %zu (%zu <= height <= %zu)", what, height, (size_t)MT_MIN_HEIGHT, (size_t)MT_MAX_HEIGHT);
    if (!leaf_len || leaf_len > (size_t)leaf->num_windows * leaf->window_size / 8)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: %zu leaf bytes do not fit %u windows of %u bits", what, leaf_len, leaf->num_windows,
                       leaf->window_size);
    if ((size_t)inner->num_windows * inner->window_size < 512)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: the two-to-one parameters hold fewer than 2 x 256 bits", what);
    return SWM_OK;
}

static int mt_alloc(swm_ctx* ctx, const char* what, const swm_pedersen* leaf, const swm_pedersen* inner, size_t height, size_t leaf_len,
                    std::unique_ptr<swm_merkle_tree>* out) {
    std::unique_ptr<swm_merkle_tree> t(new swm_merkle_tree);
    t->leaf = leaf;
    t->inner = inner;
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

static void mt_release(swm_ctx* ctx, std::unique_ptr<swm_merkle_tree>& t) {  // a create that failed after its allocation
    drain_streams(ctx);
    (void)hipFree(t->d_nodes);
    t.reset();
}

static int mt_blank_run(swm_ctx* ctx, swm_merkle_tree* t) {
    const unsigned levels = (unsigned)t->levels();
    uint32_t* d_chain = nullptr;
    SWM_TRY(scratch(ctx, "merkle.chain", (MT_MAX_LEVELS + 1) * 32, (void**)&d_chain));
    SWM_LAUNCH(ctx, "merkle_blank_chain", merkle_blank_chain_kernel, dim3(1), dim3(64), 0, rows_of(t->inner), t->inner->num_windows,
               t->inner->window_size, levels, d_chain, two_d());
    const size_t halves = 2 * t->num_nodes();
    const unsigned blocks = (unsigned)std::min<size_t>((halves + 255) / 256, 1u << 16);
    SWM_LAUNCH(ctx, "merkle_blank_fill", merkle_blank_fill_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<const uint4*>(d_chain), levels,
               reinterpret_cast<uint4*>(t->d_nodes));
    return SWM_OK;
}

static int mt_from_leaves_args(swm_ctx* ctx, const swm_pedersen* leaf, const swm_pedersen* inner, const void* leaves, size_t leaf_len, size_t n,
                               swm_merkle_tree** out, size_t* height) {
    if (!ctx || !leaf || !inner || !leaves || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_tree_create_from_leaves: bad arguments");
    if (n < 2 || (n & (n - 1)) || n > ((size_t)1 << (MT_MAX_HEIGHT - 1)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_tree_create_from_leaves: %zu leaves (a power of two, 2 .. 2^%zu)", n,
                       (size_t)MT_MAX_HEIGHT - 1);
    size_t h = 1;
    while (((size_t)1 << (h - 1)) < n) h++;
    *height = h;
    return mt_check_params(ctx, "merkle_tree_create_from_leaves", leaf, inner, h, leaf_len);
}

// The launches of one batch.  `d` is the batch's dirty set, d_leaves the batch's leaf bytes on the device.  *uploaded: an index
// list went up from `words` (host memory of this call), so the caller waits before `words` goes out of scope.
static int mt_update_run(swm_ctx* ctx, swm_merkle_tree* t, const MerkleDirty& d, const uint8_t* d_leaves, std::vector<uint32_t>* words,
                         bool* uploaded) {
    *uploaded = false;
    const size_t jobs = d.leaves.size();
    if (!jobs) return SWM_OK;
    const unsigned levels = (unsigned)t->levels();
    // leaf jobs (dst | src), then the parents of every level the finishing workgroup does not take
    std::vector<size_t> at(levels, 0);
    if (jobs > MT_TAIL) {
        words->resize(2 * jobs);
        for (size_t j = 0; j < jobs; j++) {
            (*words)[j] = d.leaves[j].index;
            (*words)[jobs + j] = d.leaves[j].src;
        }
        for (unsigned l = 0; l < levels && d.parents[l].size() > MT_TAIL; l++) {
            at[l] = words->size();
            words->insert(words->end(), d.parents[l].begin(), d.parents[l].end());
        }
    }
    uint32_t* d_words = nullptr;
    if (!words->empty()) {
        SWM_TRY(scratch(ctx, "merkle.jobs", words->size() * 4, (void**)&d_words));
        SWM_HIP(ctx, hipMemcpyAsync(d_words, words->data(), words->size() * 4, hipMemcpyHostToDevice, ctx->stream));
        *uploaded = true;
    }
    const Fr k2d = two_d();
    MtSmall small = {};
    if (jobs <= MT_TAIL)
        for (size_t j = 0; j < jobs; j++) {
            small.dst[j] = d.leaves[j].index;
            small.src[j] = d.leaves[j].src;
        }
    {
        const unsigned lanes = lanes_for(jobs);
        SWM_LAUNCH(ctx, "merkle_update_leaves", merkle_hash_indexed_kernel, dim3((unsigned)((jobs * lanes + 255) / 256)), dim3(256), 0,
                   rows_of(t->leaf), t->leaf->num_windows, t->leaf->window_size, d_leaves, t->leaf_len, t->leaf_len, jobs, lanes, k2d,
                   t->d_nodes, d_words, d_words ? d_words + jobs : nullptr, small);
    }
    unsigned l = 0;
    for (; l < levels && d.parents[l].size() > MT_TAIL; l++) {
        const size_t cnt = d.parents[l].size();
        const unsigned lanes = lanes_for(cnt);
        const uint32_t* list = d_words + at[l];
        SWM_LAUNCH(ctx, "merkle_update_level", merkle_hash_indexed_kernel, dim3((unsigned)((cnt * lanes + 255) / 256)), dim3(256), 0,
                   rows_of(t->inner), t->inner->num_windows, t->inner->window_size, t->d_nodes + 32 * merkle_level_offset(levels, l), (size_t)64,
                   (size_t)64, cnt, lanes, k2d, t->d_nodes + 32 * merkle_level_offset(levels, l + 1), list, list, MtSmall{});
    }
    // (the root's level always has one dirty node: l < levels here)
    MtTail tail = {};
    tail.levels = levels;
    tail.first = l;
    for (unsigned k = l; k < levels; k++) {
        tail.count[k] = (uint32_t)d.parents[k].size();
        for (size_t j = 0; j < d.parents[k].size(); j++) tail.node[k][j] = d.parents[k][j];
    }
    SWM_LAUNCH(ctx, "merkle_update_tail", merkle_tail_kernel, dim3(1), dim3(64 * MT_TAIL), 0, rows_of(t->inner), t->inner->num_windows,
               t->inner->window_size, t->d_nodes, tail, k2d);
    return SWM_OK;
}

static int mt_update_args(swm_ctx* ctx, const swm_merkle_tree* t, const uint64_t* indices, const void* leaves, size_t leaf_len, size_t count,
                          MerkleDirty* d) {
    if (!ctx || !t || (count && (!indices || !leaves))) return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_tree_update: bad arguments");
    if (leaf_len != t->leaf_len)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_tree_update: leaves of %zu bytes in a tree of %zu-byte leaves", leaf_len, t->leaf_len);
    size_t bad_at = 0;
    switch (merkle_dirty(t->height, indices, count, d, &bad_at)) {
        case MT_DIRTY_OK: return SWM_OK;
        case MT_DIRTY_BAD_INDEX:
            return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_tree_update: update %zu: leaf index %llu in a tree of %zu leaves", bad_at,
                           (unsigned long long)indices[bad_at], t->n());
        default: return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_tree_update: %zu updates in one call", count);
    }
}

static int mt_paths_run(swm_ctx* ctx, const swm_merkle_tree* t, const uint64_t* d_indices, size_t count, uint8_t* d_out) {
    const size_t words = count * t->levels() * 8;
    const unsigned blocks = (unsigned)std::min<size_t>((words + 255) / 256, 1u << 16);
    SWM_LAUNCH(ctx, "merkle_paths", merkle_paths_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<const uint32_t*>(t->d_nodes),
               (unsigned)t->levels(), d_indices, count, reinterpret_cast<uint32_t*>(d_out));
    return SWM_OK;
}

static int mt_verify_args(swm_ctx* ctx, const swm_pedersen* leaf, const swm_pedersen* inner, size_t height, const void* roots, size_t root_stride,
                          const void* leaves, size_t leaf_len, const void* indices, const void* siblings, size_t count, const void* ok) {
    if (!ctx || !leaf || !inner || (count && (!roots || !leaves || !indices || !siblings || !ok)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_verify_paths: bad arguments");
    if (root_stride != 0 && root_stride != 32)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_verify_paths: a root stride of %zu (0: one root for all paths, 32: one per path)", root_stride);
    if (count > 0x7FFFFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_verify_paths: %zu paths in one call", count);
    return mt_check_params(ctx, "merkle_verify_paths", leaf, inner, height, leaf_len);
}

static int mt_verify_run(swm_ctx* ctx, const swm_pedersen* leaf, const swm_pedersen* inner, size_t height, const uint8_t* d_roots,
                         size_t root_stride, const uint8_t* d_leaves, size_t leaf_len, const uint64_t* d_indices, const uint8_t* d_siblings,
                         size_t count, uint8_t* d_ok, uint32_t* d_status) {
    const unsigned lanes = lanes_for(count);
    SWM_LAUNCH(ctx, "merkle_verify_paths", merkle_verify_paths_kernel, dim3((unsigned)((count * lanes + 255) / 256)), dim3(256), 0, rows_of(leaf),
               leaf->num_windows, leaf->window_size, rows_of(inner), inner->num_windows, inner->window_size, (unsigned)(height - 1), d_roots,
               root_stride, d_leaves, leaf_len, d_indices, d_siblings, count, lanes, two_d(), d_ok, d_status);
    return SWM_OK;
}

}  // namespace swm

using namespace swm;

extern "C" {

int swm_merkle_tree_create_blank(swm_ctx* ctx, const swm_pedersen* leaf, const swm_pedersen* inner, size_t height, size_t leaf_len,
                                 swm_merkle_tree** out) {
    if (!ctx || !leaf || !inner || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_tree_create_blank: bad arguments");
    SWM_TRY(mt_check_params(ctx, "merkle_tree_create_blank", leaf, inner, height, leaf_len));
    SWM_ON_DEVICE(ctx);
    std::unique_ptr<swm_merkle_tree> t;
    SWM_TRY(mt_alloc(ctx, "merkle_tree_create_blank", leaf, inner, height, leaf_len, &t));
    const int rc = mt_blank_run(ctx, t.get());
    if (rc != SWM_OK) {
        mt_release(ctx, t);
        return rc;
    }
    *out = t.release();
    return SWM_OK;
}

int swm_merkle_tree_create_from_leaves_dev(swm_ctx* ctx, const swm_pedersen* leaf, const swm_pedersen* inner, const void* d_leaves,
                                           size_t leaf_len, size_t n_leaves, swm_merkle_tree** out) {
    size_t height = 0;
    SWM_TRY(mt_from_leaves_args(ctx, leaf, inner, d_leaves, leaf_len, n_leaves, out, &height));
    SWM_ON_DEVICE(ctx);
    std::unique_ptr<swm_merkle_tree> t;
    SWM_TRY(mt_alloc(ctx, "merkle_tree_create_from_leaves", leaf, inner, height, leaf_len, &t));
    const int rc = merkle_build_run(ctx, leaf, inner, (const uint8_t*)d_leaves, leaf_len, n_leaves, t->d_nodes);
    if (rc != SWM_OK) {
        mt_release(ctx, t);
        return rc;
    }
    *out = t.release();
    return SWM_OK;
}

int swm_merkle_tree_create_from_leaves(swm_ctx* ctx, const swm_pedersen* leaf, const swm_pedersen* inner, const uint8_t* leaves,
                                       size_t leaf_len, size_t n_leaves, swm_merkle_tree** out) {
    size_t height = 0;
    SWM_TRY(mt_from_leaves_args(ctx, leaf, inner, leaves, leaf_len, n_leaves, out, &height));
    SWM_ON_DEVICE(ctx);
    uint8_t* d_in = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", n_leaves * leaf_len + 32, (void**)&d_in));
    SWM_HIP(ctx, hipMemcpyAsync(d_in, leaves, n_leaves * leaf_len, hipMemcpyHostToDevice, ctx->stream));
    swm_merkle_tree* t = nullptr;
    const int rc = swm_merkle_tree_create_from_leaves_dev(ctx, leaf, inner, d_in, leaf_len, n_leaves, &t);
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // `leaves` is the caller's
    if (rc != SWM_OK) return rc;
    if (e != hipSuccess) {
        swm_merkle_tree_destroy(ctx, t);
        return set_err(ctx, SWM_ERR_HIP, "merkle_tree_create_from_leaves: %s", hipGetErrorString(e));
    }
    *out = t;
    return SWM_OK;
}

void swm_merkle_tree_destroy(swm_ctx* ctx, swm_merkle_tree* t) {
    if (!t) return;
    DeviceGuard guard(ctx);
    if (ctx) drain_streams(ctx);
    if (t->d_nodes) (void)hipFree(t->d_nodes);
    delete t;
}

int swm_merkle_tree_update_dev(swm_ctx* ctx, swm_merkle_tree* t, const uint64_t* indices, const void* d_leaves, size_t leaf_len, size_t count) {
    MerkleDirty d;
    SWM_TRY(mt_update_args(ctx, t, indices, d_leaves, leaf_len, count, &d));
    if (!count) return SWM_OK;
    SWM_ON_DEVICE(ctx);
    std::vector<uint32_t> words;
    bool uploaded = false;
    const int rc = mt_update_run(ctx, t, d, (const uint8_t*)d_leaves, &words, &uploaded);
    if (uploaded) SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `words` goes out of scope
    return rc;
}

int swm_merkle_tree_update(swm_ctx* ctx, swm_merkle_tree* t, const uint64_t* indices, const uint8_t* leaves, size_t leaf_len, size_t count) {
    MerkleDirty d;
    SWM_TRY(mt_update_args(ctx, t, indices, leaves, leaf_len, count, &d));
    if (!count) return SWM_OK;
    SWM_ON_DEVICE(ctx);
    uint8_t* d_in = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", count * leaf_len + 32, (void**)&d_in));
    SWM_HIP(ctx, hipMemcpyAsync(d_in, leaves, count * leaf_len, hipMemcpyHostToDevice, ctx->stream));
    std::vector<uint32_t> words;
    bool uploaded = false;
    const int rc = mt_update_run(ctx, t, d, d_in, &words, &uploaded);
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `leaves` is the caller's, `words` goes out of scope
    return rc;
}

int swm_merkle_tree_root(swm_ctx* ctx, const swm_merkle_tree* t, uint8_t root[32]) {
    if (!ctx || !t || !root) return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_tree_root: bad arguments");
    SWM_ON_DEVICE(ctx);
    SWM_HIP(ctx, hipMemcpyAsync(root, t->d_nodes + 32 * (t->num_nodes() - 1), 32, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWM_OK;
}

int swm_merkle_tree_nodes(swm_ctx* ctx, const swm_merkle_tree* t, uint8_t* nodes) {
    if (!ctx || !t || !nodes) return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_tree_nodes: bad arguments");
    SWM_ON_DEVICE(ctx);
    SWM_HIP(ctx, hipMemcpyAsync(nodes, t->d_nodes, t->num_nodes() * 32, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWM_OK;
}

int swm_merkle_tree_dev_nodes(const swm_merkle_tree* t, void** d_nodes, size_t* n_nodes) {
    if (!t || !d_nodes || !n_nodes) return set_err(nullptr, SWM_ERR_INVALID_ARG, "merkle_tree_dev_nodes: bad arguments");
    *d_nodes = t->d_nodes;
    *n_nodes = t->num_nodes();
    return SWM_OK;
}

int swm_merkle_tree_paths_dev(swm_ctx* ctx, const swm_merkle_tree* t, const void* d_indices, size_t count, void* d_siblings) {
    if (!ctx || !t || (count && (!d_indices || !d_siblings))) return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_tree_paths: bad arguments");
    if (!count) return SWM_OK;
    SWM_ON_DEVICE(ctx);
    return mt_paths_run(ctx, t, (const uint64_t*)d_indices, count, (uint8_t*)d_siblings);
}

int swm_merkle_tree_paths(swm_ctx* ctx, const swm_merkle_tree* t, const uint64_t* indices, size_t count, uint8_t* siblings) {
    if (!ctx || !t || (count && (!indices || !siblings))) return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_tree_paths: bad arguments");
    for (size_t p = 0; p < count; p++)
        if (indices[p] >= t->n())
            return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_tree_paths: path %zu: leaf index %llu in a tree of %zu leaves", p,
                           (unsigned long long)indices[p], t->n());
    if (!count) return SWM_OK;
    SWM_ON_DEVICE(ctx);
    const size_t bytes = count * t->levels() * 32;
    uint8_t *d_in = nullptr, *d_out = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", 8 * count, (void**)&d_in));
    SWM_TRY(scratch(ctx, "stage.b", bytes, (void**)&d_out));
    SWM_HIP(ctx, hipMemcpyAsync(d_in, indices, 8 * count, hipMemcpyHostToDevice, ctx->stream));
    SWM_TRY(mt_paths_run(ctx, t, (const uint64_t*)d_in, count, d_out));
    SWM_HIP(ctx, hipMemcpyAsync(siblings, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWM_OK;
}

int swm_merkle_verify_paths_dev(swm_ctx* ctx, const swm_pedersen* leaf, const swm_pedersen* inner, size_t height, const void* d_roots,
                                size_t root_stride, const void* d_leaves, size_t leaf_len, const void* d_indices, const void* d_siblings,
                                size_t count, void* d_ok, void* d_status) {
    SWM_TRY(mt_verify_args(ctx, leaf, inner, height, d_roots, root_stride, d_leaves, leaf_len, d_indices, d_siblings, count, d_ok));
    if (!count) return SWM_OK;
    SWM_ON_DEVICE(ctx);
    return mt_verify_run(ctx, leaf, inner, height, (const uint8_t*)d_roots, root_stride, (const uint8_t*)d_leaves, leaf_len,
                         (const uint64_t*)d_indices, (const uint8_t*)d_siblings, count, (uint8_t*)d_ok, (uint32_t*)d_status);
}

int swm_merkle_verify_paths(swm_ctx* ctx, const swm_pedersen* leaf, const swm_pedersen* inner, size_t height, const uint8_t* roots,
                            size_t root_stride, const uint8_t* leaves, size_t leaf_len, const uint64_t* indices, const uint8_t* siblings,
                            size_t count, uint8_t* ok, uint32_t* status) {
    SWM_TRY(mt_verify_args(ctx, leaf, inner, height, roots, root_stride, leaves, leaf_len, indices, siblings, count, ok));
    if (!count) return SWM_OK;
    SWM_ON_DEVICE(ctx);
    // indices | siblings | roots | leaves in one staging buffer; status | ok in the other
    const size_t sib_bytes = count * (height - 1) * 32, root_bytes = root_stride ? 32 * count : 32;
    uint8_t *d_in = nullptr, *d_out = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", 8 * count + sib_bytes + root_bytes + count * leaf_len, (void**)&d_in));
    SWM_TRY(scratch(ctx, "stage.b", 5 * count, (void**)&d_out));
    uint8_t *d_sib = d_in + 8 * count, *d_roots = d_sib + sib_bytes, *d_leaves = d_roots + root_bytes;
    SWM_HIP(ctx, hipMemcpyAsync(d_in, indices, 8 * count, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(d_sib, siblings, sib_bytes, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(d_roots, roots, root_bytes, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(d_leaves, leaves, count * leaf_len, hipMemcpyHostToDevice, ctx->stream));
    SWM_TRY(mt_verify_run(ctx, leaf, inner, height, d_roots, root_stride, d_leaves, leaf_len, (const uint64_t*)d_in, d_sib, count,
                          d_out + 4 * count, (uint32_t*)d_out));
    SWM_HIP(ctx, hipMemcpyAsync(ok, d_out + 4 * count, count, hipMemcpyDeviceToHost, ctx->stream));
    if (status) SWM_HIP(ctx, hipMemcpyAsync(status, d_out, 4 * count, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWM_OK;
}

}  // extern "C"

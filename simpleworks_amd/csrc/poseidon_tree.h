// poseidon_tree.h — the resident Poseidon Merkle tree's handle and the two hashes of the tree on one lane (poseidon_tree.hip builds
// and updates the tree and checks paths; poseidon_tree_witness.hip walks a path with the same functions and reads the tree's
// nodes).
//   leaf digest   HL(leaf) = the sponge over the leaf's bytes (poseidon_hash_kernel<true>, one output)
//   two-to-one    H2(a, b) = state (a, b, 0), one permutation, state[0] (poseidon_hash_kernel<false>, n_in = 2, n_out = 1)
// A tree input is a canonical node (< r; a caller's sibling may be any value < 2^256) or a 31-byte chunk: each enters as an
// absorbed element through the product with table row 0, so the bounds at the head of poseidon.hip hold as they stand.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ff.cuh"
#include "fr29.cuh"
#include "poseidon.h"
#include "poseidon_permute.cuh"

struct swm_poseidon_tree {
    const swm_poseidon* params = nullptr;
    size_t height = 0, leaf_len = 0;
    uint8_t* d_nodes = nullptr;  // (2 n - 1) x 32 bytes, owned
    size_t levels() const { return height - 1; }
    size_t n() const { return (size_t)1 << (height - 1); }
    size_t num_nodes() const { return 2 * n() - 1; }
};

namespace swm {

struct PtParams {  // the launch-uniform part of a swm_poseidon
    unsigned rows, half_full, partial, alpha;
};

// what a launch of one lane per item over `p` takes: the uniform part, the table, its LDS bytes, the workgroups for `count` items
static PtParams pt_params(const swm_poseidon* p) { return PtParams{(unsigned)p->rows, p->full_rounds / 2, p->partial_rounds, p->alpha}; }
static size_t pt_lds(const swm_poseidon* p) { return p->rows * PS_ROW * sizeof(uint32_t); }
static const uint4* pt_table(const swm_poseidon* p) { return reinterpret_cast<const uint4*>(p->d_table); }
static unsigned pt_blocks(size_t count) { return (unsigned)((count + PS_LANES - 1) / PS_LANES); }

__device__ __forceinline__ void pt_load_table(uint32_t* tab, const uint4* __restrict__ table, unsigned rows) {
    for (unsigned i = threadIdx.x; i < rows * (PS_ROW / 4); i += blockDim.x) reinterpret_cast<uint4*>(tab)[i] = table[i];
    __syncthreads();
}

__device__ __forceinline__ Fr pt_load(const uint32_t* p) {
    Fr x;
#pragma unroll
    for (int w = 0; w < 8; w++) x.v[w] = p[w];
    return x;
}
__device__ __forceinline__ void pt_store(uint32_t* p, const Fr& x) {
#pragma unroll
    for (int w = 0; w < 8; w++) p[w] = x.v[w];
}
__device__ __forceinline__ bool pt_canonical(const Fr& x) {
    Fr r;
#pragma unroll
    for (int w = 0; w < 8; w++) r.v[w] = FrParams::P[w];
    return fp_cmp_std(x, r) < 0;
}

// state[0] out of the 2^261 form: (lazy state < 6r) x 1 -> < 2r -> canonical
__device__ __forceinline__ Fr pt_squeeze(const Fr29& s0) {
    Fr29 one;
#pragma unroll
    for (int i = 0; i < 9; i++) one.l[i] = i == 0 ? 1u : 0u;
    return fr29_pack(fr29_canonical(fr29_mul_fenced(s0, one), true));
}

// H2(a, b): a and b in standard form, < 2^256
__device__ __forceinline__ Fr pt_hash2(const uint32_t* tab, const PtParams& P, const Fr& a, const Fr& b) {
    const Fr29 to_mont = ps_row(tab, 0);
    Fr29 s0 = fr29_mul_fenced(fr29_unpack(a), to_mont), s1 = fr29_mul_fenced(fr29_unpack(b), to_mont), s2;
#pragma unroll
    for (int i = 0; i < 9; i++) s2.l[i] = 0;
    ps_permute(tab, P.half_full, P.partial, P.alpha, 31 - __clz((int)P.alpha), s0, s1, s2);
    return pt_squeeze(s0);
}

// HL: the digest of item `item` of `leaves` (leaf_len bytes each)
__device__ __forceinline__ Fr pt_hash_leaf(const uint32_t* tab, const PtParams& P, const uint8_t* __restrict__ leaves, size_t item,
                                           size_t leaf_len) {
    const Fr29 to_mont = ps_row(tab, 0);
    const int alpha_top = 31 - __clz((int)P.alpha);
    const size_t n_elems = (8 + leaf_len + 30) / 31;
    Fr29 s0, s1, s2;
#pragma unroll
    for (int i = 0; i < 9; i++) s0.l[i] = s1.l[i] = s2.l[i] = 0;
    bool unused = false;
#pragma unroll 1
    for (size_t e = 0; e < n_elems; e += 2) {
        if (e) ps_permute(tab, P.half_full, P.partial, P.alpha, alpha_top, s0, s1, s2);
        s0 = fr29_add(s0, fr29_mul_fenced(fr29_unpack(ps_fetch<true>(leaves, item, leaf_len, e, unused)), to_mont));
        if (e + 1 < n_elems) s1 = fr29_add(s1, fr29_mul_fenced(fr29_unpack(ps_fetch<true>(leaves, item, leaf_len, e + 1, unused)), to_mont));
    }
    ps_permute(tab, P.half_full, P.partial, P.alpha, alpha_top, s0, s1, s2);
    return pt_squeeze(s0);
}

// Path::verify's walk: cur_0 = HL(leaf), cur_{l+1} = H2 of (cur_l, sibling_l) in the order bit l of the index gives.  `digests`
// (may be NULL): cur_0 .. cur_L, 8 words each.  bad |= 1 for a sibling >= r.  Returns cur_L.
__device__ __forceinline__ Fr pt_walk(const uint32_t* tab, const PtParams& P, const uint8_t* __restrict__ leaves, size_t item, size_t leaf_len,
                                      uint64_t index, const uint32_t* __restrict__ sib, unsigned levels, uint32_t* __restrict__ digests,
                                      unsigned& bad) {
    Fr cur = pt_hash_leaf(tab, P, leaves, item, leaf_len);
    if (digests) pt_store(digests, cur);
#pragma unroll 1
    for (unsigned l = 0; l < levels; l++) {
        const Fr s = pt_load(sib + 8 * l);
        if (!pt_canonical(s)) bad |= 1u;
        const bool right = (index >> l) & 1u;  // the running digest is the right child
        cur = pt_hash2(tab, P, right ? s : cur, right ? cur : s);
        if (digests) pt_store(digests + 8 * (l + 1), cur);
    }
    return cur;
}

}  // namespace swm

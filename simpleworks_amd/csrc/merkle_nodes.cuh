// merkle_nodes.cuh — kernels over the node array of a resident Merkle tree that do not hash: filling a blank tree from its chain
// of per-level digests and reading authentication paths.  The layout (n = 2^L leaf digests | n / 2 | ... | root, 32 bytes each) is
// shared by the Pedersen tree (merkle_tree.hip) and the Poseidon tree (poseidon_tree.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace swm {

__device__ __forceinline__ size_t mt_level_offset(unsigned levels, unsigned l) { return ((size_t)2 << levels) - (((size_t)2 << levels) >> l); }

// every node of level l = chain[l]; i runs over the 16-byte halves of the nodes
static __global__ void __launch_bounds__(256) merkle_blank_fill_kernel(const uint4* __restrict__ chain, unsigned levels, uint4* __restrict__ nodes) {
    const size_t halves = 2 * (((size_t)2 << levels) - 1);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < halves; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long from_root = (((unsigned long long)2 << levels) - 2) - (i >> 1);  // 0 at the root
        const unsigned level = levels - (63u - (unsigned)__clzll((long long)(from_root + 1)));
        nodes[i] = chain[2 * level + (i & 1)];
    }
}

// word i of the output: sibling of level l of path p, bottom up; an index beyond the leaves reads as zeros
static __global__ void __launch_bounds__(256) merkle_paths_kernel(const uint32_t* __restrict__ nodes, unsigned levels,
                                                           const uint64_t* __restrict__ indices, size_t count, uint32_t* __restrict__ out) {
    const size_t words = count * levels * 8;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
        const size_t s = i >> 3, p = s / levels;
        const unsigned l = (unsigned)(s % levels);
        const uint64_t index = indices[p];
        out[i] = (index >> levels) ? 0u : nodes[8 * (mt_level_offset(levels, l) + ((index >> l) ^ 1)) + (i & 7)];
    }
}

}  // namespace swm

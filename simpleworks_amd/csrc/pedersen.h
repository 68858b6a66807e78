// pedersen.h — the resident form of a Pedersen parameter set (pedersen.hip builds it; merkle_witness.hip and merkle_tree.hip
// read it) and the host entry points of pedersen.hip that merkle_tree.hip builds on.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct swm_ctx;

struct swm_pedersen {
    void* d_table = nullptr;  // num_windows x 2^window_size rows (swm::EdRow)
    unsigned num_windows = 0, window_size = 0;
};

namespace swm {

// lanes per hash for a launch of `count` hashes: a power of two <= 64, more the fewer hashes there are
unsigned lanes_for(size_t count);
// `count` hashes of `len` bytes each, input h at d_in + h * stride, digest h at d_out + 32 h
int pedersen_hash_run(swm_ctx* ctx, const swm_pedersen* p, const uint8_t* d_in, size_t stride, size_t len, size_t count, uint8_t* d_out);
// nodes: n leaf digests | n / 2 | ... | root — (2 n - 1) x 32 bytes
int merkle_build_run(swm_ctx* ctx, const swm_pedersen* leaf, const swm_pedersen* inner, const uint8_t* d_leaves, size_t leaf_len, size_t n,
                     uint8_t* d_nodes);

}  // namespace swm

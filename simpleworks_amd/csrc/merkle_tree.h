// merkle_tree.h — the resident Pedersen Merkle tree's handle (merkle_tree.hip builds and updates the tree and checks paths;
// pedersen_payment_witness.hip reads its nodes).  Layout: merkle_tree.hip's head.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pedersen.h"

struct swm_merkle_tree {
    const swm_pedersen* leaf = nullptr;
    const swm_pedersen* inner = nullptr;
    size_t height = 0, leaf_len = 0;
    uint8_t* d_nodes = nullptr;  // (2 n - 1) x 32 bytes, owned
    size_t levels() const { return height - 1; }
    size_t n() const { return (size_t)1 << (height - 1); }
    size_t num_nodes() const { return 2 * n() - 1; }
};

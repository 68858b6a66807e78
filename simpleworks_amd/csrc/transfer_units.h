// transfer_units.h — what the two transfer units (transfer_witness.hip over the Poseidon account tree, pedersen_transfer_witness.hip
// over the Pedersen one) hand to another unit that lays their witnesses out in a vector of its own (rollup_witness.hip): the
// circuit handles, the tree checks and the launchers with the item stride as an argument.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "context.h"
#include "ff.cuh"
#include "host/pedersen_transfer_shape.h"
#include "host/transfer_shape.h"
#include "merkle_tree.h"
#include "pedersen.h"
#include "poseidon_tree.h"
#include "witness_runs.h"

struct swm_transfer_circuit {
    swm_schnorr_circuit schnorr;      // over PY_MSG_LEN bytes
    swm_poseidon_tree_circuit tree;   // over PY_LEAF_LEN bytes
    swm::TransferShape shape;
};

struct swm_pedersen_transfer_circuit {
    swm_schnorr_circuit schnorr;  // over PP_MSG_LEN bytes
    const swm_pedersen* leaf = nullptr;
    const swm_pedersen* inner = nullptr;
    swm::PedersenTransferShape shape;
};

namespace swm {

struct TransferRunOut {      // the small results of a pass over n transfers, on the device (the unit's aux scratch)
    const uint32_t* roots;   // 2 x n x 8 words, canonical: old roots | new roots
    const uint8_t* flags;    // n
    const uint32_t* status;  // n
    const uint32_t* verdict; // 1: nonzero when the table is not the tree's (then nothing else here is defined)
};

// n transfers on device buffers, in order: the tree's nodes and d_accounts are advanced (unless the table is refused).  Item i's
// witnesses from d_w + i * stride, nothing between its num_witness and the stride is touched.  d_w 16-byte aligned, d_sigs 4-byte.
int transfer_run_strided(swm_ctx* ctx, const swm_transfer_circuit* c, swm_poseidon_tree* tree, uint8_t* d_accounts, const uint8_t* d_msgs,
                         const uint8_t* d_sigs, size_t n, Fr* d_w, size_t stride, TransferRunOut* out);
int pedersen_transfer_run_strided(swm_ctx* ctx, const swm_pedersen_transfer_circuit* c, swm_merkle_tree* tree, uint8_t* d_accounts,
                                  const uint8_t* d_msgs, const uint8_t* d_sigs, size_t n, Fr* d_w, size_t stride, TransferRunOut* out);
int transfer_check_tree(swm_ctx* ctx, const char* what, const swm_transfer_circuit* c, const swm_poseidon_tree* t);
int pedersen_transfer_check_tree(swm_ctx* ctx, const char* what, const swm_pedersen_transfer_circuit* c, const swm_merkle_tree* t);

}  // namespace swm

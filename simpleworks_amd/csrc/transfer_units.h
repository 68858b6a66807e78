// transfer_units.h — what the two transfer units (transfer_witness.hip over the Poseidon account tree, pedersen_transfer_witness.hip
// over the Pedersen one) hand to the host layer (ledger_witness_host.h) and to another unit that lays their witnesses out in a
// vector of its own (rollup_witness.hip): the circuit handles, the launchers with the item stride as an argument, and per tree
// what a unit struct U is made of but its name.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "context.h"
#include "ff.cuh"
#include "host/pedersen_transfer_shape.h"
#include "host/transfer_shape.h"
#include "ledger_witness_host.h"
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

static_assert(PP_MSG_LEN == PY_MSG_LEN && PP_LEAF_LEN == PY_LEAF_LEN, "the block driver's message and leaf");

// n transfers on device buffers, in order: the tree's nodes and d_accounts are advanced (unless the table is refused).  Item i's
// witnesses from d_w + i * stride, nothing between its num_witness and the stride is touched.  d_w 16-byte aligned, d_sigs 4-byte.
int transfer_run_strided(swm_ctx* ctx, const swm_transfer_circuit* c, swm_poseidon_tree* tree, uint8_t* d_accounts, const uint8_t* d_msgs,
                         const uint8_t* d_sigs, size_t n, Fr* d_w, size_t stride, BlockRunOut* out);
int pedersen_transfer_run_strided(swm_ctx* ctx, const swm_pedersen_transfer_circuit* c, swm_merkle_tree* tree, uint8_t* d_accounts,
                                  const uint8_t* d_msgs, const uint8_t* d_sigs, size_t n, Fr* d_w, size_t stride, BlockRunOut* out);

struct PoseidonTransfers {  // a unit over the Poseidon tree adds its name
    using Circuit = swm_transfer_circuit;
    using Tree = swm_poseidon_tree;
    static constexpr const char* accounts_scratch = "transfer.accounts";
    static constexpr const char* witness_scratch = "transfer.w";
    static constexpr auto run = transfer_run_strided;
    static int check_tree(swm_ctx* ctx, const char* what, const Circuit* c, const Tree* t) {
        return ledger_check_tree(ctx, what, c->tree.params, c->shape.height, t);
    }
};

struct PedersenTransfers {  // a unit over the Pedersen tree adds its name
    using Circuit = swm_pedersen_transfer_circuit;
    using Tree = swm_merkle_tree;
    static constexpr const char* accounts_scratch = "ptransfer.accounts";
    static constexpr const char* witness_scratch = "ptransfer.w";
    static constexpr auto run = pedersen_transfer_run_strided;
    static int check_tree(swm_ctx* ctx, const char* what, const Circuit* c, const Tree* t) {
        return ledger_check_tree(ctx, what, c->leaf, c->inner, c->shape.height, t);
    }
};

}  // namespace swm

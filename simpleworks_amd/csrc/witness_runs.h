// witness_runs.h — the two witness launchers that another circuit's unit may reuse for a block of its own witness vector
// (payment_witness.hip does): schnorr_witness.hip and poseidon_tree_witness.hip define them next to their kernels.  Both write
// item i's block at d_witness + i * stride; the stand-alone circuits pass their own num_witness as the stride, a composed circuit
// its larger one with d_witness moved to the block's first element.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "context.h"
#include "ff.cuh"
#include "host/poseidon_tree_shape.h"
#include "host/schnorr_shape.h"
#include "poseidon.h"
#include "poseidon_tree.h"
#include "schnorr.h"

struct swm_schnorr_circuit {
    const swm_schnorr* params = nullptr;
    swm::SchnorrShape shape;
};

struct swm_poseidon_tree_circuit {
    const swm_poseidon* params = nullptr;
    swm::PoseidonTreeShape shape;
};

namespace swm {

// One workgroup per signature.  d_keys: 64 bytes each, d_sigs: 64 bytes each (both 4-byte aligned), d_msgs: msg_len bytes each.
// d_ok, d_status (may be NULL): per item.  A refused key clears the item's c->shape.num_witness elements and nothing beyond them.
int schnorr_witness_run(swm_ctx* ctx, const swm_schnorr_circuit* c, const uint8_t* d_keys, const uint8_t* d_msgs, const uint8_t* d_sigs,
                        size_t count, Fr* d_witness, size_t stride, uint8_t* d_ok, uint32_t* d_status);
// the host form's check: what the device form reports per item
int schnorr_check_keys(swm_ctx* ctx, const uint8_t* keys, size_t count);

// `count` membership witnesses.  With a tree the digests and the siblings are gathered from its nodes (d_siblings is not read);
// without one the paths are walked and d_roots (may be NULL) takes their roots.
int ptw_run(swm_ctx* ctx, const swm_poseidon_tree_circuit* c, const swm_poseidon_tree* tree, const uint8_t* d_leaves, const uint64_t* d_indices,
            const uint8_t* d_siblings, size_t count, Fr* d_witness, size_t stride, uint32_t* d_roots);
// Its record half alone, from digests (count x (L + 1) x 8 words, cur_0 .. cur_L per path) and siblings (count x L x 8 words) that
// the caller has: one launch.  own_path false: an update block (transfer_witness.hip), which walks another block's path with
// another leaf: deltas | leaf chain | levels from d_witness on, no bits and no siblings of its own.
int ptw_record(swm_ctx* ctx, const swm_poseidon_tree_circuit* c, const uint8_t* d_leaves, const uint64_t* d_indices, const uint32_t* d_dig,
               const uint32_t* d_sib, size_t count, Fr* d_witness, size_t stride, bool own_path);

}  // namespace swm

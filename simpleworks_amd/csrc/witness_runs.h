// witness_runs.h — the two witness launchers that another circuit's unit may reuse for a block of its own witness vector
// (payment_witness.hip does): schnorr_witness.hip and poseidon_tree_witness.hip define them next to their kernels.  Both write
// item i's block at d_witness + i * stride; the stand-alone circuits pass their own num_witness as the stride, a composed circuit
// its larger one with d_witness moved to the block's first element.  And the parts of a payment's witness pass that do not depend
// on the account tree's hash (payment_witness.hip defines them; pedersen_payment_witness.hip calls them with its own offsets).
// Kernel launchers only: the host layer above them is witness_host.h and, for payments, transfers and account updates over either
// tree, ledger_witness_host.h (which also holds the tree and CRH checks of the ledger circuits).
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
#include "swmarlin.h"

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

// ---- a payment (payment_witness.hip): messages of 10 bytes, leaves of 72, whatever the tree hashes with
// The 72-byte sender leaves unzipped into the 64-byte key array the Schnorr kernel reads, and the two id bytes of each message as
// uint64 leaf indices masked to `levels` bits.
int payment_prep_run(swm_ctx* ctx, const uint8_t* d_msgs, const uint8_t* d_sender_leaves, size_t n, unsigned levels, uint32_t* d_keys,
                     uint64_t* d_idx_s, uint64_t* d_idx_r);
// The 704 bit witnesses (64 balance bits and 64 diff bits from balance_at, 576 recipient leaf bits from recipient_bits_at), the flag
// byte (bit 0: d_sig_ok, bit 1: amount <= balance) and the status word completed: bit 1 a sibling >= r (the two sibling arrays may
// be NULL: a resident tree's), bit 2 an id at or above 2^levels.
int payment_bits_run(swm_ctx* ctx, size_t n, size_t stride, size_t balance_at, size_t recipient_bits_at, unsigned levels, const uint8_t* d_msgs,
                     const uint8_t* d_sender_leaves, const uint8_t* d_recipient_leaves, const uint32_t* d_sender_sib,
                     const uint32_t* d_recipient_sib, const uint8_t* d_sig_ok, Fr* d_w, uint8_t* d_flags, uint32_t* d_status);

// ---- Pedersen sections (pedersen_payment_witness.hip): the leaf stages and the level stages of every section of n items, one
// launch each.  Section k of item i: the 72-byte leaf at leaves + 72 i, cur_0 .. cur_L at dig + dig_stride i (words), the L
// siblings at sib + 8 L i, the leaf index idx[i]; its witnesses from d_w + stride i + at.  update: an update section (the transfer
// circuit over the Pedersen tree): a level stores no dir and no sibling, its groups two elements earlier.
static constexpr unsigned PP_MAX_SECTIONS = 4;
struct PpSection {
    const uint8_t* leaves;
    const uint32_t *dig, *sib;
    const uint64_t* idx;
    size_t at;
    unsigned update;
};
struct PpArgs {
    size_t stride, dig_stride;
    unsigned levels, sections;
    PpSection s[PP_MAX_SECTIONS];
};
int pp_record_run(swm_ctx* ctx, const swm_pedersen* leaf, const swm_pedersen* inner, const PpArgs& A, size_t n, Fr* d_w);

// ---- an account table against a Pedersen tree's leaf level (pedersen_transfer_witness.hip: pedersen_transfer_check_kernel): the
// digest of each of the n_leaves 72-byte entries against node h; a leaf that differs stores 1 into *d_verdict, which the caller has
// cleared in stream order.  One launch.
int pedersen_transfer_check_run(swm_ctx* ctx, const swm_pedersen* leaf, const uint32_t* d_nodes, const uint8_t* d_accounts, unsigned n_leaves,
                                uint32_t* d_verdict);

// ---- a block of transfers (transfer_witness.hip), whatever the tree hashes with
// The senders' keys out of the account table (2^levels leaves of 72 bytes): 16 words per transfer for the Schnorr kernel.
int transfer_prep_run(swm_ctx* ctx, const uint8_t* d_msgs, const uint8_t* d_accounts, size_t n, unsigned levels, uint32_t* d_keys);
// The 769 loose elements of a transfer: balance, diff, sum and the recipient's bits out of d_leaves (4 x n x 72 bytes: sender old |
// sender new | recipient in the tree of R1 | recipient new), R1 = the last of the sender's new digests (n x (levels + 1) x 8 words).
int transfer_bits_run(swm_ctx* ctx, size_t n, size_t stride, size_t balance_at, size_t sum_at, size_t r1_at, size_t recipient_bits_at,
                      unsigned levels, const uint8_t* d_leaves, const uint32_t* d_sender_new_dig, Fr* d_w);

}  // namespace swm

//! Raw bindings: one declaration per symbol of include/swmarlin.h that the Marlin surface needs (plus the K1-K4 kernel
//! entry points for callers that keep their own arkworks pipeline).
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_uint, c_void};

#[repr(C)] pub struct swm_ctx { _p: [u8; 0] }
#[repr(C)] pub struct swm_rng { _p: [u8; 0] }
#[repr(C)] pub struct swm_srs { _p: [u8; 0] }
#[repr(C)] pub struct swm_pk { _p: [u8; 0] }
#[repr(C)] pub struct swm_vk { _p: [u8; 0] }
#[repr(C)] pub struct swm_bases { _p: [u8; 0] }
#[repr(C)] pub struct swm_pedersen { _p: [u8; 0] }
#[repr(C)] pub struct swm_schnorr { _p: [u8; 0] }
#[repr(C)] pub struct swm_merkle_circuit { _p: [u8; 0] }
#[repr(C)] pub struct swm_merkle_tree { _p: [u8; 0] }
#[repr(C)] pub struct swm_schnorr_circuit { _p: [u8; 0] }
#[repr(C)] pub struct swm_poseidon { _p: [u8; 0] }
#[repr(C)] pub struct swm_poseidon_circuit { _p: [u8; 0] }
#[repr(C)] pub struct swm_poseidon_tree { _p: [u8; 0] }
#[repr(C)] pub struct swm_poseidon_tree_circuit { _p: [u8; 0] }
#[repr(C)] pub struct swm_payment_circuit { _p: [u8; 0] }
#[repr(C)] pub struct swm_pedersen_payment_circuit { _p: [u8; 0] }
#[repr(C)] pub struct swm_transfer_circuit { _p: [u8; 0] }
#[repr(C)] pub struct swm_pedersen_transfer_circuit { _p: [u8; 0] }
#[repr(C)] pub struct swm_account_update_circuit { _p: [u8; 0] }
#[repr(C)] pub struct swm_pedersen_account_update_circuit { _p: [u8; 0] }
#[repr(C)] pub struct swm_program { _p: [u8; 0] }

pub const SWM_OK: c_int = 0;
pub const SWM_ERR_UNSATISFIED: c_int = -5;
pub const SWM_PROOF_UNCOMPRESSED: c_uint = 1;
/// swm_{pk,vk}_{serialize,deserialize}_ex: the serialize_uncompressed layout; readers only, with the former: deserialize_unchecked
pub const SWM_KEY_UNCOMPRESSED: c_uint = 1;
pub const SWM_KEY_UNCHECKED: c_uint = 2;

/// struct swm_r1cs: a synthesised constraint system as flat arrays (instance[0] is the constant one).
#[repr(C)]
pub struct swm_r1cs {
    pub num_instance: usize,
    pub num_witness: usize,
    pub num_constraints: usize,
    pub instance: *const u64,
    pub witness: *const u64,
    pub a_rowptr: *const u32, pub a_col: *const u32, pub a_val: *const u64,
    pub b_rowptr: *const u32, pub b_col: *const u32, pub b_val: *const u64,
    pub c_rowptr: *const u32, pub c_col: *const u32, pub c_val: *const u64,
}

pub type swm_fill_bytes_fn = unsafe extern "C" fn(user: *mut c_void, dest: *mut u8, len: usize);
pub type swm_allgather_fn = unsafe extern "C" fn(user: *mut c_void, send: *const c_void, bytes: usize, recv: *mut c_void) -> c_int;

extern "C" {
    pub fn swm_version() -> c_int;
    pub fn swm_strerror(code: c_int) -> *const c_char;
    pub fn swm_init(device: c_int, out: *mut *mut swm_ctx) -> c_int;
    pub fn swm_destroy(ctx: *mut swm_ctx);
    pub fn swm_last_error(ctx: *mut swm_ctx) -> *const c_char;

    // generate_rand / caller-owned randomness (src/marlin/mod.rs:33-35, :49, :73, :83)
    pub fn swm_rng_test_new(out: *mut *mut swm_rng) -> c_int;
    pub fn swm_rng_from_seed(seed: *const u8, out: *mut *mut swm_rng) -> c_int;
    pub fn swm_rng_from_callback(fill_bytes: swm_fill_bytes_fn, user: *mut c_void, out: *mut *mut swm_rng) -> c_int;
    pub fn swm_rng_from_chacha(key: *const u8, word_pos: u64, rounds: c_int, out: *mut *mut swm_rng) -> c_int;
    pub fn swm_rng_word_pos(rng: *const swm_rng, word_pos: *mut u64) -> c_int;
    pub fn swm_rng_fill_bytes(rng: *mut swm_rng, dest: *mut u8, len: usize) -> c_int;
    pub fn swm_rng_fill_bytes_cb(user: *mut c_void, dest: *mut u8, len: usize);
    pub fn swm_rng_free(rng: *mut swm_rng);

    // generate_universal_srs (src/marlin/mod.rs:45-55)
    pub fn swm_generate_universal_srs(ctx: *mut swm_ctx, nc: usize, nv: usize, nnz: usize, rng: *mut swm_rng,
                                      out: *mut *mut swm_srs) -> c_int;
    pub fn swm_srs_destroy(ctx: *mut swm_ctx, srs: *mut swm_srs);
    pub fn swm_srs_max_degree(srs: *const swm_srs) -> usize;
    pub fn swm_srs_export(ctx: *mut swm_ctx, srs: *const swm_srs, first: usize, count: usize, powers_xy: *mut u64,
                          gamma_xy: *mut u64, h: *mut u64, beta_h: *mut u64) -> c_int;
    pub fn swm_srs_import(ctx: *mut swm_ctx, powers_xy: *const u64, n_powers: usize, gamma_xy: *const u64,
                          h: *const u64, beta_h: *const u64, out: *mut *mut swm_srs) -> c_int;

    // generate_proving_and_verifying_keys (src/marlin/mod.rs:88-94)
    pub fn swm_generate_proving_and_verifying_keys(ctx: *mut swm_ctx, srs: *const swm_srs, cs: *const swm_r1cs,
                                                   pk: *mut *mut swm_pk, vk: *mut *mut swm_vk) -> c_int;
    pub fn swm_pk_destroy(ctx: *mut swm_ctx, pk: *mut swm_pk);
    pub fn swm_pk_retain(pk: *mut swm_pk) -> c_int;
    pub fn swm_pk_attach(ctx: *mut swm_ctx, pk: *mut swm_pk) -> c_int;
    pub fn swm_pk_device(pk: *const swm_pk) -> c_int;
    pub fn swm_pk_refcount(pk: *const swm_pk) -> c_int;
    pub fn swm_vk_destroy(vk: *mut swm_vk);

    // generate_proof (src/marlin/mod.rs:70-77) and verify_proof (:79-86)
    pub fn swm_generate_proof(ctx: *mut swm_ctx, pk: *const swm_pk, cs: *const swm_r1cs, rng: *mut swm_rng,
                              proof_out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    /// flags: SWM_PROOF_UNCOMPRESSED = 1 (the proof as serialize_uncompressed bytes, <= 2048 B)
    pub fn swm_generate_proof_ex(ctx: *mut swm_ctx, pk: *const swm_pk, cs: *const swm_r1cs, rng: *mut swm_rng, flags: c_uint,
                                 proof_out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    pub fn swm_proof_recode(bytes: *const u8, len: usize, to_uncompressed: c_int, out: *mut u8, cap: usize, out_len: *mut usize) -> c_int;
    pub fn swm_verify_proof(vk: *const swm_vk, public_inputs: *const u64, n: usize, proof: *const u8, len: usize,
                            rng: *mut swm_rng, ok: *mut c_int) -> c_int;
    // batch form (an extension beyond the reference's calls): `count` proofs against one key, one pairing check on the GPU
    pub fn swm_verify_proofs_batch(ctx: *mut swm_ctx, vk: *const swm_vk, public_inputs: *const u64, n_inputs: usize,
                                   proofs: *const *const u8, lens: *const usize, count: usize, flags: c_uint, rng: *mut swm_rng,
                                   ok: *mut c_int, results: *mut c_int) -> c_int;
    pub fn swm_selftest_verify_batch(ctx: *mut swm_ctx, vk: *const swm_vk, public_inputs: *const u64, n_inputs: usize,
                                     proofs: *const *const u8, lens: *const usize, count: usize, flags: c_uint, rng: *mut swm_rng,
                                     ok: *mut c_int, results: *mut c_int, tw_xy: *mut u64, tc_xy: *mut u64) -> c_int;

    // src/marlin/serialization.rs:5-45 (ark-serialize bytes in both directions)
    pub fn swm_vk_serialize(vk: *const swm_vk, out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    pub fn swm_vk_deserialize(bytes: *const u8, len: usize, out: *mut *mut swm_vk) -> c_int;
    pub fn swm_proof_validate(bytes: *const u8, len: usize) -> c_int;
    pub fn swm_pk_serialize(ctx: *mut swm_ctx, pk: *const swm_pk, out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    pub fn swm_pk_deserialize(ctx: *mut swm_ctx, bytes: *const u8, len: usize, out: *mut *mut swm_pk) -> c_int;
    // the other two forms of a key: flags = 0 is the function above; SWM_KEY_UNCOMPRESSED; readers: | SWM_KEY_UNCHECKED
    pub fn swm_vk_serialize_ex(vk: *const swm_vk, flags: c_uint, out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    pub fn swm_vk_deserialize_ex(bytes: *const u8, len: usize, flags: c_uint, out: *mut *mut swm_vk) -> c_int;
    pub fn swm_pk_serialize_ex(ctx: *mut swm_ctx, pk: *const swm_pk, flags: c_uint, out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    pub fn swm_pk_deserialize_ex(ctx: *mut swm_ctx, bytes: *const u8, len: usize, flags: c_uint, out: *mut *mut swm_pk) -> c_int;
    pub fn swm_r1cs_is_satisfied(ctx: *mut swm_ctx, cs: *const swm_r1cs, ok: *mut c_int, first_bad: *mut usize) -> c_int;

    // one proof over several GPUs
    pub fn swm_set_msm_sharding(ctx: *mut swm_ctx, rank: c_uint, world: c_uint, allgather: Option<swm_allgather_fn>,
                                user: *mut c_void) -> c_int;
    pub fn swm_set_rccl_comm(ctx: *mut swm_ctx, nccl_comm: *mut c_void, rank: c_uint, world: c_uint) -> c_int;

    // K1-K4 for callers that keep arkworks' prover and only swap kernels
    pub fn swm_srs_upload(ctx: *mut swm_ctx, xy: *const u64, n: usize, out: *mut *mut swm_bases) -> c_int;
    pub fn swm_srs_free(ctx: *mut swm_ctx, bases: *mut swm_bases) -> c_int;
    pub fn swm_msm_g1(ctx: *mut swm_ctx, bases: *const swm_bases, offset: usize, scalars: *const u64, n: usize,
                      out_jac: *mut u64) -> c_int; // VariableBaseMSM::multi_scalar_mul
    pub fn swm_ntt_fr(ctx: *mut swm_ctx, data: *mut u64, log_n: c_uint, inverse: c_int, coset: c_int) -> c_int;
    pub fn swm_ntt_fr_sharded_dev(ctx: *mut swm_ctx, d_local: *mut c_void, log_n: c_uint, inverse: c_int, blocks_in: c_int) -> c_int;
    pub fn swm_spmv_fr(ctx: *mut swm_ctx, rowptr: *const u32, col: *const u32, val: *const u64, z: *const u64,
                       z_len: usize, out: *mut u64, rows: usize, nnz: usize) -> c_int;
    pub fn swm_batch_inverse_fr(ctx: *mut swm_ctx, data: *mut u64, n: usize) -> c_int;

    // the native Pedersen hash and MerkleTree::new of src/merkle_tree/simple_merkle_tree.rs:47-49, src/hash/mod.rs:23-28
    pub fn swm_pedersen_create(ctx: *mut swm_ctx, generators_xy: *const u8, num_windows: usize, window_size: usize,
                               out: *mut *mut swm_pedersen) -> c_int;
    pub fn swm_pedersen_destroy(ctx: *mut swm_ctx, params: *mut swm_pedersen);
    pub fn swm_pedersen_hash(ctx: *mut swm_ctx, params: *const swm_pedersen, inputs: *const u8, input_len: usize, count: usize,
                             digests: *mut u8) -> c_int;
    pub fn swm_merkle_tree_build(ctx: *mut swm_ctx, leaf_params: *const swm_pedersen, two_to_one_params: *const swm_pedersen,
                                 leaves: *const u8, leaf_len: usize, n_leaves: usize, nodes: *mut u8) -> c_int;

    // the membership circuit's witness on the GPU: SimpleMerkleTree::prove (src/merkle_tree/simple_merkle_tree.rs:105-123) without
    // running the constraint synthesizer on the host (roots and siblings: 32 canonical LE bytes; witness: Montgomery limbs)
    pub fn swm_merkle_circuit_shape(height: usize, gadget_byte_ops: usize, num_instance: *mut usize, num_witness: *mut usize,
                                    num_constraints: *mut usize) -> c_int;
    pub fn swm_merkle_circuit_create(ctx: *mut swm_ctx, leaf_params: *const swm_pedersen, two_to_one_params: *const swm_pedersen,
                                     height: usize, gadget_byte_ops: usize, out: *mut *mut swm_merkle_circuit) -> c_int;
    pub fn swm_merkle_circuit_destroy(ctx: *mut swm_ctx, circuit: *mut swm_merkle_circuit);
    pub fn swm_merkle_witness(ctx: *mut swm_ctx, circuit: *const swm_merkle_circuit, leaves: *const u8, indices: *const u64,
                              siblings: *const u8, count: usize, witness: *mut u64, roots: *mut u8) -> c_int;
    pub fn swm_merkle_witness_dev(ctx: *mut swm_ctx, circuit: *const swm_merkle_circuit, d_leaves: *const c_void,
                                  d_indices: *const c_void, d_siblings: *const c_void, count: usize, d_witness: *mut c_void,
                                  d_roots: *mut c_void, d_status: *mut c_void) -> c_int;
    pub fn swm_merkle_prove(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_merkle_circuit, root: *const u8, leaf: u8,
                            index: u64, siblings: *const u8, rng: *mut swm_rng, flags: c_uint, proof_out: *mut u8, cap: usize,
                            len: *mut usize) -> c_int;

    // the account tree of examples/simple-payments resident on the GPU: MerkleTree::blank / new, batched tree.update, tree.root,
    // tree.generate_proof and Path::verify (ledger.rs:106-173, transaction.rs:163-173); `height` counts the leaf level; digests and
    // siblings: 32 canonical LE bytes; update indices are host memory in both forms
    pub fn swm_merkle_tree_create_blank(ctx: *mut swm_ctx, leaf_params: *const swm_pedersen, two_to_one_params: *const swm_pedersen,
                                        height: usize, leaf_len: usize, out: *mut *mut swm_merkle_tree) -> c_int;
    pub fn swm_merkle_tree_create_from_leaves(ctx: *mut swm_ctx, leaf_params: *const swm_pedersen, two_to_one_params: *const swm_pedersen,
                                              leaves: *const u8, leaf_len: usize, n_leaves: usize, out: *mut *mut swm_merkle_tree) -> c_int;
    pub fn swm_merkle_tree_create_from_leaves_dev(ctx: *mut swm_ctx, leaf_params: *const swm_pedersen,
                                                  two_to_one_params: *const swm_pedersen, d_leaves: *const c_void, leaf_len: usize,
                                                  n_leaves: usize, out: *mut *mut swm_merkle_tree) -> c_int;
    pub fn swm_merkle_tree_destroy(ctx: *mut swm_ctx, tree: *mut swm_merkle_tree);
    pub fn swm_merkle_tree_update(ctx: *mut swm_ctx, tree: *mut swm_merkle_tree, indices: *const u64, leaves: *const u8, leaf_len: usize,
                                  count: usize) -> c_int;
    pub fn swm_merkle_tree_update_dev(ctx: *mut swm_ctx, tree: *mut swm_merkle_tree, indices: *const u64, d_leaves: *const c_void,
                                      leaf_len: usize, count: usize) -> c_int;
    pub fn swm_merkle_tree_root(ctx: *mut swm_ctx, tree: *const swm_merkle_tree, root: *mut u8) -> c_int;
    pub fn swm_merkle_tree_paths(ctx: *mut swm_ctx, tree: *const swm_merkle_tree, indices: *const u64, count: usize,
                                 siblings: *mut u8) -> c_int;
    pub fn swm_merkle_tree_paths_dev(ctx: *mut swm_ctx, tree: *const swm_merkle_tree, d_indices: *const c_void, count: usize,
                                     d_siblings: *mut c_void) -> c_int;
    pub fn swm_merkle_tree_nodes(ctx: *mut swm_ctx, tree: *const swm_merkle_tree, nodes: *mut u8) -> c_int;
    pub fn swm_merkle_tree_dev_nodes(tree: *const swm_merkle_tree, d_nodes: *mut *mut c_void, n_nodes: *mut usize) -> c_int;
    pub fn swm_merkle_verify_paths(ctx: *mut swm_ctx, leaf_params: *const swm_pedersen, two_to_one_params: *const swm_pedersen,
                                   height: usize, roots: *const u8, root_stride: usize, leaves: *const u8, leaf_len: usize,
                                   indices: *const u64, siblings: *const u8, count: usize, ok: *mut u8, status: *mut u32) -> c_int;
    pub fn swm_merkle_verify_paths_dev(ctx: *mut swm_ctx, leaf_params: *const swm_pedersen, two_to_one_params: *const swm_pedersen,
                                       height: usize, d_roots: *const c_void, root_stride: usize, d_leaves: *const c_void,
                                       leaf_len: usize, d_indices: *const c_void, d_siblings: *const c_void, count: usize,
                                       d_ok: *mut c_void, d_status: *mut c_void) -> c_int;

    // the native Schnorr scheme of src/schnorr_signature/schnorr.rs:57-160, batched (points: x || y, 32 LE bytes each; a signature:
    // prover_response || verifier_challenge; secrets and nonces are the caller's draws)
    pub fn swm_schnorr_create(ctx: *mut swm_ctx, generator_xy: *const u8, salt32_or_null: *const u8, out: *mut *mut swm_schnorr) -> c_int;
    pub fn swm_schnorr_destroy(ctx: *mut swm_ctx, params: *mut swm_schnorr);
    pub fn swm_schnorr_keygen(ctx: *mut swm_ctx, params: *const swm_schnorr, secret_keys: *const u8, count: usize,
                              public_keys_xy: *mut u8) -> c_int;
    pub fn swm_schnorr_sign(ctx: *mut swm_ctx, params: *const swm_schnorr, secret_keys: *const u8, public_keys_xy: *const u8,
                            nonces: *const u8, messages: *const u8, msg_len: usize, count: usize, signatures: *mut u8) -> c_int;
    pub fn swm_schnorr_verify(ctx: *mut swm_ctx, params: *const swm_schnorr, public_keys_xy: *const u8, messages: *const u8,
                              msg_len: usize, signatures: *const u8, count: usize, ok: *mut u8) -> c_int;
    pub fn swm_schnorr_commitments(ctx: *mut swm_ctx, params: *const swm_schnorr, public_keys_xy: *const u8, signatures: *const u8,
                                   count: usize, commitments_xy: *mut u8) -> c_int;

    // the Schnorr verification circuit's witness on the GPU: the proof of examples/simple-payments/transaction.rs:108-126 without
    // running the constraint synthesizer on the host (no public input; witness: Montgomery limbs; ok: one byte per signature)
    pub fn swm_schnorr_circuit_shape(msg_len: usize, salted: c_int, num_instance: *mut usize, num_witness: *mut usize,
                                     num_constraints: *mut usize) -> c_int;
    pub fn swm_schnorr_circuit_create(ctx: *mut swm_ctx, params: *const swm_schnorr, msg_len: usize,
                                      out: *mut *mut swm_schnorr_circuit) -> c_int;
    pub fn swm_schnorr_circuit_destroy(ctx: *mut swm_ctx, circuit: *mut swm_schnorr_circuit);
    pub fn swm_schnorr_witness(ctx: *mut swm_ctx, circuit: *const swm_schnorr_circuit, public_keys_xy: *const u8, messages: *const u8,
                               signatures: *const u8, count: usize, witness: *mut u64, ok: *mut u8) -> c_int;
    pub fn swm_schnorr_witness_dev(ctx: *mut swm_ctx, circuit: *const swm_schnorr_circuit, d_public_keys: *const c_void,
                                   d_messages: *const c_void, d_signatures: *const c_void, count: usize, d_witness: *mut c_void,
                                   d_ok: *mut c_void, d_status: *mut c_void) -> c_int;
    pub fn swm_schnorr_prove(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_schnorr_circuit, public_key_xy: *const u8,
                             message: *const u8, signature: *const u8, rng: *mut swm_rng, flags: c_uint, proof_out: *mut u8,
                             cap: usize, len: *mut usize) -> c_int;

    // the native Poseidon hash of src/hash/mod.rs:30-43 (PoseidonSponge<Fq>, rate 2), batched; a field element: 32 canonical LE bytes;
    // the parameters are the caller's (mds: 9 elements row-major, ark: (full + partial) x 3)
    pub fn swm_poseidon_create(ctx: *mut swm_ctx, full_rounds: usize, partial_rounds: usize, alpha: u64, mds: *const u8, ark: *const u8,
                               out: *mut *mut swm_poseidon) -> c_int;
    pub fn swm_poseidon_destroy(ctx: *mut swm_ctx, params: *mut swm_poseidon);
    pub fn swm_poseidon_hash_fr(ctx: *mut swm_ctx, params: *const swm_poseidon, elems: *const u8, n_in: usize, count: usize,
                                n_out: usize, out: *mut u8) -> c_int;
    pub fn swm_poseidon_hash_fr_dev(ctx: *mut swm_ctx, params: *const swm_poseidon, d_elems: *const c_void, n_in: usize, count: usize,
                                    n_out: usize, d_out: *mut c_void, d_status: *mut c_void) -> c_int;
    pub fn swm_poseidon_hash_bytes(ctx: *mut swm_ctx, params: *const swm_poseidon, inputs: *const u8, input_len: usize, count: usize,
                                   digests: *mut u8) -> c_int;
    pub fn swm_poseidon_hash_bytes_dev(ctx: *mut swm_ctx, params: *const swm_poseidon, d_inputs: *const c_void, input_len: usize,
                                       count: usize, d_digests: *mut c_void) -> c_int;
    pub fn swm_poseidon_pack_bytes(input: *const u8, len: usize, elems: *mut u8, cap_elems: usize, n_elems: *mut usize) -> c_int;

    // the Poseidon hash circuit's witness on the GPU (the gadget of src/gadgets/poseidon.rs:12-31 in this library's row layout): the
    // outputs are the public input; witness: Montgomery limbs; outputs: canonical LE bytes.  (Declarations only: nothing in this
    // crate is compiled or linked by the library's own build or tests.)
    pub fn swm_poseidon_circuit_shape(full_rounds: usize, partial_rounds: usize, alpha: u64, bytes_form: c_int, n_in: usize,
                                      n_out: usize, num_instance: *mut usize, num_witness: *mut usize,
                                      num_constraints: *mut usize) -> c_int;
    pub fn swm_poseidon_circuit_create(ctx: *mut swm_ctx, params: *const swm_poseidon, bytes_form: c_int, n_in: usize, n_out: usize,
                                       out: *mut *mut swm_poseidon_circuit) -> c_int;
    pub fn swm_poseidon_circuit_destroy(ctx: *mut swm_ctx, circuit: *mut swm_poseidon_circuit);
    pub fn swm_poseidon_witness(ctx: *mut swm_ctx, circuit: *const swm_poseidon_circuit, inputs: *const u8, count: usize,
                                witness: *mut u64, outputs: *mut u8) -> c_int;
    pub fn swm_poseidon_witness_dev(ctx: *mut swm_ctx, circuit: *const swm_poseidon_circuit, d_inputs: *const c_void, count: usize,
                                    d_witness: *mut c_void, d_outputs: *mut c_void, d_status: *mut c_void) -> c_int;
    pub fn swm_poseidon_prove(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_poseidon_circuit, input: *const u8,
                              rng: *mut swm_rng, flags: c_uint, outputs: *mut u8, proof_out: *mut u8, cap: usize,
                              len: *mut usize) -> c_int;
    // the resident Poseidon Merkle tree (leaf digest: the byte sponge; inner node: the two-to-one form) and the path check
    pub fn swm_poseidon_tree_create_blank(ctx: *mut swm_ctx, params: *const swm_poseidon, height: usize, leaf_len: usize,
                                          out: *mut *mut swm_poseidon_tree) -> c_int;
    pub fn swm_poseidon_tree_create_from_leaves(ctx: *mut swm_ctx, params: *const swm_poseidon, leaves: *const u8, leaf_len: usize,
                                                n_leaves: usize, out: *mut *mut swm_poseidon_tree) -> c_int;
    pub fn swm_poseidon_tree_destroy(ctx: *mut swm_ctx, tree: *mut swm_poseidon_tree);
    pub fn swm_poseidon_tree_update(ctx: *mut swm_ctx, tree: *mut swm_poseidon_tree, indices: *const u64, leaves: *const u8,
                                    leaf_len: usize, count: usize) -> c_int;
    pub fn swm_poseidon_tree_root(ctx: *mut swm_ctx, tree: *const swm_poseidon_tree, root: *mut u8) -> c_int;
    pub fn swm_poseidon_tree_paths(ctx: *mut swm_ctx, tree: *const swm_poseidon_tree, indices: *const u64, count: usize,
                                   siblings: *mut u8) -> c_int;
    pub fn swm_poseidon_tree_nodes(ctx: *mut swm_ctx, tree: *const swm_poseidon_tree, nodes: *mut u8) -> c_int;
    pub fn swm_poseidon_tree_dev_nodes(tree: *const swm_poseidon_tree, d_nodes: *mut *mut c_void, n_nodes: *mut usize) -> c_int;
    pub fn swm_poseidon_verify_paths(ctx: *mut swm_ctx, params: *const swm_poseidon, height: usize, roots: *const u8,
                                     root_stride: usize, leaves: *const u8, leaf_len: usize, indices: *const u64,
                                     siblings: *const u8, count: usize, ok: *mut u8, status: *mut u32) -> c_int;
    // the membership circuit over that tree: public input (root, leaf bits); witness: Montgomery limbs
    pub fn swm_poseidon_tree_circuit_shape(full_rounds: usize, partial_rounds: usize, alpha: u64, height: usize, leaf_len: usize,
                                           num_instance: *mut usize, num_witness: *mut usize, num_constraints: *mut usize) -> c_int;
    pub fn swm_poseidon_tree_circuit_create(ctx: *mut swm_ctx, params: *const swm_poseidon, height: usize, leaf_len: usize,
                                            out: *mut *mut swm_poseidon_tree_circuit) -> c_int;
    pub fn swm_poseidon_tree_circuit_destroy(ctx: *mut swm_ctx, circuit: *mut swm_poseidon_tree_circuit);
    pub fn swm_poseidon_tree_witness(ctx: *mut swm_ctx, circuit: *const swm_poseidon_tree_circuit, leaves: *const u8,
                                     indices: *const u64, siblings: *const u8, count: usize, witness: *mut u64,
                                     roots: *mut u8) -> c_int;
    pub fn swm_poseidon_tree_witness_at(ctx: *mut swm_ctx, circuit: *const swm_poseidon_tree_circuit, tree: *const swm_poseidon_tree,
                                        leaves: *const u8, indices: *const u64, count: usize, witness: *mut u64) -> c_int;
    pub fn swm_poseidon_tree_prove(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_poseidon_tree_circuit, root: *const u8,
                                   leaf: *const u8, index: u64, siblings: *const u8, rng: *mut swm_rng, flags: c_uint,
                                   proof_out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    pub fn swm_poseidon_tree_prove_at(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_poseidon_tree_circuit,
                                      tree: *const swm_poseidon_tree, leaf: *const u8, index: u64, rng: *mut swm_rng, flags: c_uint,
                                      proof_out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    // the payment circuit over a Poseidon account tree: witness on host and device buffers, proofs against a resident tree
    pub fn swm_payment_circuit_shape(full_rounds: usize, partial_rounds: usize, alpha: u64, height: usize, salted: c_int,
                                     num_instance: *mut usize, num_witness: *mut usize, num_constraints: *mut usize) -> c_int;
    pub fn swm_payment_circuit_create(ctx: *mut swm_ctx, schnorr: *const swm_schnorr, poseidon: *const swm_poseidon, height: usize,
                                      out: *mut *mut swm_payment_circuit) -> c_int;
    pub fn swm_payment_circuit_destroy(ctx: *mut swm_ctx, circuit: *mut swm_payment_circuit);
    pub fn swm_payment_witness(ctx: *mut swm_ctx, circuit: *const swm_payment_circuit, messages: *const u8, signatures: *const u8,
                               sender_leaves: *const u8, recipient_leaves: *const u8, sender_siblings: *const u8,
                               recipient_siblings: *const u8, count: usize, witness: *mut u64, flags: *mut u8,
                               sender_roots: *mut u8, recipient_roots: *mut u8) -> c_int;
    pub fn swm_payment_witness_at(ctx: *mut swm_ctx, circuit: *const swm_payment_circuit, tree: *const swm_poseidon_tree,
                                  messages: *const u8, signatures: *const u8, sender_leaves: *const u8, recipient_leaves: *const u8,
                                  count: usize, witness: *mut u64, flags: *mut u8) -> c_int;
    pub fn swm_payment_witness_dev(ctx: *mut swm_ctx, circuit: *const swm_payment_circuit, tree: *const swm_poseidon_tree,
                                   d_messages: *const c_void, d_signatures: *const c_void, d_sender_leaves: *const c_void,
                                   d_recipient_leaves: *const c_void, d_sender_siblings: *const c_void,
                                   d_recipient_siblings: *const c_void, count: usize, d_witness: *mut c_void, d_flags: *mut c_void,
                                   d_status: *mut c_void, d_sender_roots: *mut c_void, d_recipient_roots: *mut c_void) -> c_int;
    pub fn swm_payment_prove_at(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_payment_circuit, tree: *const swm_poseidon_tree,
                                message: *const u8, signature: *const u8, sender_leaf: *const u8, recipient_leaf: *const u8,
                                rng: *mut swm_rng, flags: c_uint, proof_out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    pub fn swm_payment_prove_many_at(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_payment_circuit,
                                     tree: *const swm_poseidon_tree, messages: *const u8, signatures: *const u8,
                                     sender_leaves: *const u8, recipient_leaves: *const u8, count: usize, rng: *mut swm_rng,
                                     flags: c_uint, proofs_out: *mut u8, proof_cap: usize, lens: *mut usize,
                                     item_flags: *mut u8) -> c_int;
    // the payment circuit over a Pedersen account tree (swm_merkle_tree): the same entries
    pub fn swm_pedersen_payment_circuit_shape(height: usize, salted: c_int, num_instance: *mut usize, num_witness: *mut usize,
                                              num_constraints: *mut usize) -> c_int;
    pub fn swm_pedersen_payment_circuit_create(ctx: *mut swm_ctx, schnorr: *const swm_schnorr, leaf_params: *const swm_pedersen,
                                               two_to_one_params: *const swm_pedersen, height: usize,
                                               out: *mut *mut swm_pedersen_payment_circuit) -> c_int;
    pub fn swm_pedersen_payment_circuit_destroy(ctx: *mut swm_ctx, circuit: *mut swm_pedersen_payment_circuit);
    pub fn swm_pedersen_payment_witness(ctx: *mut swm_ctx, circuit: *const swm_pedersen_payment_circuit, messages: *const u8,
                                        signatures: *const u8, sender_leaves: *const u8, sender_siblings: *const u8,
                                        recipient_leaves: *const u8, recipient_siblings: *const u8, count: usize, witness: *mut u64,
                                        flags: *mut u8, sender_roots: *mut u8, recipient_roots: *mut u8) -> c_int;
    pub fn swm_pedersen_payment_witness_at(ctx: *mut swm_ctx, circuit: *const swm_pedersen_payment_circuit, tree: *const swm_merkle_tree,
                                           messages: *const u8, signatures: *const u8, sender_leaves: *const u8,
                                           recipient_leaves: *const u8, count: usize, witness: *mut u64, flags: *mut u8) -> c_int;
    pub fn swm_pedersen_payment_witness_dev(ctx: *mut swm_ctx, circuit: *const swm_pedersen_payment_circuit, tree: *const swm_merkle_tree,
                                            d_messages: *const c_void, d_signatures: *const c_void, d_sender_leaves: *const c_void,
                                            d_recipient_leaves: *const c_void, d_sender_siblings: *const c_void,
                                            d_recipient_siblings: *const c_void, count: usize, d_witness: *mut c_void,
                                            d_flags: *mut c_void, d_status: *mut c_void, d_sender_roots: *mut c_void,
                                            d_recipient_roots: *mut c_void) -> c_int;
    pub fn swm_pedersen_payment_prove_at(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_pedersen_payment_circuit,
                                         tree: *const swm_merkle_tree, message: *const u8, signature: *const u8, sender_leaf: *const u8,
                                         recipient_leaf: *const u8, rng: *mut swm_rng, flags: c_uint, proof_out: *mut u8, cap: usize,
                                         len: *mut usize) -> c_int;
    pub fn swm_pedersen_payment_prove_many_at(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_pedersen_payment_circuit,
                                              tree: *const swm_merkle_tree, messages: *const u8, signatures: *const u8,
                                              sender_leaves: *const u8, recipient_leaves: *const u8, count: usize, rng: *mut swm_rng,
                                              flags: c_uint, proofs_out: *mut u8, proof_cap: usize, lens: *mut usize,
                                              item_flags: *mut u8) -> c_int;
    // the transfer circuit over a Pedersen account tree: a block of transfers applied in order to a resident swm_merkle_tree
    pub fn swm_pedersen_transfer_circuit_shape(height: usize, salted: c_int, num_instance: *mut usize, num_witness: *mut usize,
                                               num_constraints: *mut usize) -> c_int;
    pub fn swm_pedersen_transfer_circuit_create(ctx: *mut swm_ctx, schnorr: *const swm_schnorr, leaf_params: *const swm_pedersen,
                                                two_to_one_params: *const swm_pedersen, height: usize,
                                                out: *mut *mut swm_pedersen_transfer_circuit) -> c_int;
    pub fn swm_pedersen_transfer_circuit_destroy(ctx: *mut swm_ctx, circuit: *mut swm_pedersen_transfer_circuit);
    pub fn swm_pedersen_transfer_witness_at(ctx: *mut swm_ctx, circuit: *const swm_pedersen_transfer_circuit, tree: *mut swm_merkle_tree,
                                            accounts_inout: *mut u8, messages: *const u8, signatures: *const u8, count: usize,
                                            witnesses_out: *mut u64, old_roots: *mut u8, new_roots: *mut u8, flags: *mut u8,
                                            status: *mut u32) -> c_int;
    pub fn swm_pedersen_transfer_prove_many_at(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_pedersen_transfer_circuit,
                                               tree: *mut swm_merkle_tree, accounts_inout: *mut u8, messages: *const u8,
                                               signatures: *const u8, count: usize, rng: *mut swm_rng, prove_flags: c_uint,
                                               proofs_out: *mut u8, proof_cap: usize, lens: *mut usize, old_roots: *mut u8,
                                               new_roots: *mut u8, flags: *mut u8, status: *mut u32) -> c_int;
    pub fn swm_pedersen_transfer_prove_at(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_pedersen_transfer_circuit,
                                          tree: *mut swm_merkle_tree, accounts_inout: *mut u8, message: *const u8, signature: *const u8,
                                          rng: *mut swm_rng, prove_flags: c_uint, proof_out: *mut u8, cap: usize, len: *mut usize,
                                          old_root: *mut u8, new_root: *mut u8, flag: *mut u8, status: *mut u32) -> c_int;
    // the rollup: ONE vector and ONE proof for a block of 1 .. 64 transfers over either tree, all or nothing (a transfer circuit and a count)
    pub fn swm_rollup_circuit_shape(full_rounds: usize, partial_rounds: usize, alpha: u64, height: usize, salted: c_int, n: usize,
                                    num_instance: *mut usize, num_witness: *mut usize, num_constraints: *mut usize) -> c_int;
    pub fn swm_pedersen_rollup_circuit_shape(height: usize, salted: c_int, n: usize, num_instance: *mut usize, num_witness: *mut usize,
                                             num_constraints: *mut usize) -> c_int;
    pub fn swm_rollup_witness_at(ctx: *mut swm_ctx, circuit: *const swm_transfer_circuit, tree: *mut swm_poseidon_tree,
                                 accounts_inout: *mut u8, messages: *const u8, signatures: *const u8, count: usize, witness_out: *mut u64,
                                 old_root: *mut u8, new_root: *mut u8, flags: *mut u8, status: *mut u32, applied: *mut c_int) -> c_int;
    pub fn swm_rollup_prove_at(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_transfer_circuit, tree: *mut swm_poseidon_tree,
                               accounts_inout: *mut u8, messages: *const u8, signatures: *const u8, count: usize, rng: *mut swm_rng,
                               prove_flags: c_uint, proof_out: *mut u8, cap: usize, len: *mut usize, old_root: *mut u8,
                               new_root: *mut u8, flags: *mut u8, status: *mut u32, applied: *mut c_int) -> c_int;
    pub fn swm_pedersen_rollup_witness_at(ctx: *mut swm_ctx, circuit: *const swm_pedersen_transfer_circuit, tree: *mut swm_merkle_tree,
                                          accounts_inout: *mut u8, messages: *const u8, signatures: *const u8, count: usize,
                                          witness_out: *mut u64, old_root: *mut u8, new_root: *mut u8, flags: *mut u8, status: *mut u32,
                                          applied: *mut c_int) -> c_int;
    pub fn swm_pedersen_rollup_prove_at(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_pedersen_transfer_circuit,
                                        tree: *mut swm_merkle_tree, accounts_inout: *mut u8, messages: *const u8, signatures: *const u8,
                                        count: usize, rng: *mut swm_rng, prove_flags: c_uint, proof_out: *mut u8, cap: usize,
                                        len: *mut usize, old_root: *mut u8, new_root: *mut u8, flags: *mut u8, status: *mut u32,
                                        applied: *mut c_int) -> c_int;
    // the transfer circuit: a block of transfers applied in order, the resident tree and the account table advanced on the GPU
    pub fn swm_transfer_circuit_shape(full_rounds: usize, partial_rounds: usize, alpha: u64, height: usize, salted: c_int,
                                      num_instance: *mut usize, num_witness: *mut usize, num_constraints: *mut usize) -> c_int;
    pub fn swm_transfer_circuit_create(ctx: *mut swm_ctx, schnorr: *const swm_schnorr, poseidon: *const swm_poseidon, height: usize,
                                       out: *mut *mut swm_transfer_circuit) -> c_int;
    pub fn swm_transfer_circuit_destroy(ctx: *mut swm_ctx, circuit: *mut swm_transfer_circuit);
    pub fn swm_transfer_witness_at(ctx: *mut swm_ctx, circuit: *const swm_transfer_circuit, tree: *mut swm_poseidon_tree,
                                   accounts_inout: *mut u8, messages: *const u8, signatures: *const u8, count: usize,
                                   witnesses_out: *mut u64, old_roots: *mut u8, new_roots: *mut u8, flags: *mut u8,
                                   status: *mut u32) -> c_int;
    pub fn swm_transfer_prove_many_at(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_transfer_circuit,
                                      tree: *mut swm_poseidon_tree, accounts_inout: *mut u8, messages: *const u8,
                                      signatures: *const u8, count: usize, rng: *mut swm_rng, prove_flags: c_uint,
                                      proofs_out: *mut u8, proof_cap: usize, lens: *mut usize, old_roots: *mut u8,
                                      new_roots: *mut u8, flags: *mut u8, status: *mut u32) -> c_int;
    pub fn swm_transfer_prove_at(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_transfer_circuit,
                                 tree: *mut swm_poseidon_tree, accounts_inout: *mut u8, message: *const u8, signature: *const u8,
                                 rng: *mut swm_rng, prove_flags: c_uint, proof_out: *mut u8, cap: usize, len: *mut usize,
                                 old_root: *mut u8, new_root: *mut u8, flag: *mut u8, status: *mut u32) -> c_int;
    // the account-update circuit: register and update_balance over the Poseidon account tree, a block applied in order
    pub fn swm_account_update_circuit_shape(full_rounds: usize, partial_rounds: usize, alpha: u64, height: usize,
                                            num_instance: *mut usize, num_witness: *mut usize, num_constraints: *mut usize) -> c_int;
    pub fn swm_account_update_circuit_create(ctx: *mut swm_ctx, poseidon: *const swm_poseidon, height: usize,
                                             out: *mut *mut swm_account_update_circuit) -> c_int;
    pub fn swm_account_update_circuit_destroy(ctx: *mut swm_ctx, circuit: *mut swm_account_update_circuit);
    pub fn swm_account_update_witness_at(ctx: *mut swm_ctx, circuit: *const swm_account_update_circuit, tree: *mut swm_poseidon_tree,
                                         accounts_inout: *mut u8, ids: *const u8, kinds: *const u8, keys_xy: *const u8,
                                         balances: *const u8, count: usize, witnesses_out: *mut u64, old_roots: *mut u8,
                                         new_roots: *mut u8, flags: *mut u8, status: *mut u32) -> c_int;
    pub fn swm_account_update_prove_many_at(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_account_update_circuit,
                                            tree: *mut swm_poseidon_tree, accounts_inout: *mut u8, ids: *const u8, kinds: *const u8,
                                            keys_xy: *const u8, balances: *const u8, count: usize, rng: *mut swm_rng,
                                            prove_flags: c_uint, proofs_out: *mut u8, proof_cap: usize, lens: *mut usize,
                                            old_roots: *mut u8, new_roots: *mut u8, flags: *mut u8, status: *mut u32) -> c_int;
    pub fn swm_account_update_prove_at(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_account_update_circuit,
                                       tree: *mut swm_poseidon_tree, accounts_inout: *mut u8, id: u8, kind: u8, key_xy: *const u8,
                                       balance: u64, rng: *mut swm_rng, prove_flags: c_uint, proof_out: *mut u8, cap: usize,
                                       len: *mut usize, old_root: *mut u8, new_root: *mut u8, flag: *mut u8, status: *mut u32) -> c_int;
    // the same over the reference's Pedersen account tree (a swm_merkle_tree with 72-byte leaves)
    pub fn swm_pedersen_account_update_circuit_shape(height: usize, num_instance: *mut usize, num_witness: *mut usize,
                                                     num_constraints: *mut usize) -> c_int;
    pub fn swm_pedersen_account_update_circuit_create(ctx: *mut swm_ctx, leaf: *const swm_pedersen, two_to_one: *const swm_pedersen,
                                                      height: usize, out: *mut *mut swm_pedersen_account_update_circuit) -> c_int;
    pub fn swm_pedersen_account_update_circuit_destroy(ctx: *mut swm_ctx, circuit: *mut swm_pedersen_account_update_circuit);
    pub fn swm_pedersen_account_update_witness_at(ctx: *mut swm_ctx, circuit: *const swm_pedersen_account_update_circuit,
                                                  tree: *mut swm_merkle_tree, accounts_inout: *mut u8, ids: *const u8, kinds: *const u8,
                                                  keys_xy: *const u8, balances: *const u8, count: usize, witnesses_out: *mut u64,
                                                  old_roots: *mut u8, new_roots: *mut u8, flags: *mut u8, status: *mut u32) -> c_int;
    pub fn swm_pedersen_account_update_prove_many_at(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_pedersen_account_update_circuit,
                                                     tree: *mut swm_merkle_tree, accounts_inout: *mut u8, ids: *const u8, kinds: *const u8,
                                                     keys_xy: *const u8, balances: *const u8, count: usize, rng: *mut swm_rng,
                                                     prove_flags: c_uint, proofs_out: *mut u8, proof_cap: usize, lens: *mut usize,
                                                     old_roots: *mut u8, new_roots: *mut u8, flags: *mut u8, status: *mut u32) -> c_int;
    pub fn swm_pedersen_account_update_prove_at(ctx: *mut swm_ctx, pk: *const swm_pk, circuit: *const swm_pedersen_account_update_circuit,
                                                tree: *mut swm_merkle_tree, accounts_inout: *mut u8, id: u8, kind: u8, key_xy: *const u8,
                                                balance: u64, rng: *mut swm_rng, prove_flags: c_uint, proof_out: *mut u8, cap: usize,
                                                len: *mut usize, old_root: *mut u8, new_root: *mut u8, flag: *mut u8,
                                                status: *mut u32) -> c_int;
    // the Blake2s random oracle, batched, and its circuit's witness (no handle: the shape follows from input_len)
    pub fn swm_blake2s_hash(ctx: *mut swm_ctx, inputs: *const u8, input_len: usize, count: usize, digests: *mut u8) -> c_int;
    pub fn swm_blake2s_hash_dev(ctx: *mut swm_ctx, d_inputs: *const c_void, input_len: usize, count: usize,
                                d_digests: *mut c_void) -> c_int;
    pub fn swm_blake2s_circuit_shape(input_len: usize, num_instance: *mut usize, num_witness: *mut usize,
                                     num_constraints: *mut usize) -> c_int;
    pub fn swm_blake2s_witness(ctx: *mut swm_ctx, inputs: *const u8, input_len: usize, count: usize, witness: *mut u64,
                               digests: *mut u8) -> c_int;
    pub fn swm_blake2s_witness_dev(ctx: *mut swm_ctx, d_inputs: *const c_void, input_len: usize, count: usize,
                                   d_witness: *mut c_void, d_digests: *mut c_void) -> c_int;
    pub fn swm_blake2s_prove(ctx: *mut swm_ctx, pk: *const swm_pk, input: *const u8, input_len: usize, rng: *mut swm_rng,
                             flags: c_uint, digest_out: *mut u8, proof_out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    // integer programs: a tape of typed gadget ops as one circuit, its witnesses synthesised on the GPU (program_shape.h)
    pub fn swm_program_circuit_shape(tape: *const u8, len: usize, num_instance: *mut usize, num_witness: *mut usize,
                                     num_constraints: *mut usize) -> c_int;
    pub fn swm_program_create(ctx: *mut swm_ctx, tape: *const u8, len: usize, out: *mut *mut swm_program) -> c_int;
    pub fn swm_program_destroy(ctx: *mut swm_ctx, program: *mut swm_program);
    pub fn swm_program_witness(ctx: *mut swm_ctx, program: *const swm_program, inputs: *const u8, count: usize, witness: *mut u64,
                               outputs: *mut u8, status: *mut u8) -> c_int;
    pub fn swm_program_witness_dev(ctx: *mut swm_ctx, program: *const swm_program, d_inputs: *const c_void, count: usize,
                                   d_witness: *mut c_void, d_outputs: *mut c_void, d_status: *mut c_void) -> c_int;
    pub fn swm_program_prove(ctx: *mut swm_ctx, pk: *const swm_pk, program: *const swm_program, input: *const u8, rng: *mut swm_rng,
                             flags: c_uint, output: *mut u8, status_out: *mut u8, proof_out: *mut u8, cap: usize,
                             len: *mut usize) -> c_int;
    pub fn swm_program_prove_many(ctx: *mut swm_ctx, pk: *const swm_pk, program: *const swm_program, inputs: *const u8, count: usize,
                                  rng: *mut swm_rng, flags: c_uint, outputs: *mut u8, status: *mut u8, proofs_out: *mut u8,
                                  proof_cap: usize, lens: *mut usize) -> c_int;
}

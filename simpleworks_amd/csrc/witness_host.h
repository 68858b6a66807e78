// witness_host.h — the host driver every circuit unit (csrc/*_witness.hip) shares: how many items go through the device at a
// time, what an error leaves behind, the call of the prover over a witness that is already on the device, and the end of a
// circuit handle.  A unit writes its kernels, its *_run launcher, its staging layout and its instance vector; the rest is here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "context.h"
#include "ff.cuh"
#include "host/witness_chunks.h"
#include "swmarlin.h"

namespace swm {

inline int drained(swm_ctx* ctx, int rc) {  // an error leaves nothing of this call queued behind it
    if (rc != SWM_OK) drain_streams(ctx);
    return rc;
}

// Items of `item_bytes` witness bytes per chunk under the context's cap (host/witness_chunks.h); 0: item_bytes = 0.
inline size_t witness_stage_items(const swm_ctx* ctx, size_t item_bytes) { return witness_chunk_items(item_bytes, ctx->witness_stage_bytes); }

// The prover over one item's witnesses at d_w (num_witness elements on the context's device), `inst` its num_instance public
// inputs in Montgomery form.  The only place that sets swm_ctx::witness_dev, and it is null again on every way out: a stale
// device witness never reaches the next proof.
inline int prove_device_witness(swm_ctx* ctx, const swm_pk* pk, size_t num_instance, size_t num_witness, size_t num_constraints, const Fr* inst,
                                const Fr* d_w, swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len) {
    swm_r1cs cs = {};
    cs.num_instance = num_instance;
    cs.num_witness = num_witness;
    cs.num_constraints = num_constraints;
    cs.instance = reinterpret_cast<const uint64_t*>(inst);
    cs.witness = reinterpret_cast<const uint64_t*>(d_w);  // never read on the host: the context carries the device source
    struct DevWitnessScope {
        swm_ctx* c;
        ~DevWitnessScope() { c->witness_dev = nullptr; }
    } scope{ctx};
    ctx->witness_dev = d_w;
    return swm_generate_proof_ex(ctx, pk, &cs, rng, flags, proof_out, cap, len);
}

// Whether the prover would take a system of these counts under `pk` (marlin_prove.hip: what prove_shape compares, SWM_ERR_MISMATCH
// otherwise).  For a unit that changes state before it proves: it asks first.
bool pk_takes_shape(const swm_pk* pk, size_t num_instance, size_t num_witness, size_t num_constraints);

// The end of a circuit handle: nothing queued on the context still reads it.  free_device: its device arrays, if it has any.
template <class T, class FreeDevice>
void destroy_circuit(swm_ctx* ctx, T* c, FreeDevice free_device) {
    if (!c) return;
    DeviceGuard guard(ctx);
    if (ctx) drain_streams(ctx);
    free_device(c);
    delete c;
}
template <class T>
void destroy_circuit(swm_ctx* ctx, T* c) {
    destroy_circuit(ctx, c, [](T*) {});
}

}  // namespace swm

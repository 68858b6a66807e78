// poseidon_witness.hip — the witness of the Poseidon hash circuit, synthesised on the GPU: the step between an input of the sponge
// (poseidon.hip) and the proof of its digest (marlin.hip).
//
// What the reference does there: gadgets::poseidon2_hash (src/gadgets/poseidon.rs:12-31) runs PoseidonSpongeVar over a fresh
// constraint system — the whole synthesizer, on one CPU thread, per proof.  The prover reads only the ASSIGNMENT and the circuit's
// shape depends on the parameter shape, the form and the lengths alone, so what is left per proof is the witness vector.  Its
// order and values are those of simpleworks_amd/workloads.py, build_poseidon_hash: that function is the specification,
// host/poseidon_shape.h the counts and offsets.  The digest is the public input (the reference's unit test publishes nothing).
//
// On the GPU.  The native kernel's structure: one lane per item, one wave per workgroup, the state in registers, the table of
// poseidon.h in LDS — the ~600 dependent products of a permutation have no parallelism inside one sponge.  The native kernel
// computes every value the circuit holds and throws it away; pw_permute is ps_permute of poseidon.hip with a store after every
// square and every product of an S-box.  The arithmetic and its bounds are those at the head of poseidon.hip, unchanged: recording
// reads values, it does not feed any back.
// Recording.  A chain value is a normalised fr29_mul result v 2^261 (< 2r, limbs < 2^29).  The prover wants v 2^256 mod r,
// canonical, as 8 words: ONE more product, by 2^256 mod r in standard form (a launch-uniform argument, canonical: < r), then
// fr29_canonical and fr29_pack.  Bound of that product: (< 2r) x (< r) = 2 r^2 < 2^261 r, the first operand normalised — inside
// fr29_mul's contract with room.  An absorbed element of the elements form is recorded the same way from its 2^261 form.
// Stores.  A chain value leaves as it is produced: 32 bytes per lane at a stride of num_witness x 32 bytes between lanes —
// uncoalesced, and small next to the products.  The bit section of the bytes form (8 n_in x 32 bytes per item, mostly zeros) is
// written in a second pass in which the wave walks its 64 items and the lanes walk the bits: contiguous stores.
// Every lane of a launch takes the same path: the round kind, the bits of alpha, the form and the lengths are launch-uniform.  The
// idle lanes of the last workgroup recompute the last item and store nothing.
// Measured on one MI355X (tools/poseidon_witness_time.py, profiles/poseidon_witness_time.txt): 1.6 - 1.7 x the native hash of the same
// inputs up to 2^14 items, 1.9 - 2.1 x at 2^16, where the 0.7 - 2 GB of witnesses are the difference.  ONE input of 65536 bytes is a
// serial chain of about 630 000 products (and 280 000 conversions) on one lane: 409 ms, measured once, against 294 ms for the native
// hash of it.  That is not tuned: the batch is what the GPU form is for.
// Elements form: an element >= r is found by a pass over the item's elements BEFORE anything is stored; such an item computes
// like the others (an element < 2^256 is a legal operand, as in the native kernel) and every store of it writes zeros.
#include <hip/hip_runtime.h>

#include <string.h>

#include <memory>

#include "context.h"
#include "ff.cuh"
#include "fr29.cuh"
#include "host/poseidon_shape.h"
#include "poseidon.h"
#include "poseidon_record.cuh"
#include "swmarlin.h"
#include "witness_host.h"

struct swm_poseidon_circuit {
    const swm_poseidon* params = nullptr;
    swm::PoseidonShape shape;
};

namespace swm {

// `count` witnesses.  The steps are poseidon_hash_kernel's; `out` (may be NULL): count x n_out x 8 words, canonical.
template <bool BYTES>
__global__ void __launch_bounds__(PS_LANES) poseidon_witness_kernel(const uint4* __restrict__ table, PwArgs A, const uint8_t* __restrict__ in,
                                                                    Fr* __restrict__ witness, uint32_t* __restrict__ out,
                                                                    uint32_t* __restrict__ status) {
    SWM_LIGHT_KERNEL();
    extern __shared__ __align__(16) uint32_t ps_tab[];
    for (unsigned i = threadIdx.x; i < A.rows * (PS_ROW / 4); i += PS_LANES) reinterpret_cast<uint4*>(ps_tab)[i] = table[i];
    __syncthreads();
    const size_t first = blockIdx.x * (size_t)PS_LANES, lane_item = first + threadIdx.x;
    const bool act = lane_item < A.count;
    const size_t item = act ? lane_item : A.count - 1;  // an idle lane reads the last item's input and stores nothing
    const int alpha_top = 31 - __clz((int)A.alpha);
    const Fr29 to_mont = ps_row(ps_tab, 0);
    Fr29 one;
#pragma unroll
    for (int i = 0; i < 9; i++) one.l[i] = i == 0 ? 1u : 0u;
    bool bad = false;
    if (!BYTES) {
#pragma unroll 1
        for (size_t e = 0; e < A.n_in; e++) (void)ps_fetch<false>(in, item, A.n_in, e, bad);
    }
    const uint32_t keep = bad ? 0u : 0xFFFFFFFFu;
    Fr* w = witness + item * A.num_witness;
    Fr* wp = w + A.sponge_at;
    Fr29 s0, s1, s2;
#pragma unroll
    for (int i = 0; i < 9; i++) s0.l[i] = s1.l[i] = s2.l[i] = 0;
    const size_t in_blocks = (A.n_elems + 1) / 2, out_blocks = (A.n_out + 1u) / 2;
    uint32_t* o = out ? out + 8 * item * A.n_out : nullptr;
#pragma unroll 1
    for (size_t step = 0; step < in_blocks + out_blocks; step++) {
        if (step > 0 || in_blocks == 0) pw_permute(ps_tab, A, alpha_top, s0, s1, s2, wp, act, keep);
        if (step < in_blocks) {
            bool ignored = false;
            const Fr29 e0 = fr29_mul_fenced(fr29_unpack(ps_fetch<BYTES>(in, item, A.n_in, 2 * step, ignored)), to_mont);
            s0 = fr29_add(s0, e0);
            if (!BYTES) pw_put(w + 2 * step, e0, A.to_std, act, keep);
            if (2 * step + 1 < A.n_elems) {
                const Fr29 e1 = fr29_mul_fenced(fr29_unpack(ps_fetch<BYTES>(in, item, A.n_in, 2 * step + 1, ignored)), to_mont);
                s1 = fr29_add(s1, e1);
                if (!BYTES) pw_put(w + 2 * step + 1, e1, A.to_std, act, keep);
            }
        } else {
            const unsigned j = 2 * (unsigned)(step - in_blocks);
            const Fr y0 = fr29_pack(fr29_canonical(fr29_mul_fenced(s0, one), true));
            if (o && act) {
#pragma unroll
                for (int q = 0; q < 8; q++) o[8 * j + q] = y0.v[q] & keep;
            }
            if (j + 1 < A.n_out) {
                const Fr y1 = fr29_pack(fr29_canonical(fr29_mul_fenced(s1, one), true));
                if (o && act) {
#pragma unroll
                    for (int q = 0; q < 8; q++) o[8 * (j + 1) + q] = y1.v[q] & keep;
                }
            }
        }
    }
    if (status && act) status[item] = bad ? 1u : 0u;  // (the bytes form refuses nothing: its items are all "computed", 0)
    if (BYTES) {
        // the bit section: the wave walks its items, the lanes walk the bits — lane l writes witness l, l + 64, ... of the item
        const Fr f_one = fp_one<Fr>();
        const unsigned nbits = 8u * (unsigned)A.n_in;  // <= 2^19
#pragma unroll 1
        for (unsigned q = 0; q < PS_LANES && first + q < A.count; q++) {
            const uint8_t* msg = in + (first + q) * A.n_in;
            uint4* wb = reinterpret_cast<uint4*>(witness + (first + q) * A.num_witness);
            for (unsigned idx = threadIdx.x; idx < nbits; idx += PS_LANES) {
                const uint32_t set = 0u - ((msg[idx >> 3] >> (idx & 7u)) & 1u);  // all ones for a set bit: one, else zero
                wb[2 * idx] = make_uint4(f_one.v[0] & set, f_one.v[1] & set, f_one.v[2] & set, f_one.v[3] & set);
                wb[2 * idx + 1] = make_uint4(f_one.v[4] & set, f_one.v[5] & set, f_one.v[6] & set, f_one.v[7] & set);
            }
        }
    }
}

// d_witness: count x num_witness elements, 16-byte aligned; d_out (may be NULL): count x n_out x 32 bytes; d_status (may be NULL)
static int poseidon_witness_run(swm_ctx* ctx, const swm_poseidon_circuit* c, const uint8_t* d_in, size_t count, Fr* d_witness, void* d_out,
                                void* d_status) {
    if (!count) return SWM_OK;
    if (count > 0x7FFFFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_witness: %zu items in one call", count);
    const PoseidonShape& s = c->shape;
    const swm_poseidon* p = c->params;
    PwArgs A;
    A.rows = (unsigned)p->rows;
    A.half_full = p->full_rounds / 2;
    A.partial = p->partial_rounds;
    A.alpha = p->alpha;
    A.chain = (unsigned)s.chain;
    A.n_out = (unsigned)s.n_out;
    A.n_in = s.n_in;
    A.n_elems = s.elems;
    A.count = count;
    A.num_witness = s.num_witness;
    A.sponge_at = s.sponge_at;
    pw_std_limbs(fp_one<Fr>(), &A.to_std);  // the words of Montgomery(1) ARE 2^256 mod r
    const size_t lds = p->rows * PS_ROW * sizeof(uint32_t);
    const dim3 grid((unsigned)((count + PS_LANES - 1) / PS_LANES));
    if (s.bytes)
        SWM_LAUNCH(ctx, "poseidon_witness_bytes", poseidon_witness_kernel<true>, grid, dim3(PS_LANES), lds,
                   reinterpret_cast<const uint4*>(p->d_table), A, d_in, d_witness, (uint32_t*)d_out, (uint32_t*)d_status);
    else
        SWM_LAUNCH(ctx, "poseidon_witness_fr", poseidon_witness_kernel<false>, grid, dim3(PS_LANES), lds,
                   reinterpret_cast<const uint4*>(p->d_table), A, d_in, d_witness, (uint32_t*)d_out, (uint32_t*)d_status);
    return SWM_OK;
}

static size_t pw_item_bytes(const PoseidonShape& s) { return s.bytes ? s.n_in : 32 * s.n_in; }

// the host forms' check: what the device form reports per item
static int pw_check_elements(swm_ctx* ctx, const char* what, const PoseidonShape& s, const uint8_t* inputs, size_t count) {
    if (s.bytes) return SWM_OK;
    Fr v;
    for (size_t i = 0; i < count * s.n_in; i++)
        if (!ps_load_std(inputs + 32 * i, &v))
            return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: item %zu: element %zu is not a canonical field element", what, i / s.n_in, i % s.n_in);
    return SWM_OK;
}

static int poseidon_witness_host(swm_ctx* ctx, const swm_poseidon_circuit* c, const uint8_t* inputs, size_t count, uint64_t* witness,
                                 uint8_t* outputs) {
    const PoseidonShape& s = c->shape;
    const size_t item = s.num_witness * sizeof(Fr), in_item = pw_item_bytes(s), out_item = 32 * s.n_out;
    for (const WitnessChunk ch : WitnessChunks(witness_stage_items(ctx, item), count)) {
        const size_t base = ch.base, n = ch.count;
        uint8_t *d_in = nullptr, *d_out = nullptr;
        SWM_TRY(scratch(ctx, "stage.a", n * in_item + 32, (void**)&d_in));
        SWM_TRY(scratch(ctx, "poseidon.w", n * item + n * out_item, (void**)&d_out));
        if (in_item) SWM_HIP(ctx, hipMemcpyAsync(d_in, inputs + base * in_item, n * in_item, hipMemcpyHostToDevice, ctx->stream));
        SWM_TRY(poseidon_witness_run(ctx, c, d_in, n, (Fr*)d_out, d_out + n * item, nullptr));
        SWM_HIP(ctx, hipMemcpyAsync(reinterpret_cast<uint8_t*>(witness) + base * item, d_out, n * item, hipMemcpyDeviceToHost, ctx->stream));
        if (outputs) SWM_HIP(ctx, hipMemcpyAsync(outputs + base * out_item, d_out + n * item, n * out_item, hipMemcpyDeviceToHost, ctx->stream));
        SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the staging buffers are reused by the next chunk
    }
    return SWM_OK;
}

// one witness into the scratch buffer "poseidon.w", its outputs to the host
static int poseidon_witness_one(swm_ctx* ctx, const swm_poseidon_circuit* c, const uint8_t* input, Fr** d_w, uint8_t* outputs) {
    const PoseidonShape& s = c->shape;
    const size_t item = s.num_witness * sizeof(Fr), in_item = pw_item_bytes(s);
    uint8_t *d_in = nullptr, *d_out = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", in_item + 32, (void**)&d_in));
    SWM_TRY(scratch(ctx, "poseidon.w", item + 32 * s.n_out, (void**)&d_out));
    if (in_item) SWM_HIP(ctx, hipMemcpyAsync(d_in, input, in_item, hipMemcpyHostToDevice, ctx->stream));
    SWM_TRY(poseidon_witness_run(ctx, c, d_in, 1, (Fr*)d_out, d_out + item, nullptr));
    SWM_HIP(ctx, hipMemcpyAsync(outputs, d_out + item, 32 * s.n_out, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *d_w = (Fr*)d_out;
    return SWM_OK;
}

}  // namespace swm

using namespace swm;

extern "C" {

int swm_poseidon_circuit_create(swm_ctx* ctx, const swm_poseidon* params, int bytes_form, size_t n_in, size_t n_out, swm_poseidon_circuit** out) {
    if (!ctx || !params || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_circuit_create: bad arguments");
    PoseidonShape shape;
    if (!poseidon_shape(params->full_rounds, params->partial_rounds, params->alpha, bytes_form != 0, n_in, n_out, &shape))
        return set_err(ctx, SWM_ERR_INVALID_ARG,
                       "poseidon_circuit_create: %zu %s in, %zu out (at most %zu bytes and one output, or %zu elements and 1 .. %zu outputs)", n_in,
                       bytes_form ? "bytes" : "elements", n_out, (size_t)PC_MAX_BYTES, (size_t)PC_MAX_IN, (size_t)PC_MAX_OUT);
    std::unique_ptr<swm_poseidon_circuit> c(new swm_poseidon_circuit);
    c->params = params;
    c->shape = shape;
    *out = c.release();
    return SWM_OK;
}

void swm_poseidon_circuit_destroy(swm_ctx* ctx, swm_poseidon_circuit* c) {
    destroy_circuit(ctx, c);
}

int swm_poseidon_witness_dev(swm_ctx* ctx, const swm_poseidon_circuit* c, const void* d_inputs, size_t count, void* d_witness, void* d_outputs,
                             void* d_status) {
    if (!ctx || !c || (count && (!d_witness || (c->shape.n_in && !d_inputs))))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_witness: bad arguments");
    if (((uintptr_t)d_witness & 15) || ((uintptr_t)d_outputs & 3) || ((uintptr_t)d_status & 3) || (!c->shape.bytes && ((uintptr_t)d_inputs & 3)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_witness: the witness must be 16-byte aligned, elements, outputs and status 4-byte aligned");
    SWM_ON_DEVICE(ctx);
    return drained(ctx, poseidon_witness_run(ctx, c, (const uint8_t*)d_inputs, count, (Fr*)d_witness, d_outputs, d_status));
}

int swm_poseidon_witness(swm_ctx* ctx, const swm_poseidon_circuit* c, const uint8_t* inputs, size_t count, uint64_t* witness, uint8_t* outputs) {
    if (!ctx || !c || (count && (!witness || (c->shape.n_in && !inputs))))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_witness: bad arguments");
    if (!count) return SWM_OK;
    if (count > 0x7FFFFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_witness: %zu items in one call", count);
    SWM_TRY(pw_check_elements(ctx, "poseidon_witness", c->shape, inputs, count));
    SWM_ON_DEVICE(ctx);
    return drained(ctx, poseidon_witness_host(ctx, c, inputs, count, witness, outputs));
}

int swm_poseidon_prove(swm_ctx* ctx, const swm_pk* pk, const swm_poseidon_circuit* c, const uint8_t* input, swm_rng* rng, unsigned flags,
                       uint8_t* outputs, uint8_t* proof_out, size_t cap, size_t* len) {
    if (!ctx || !pk || !c || !rng || !outputs || !proof_out || !len || (c->shape.n_in && !input))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_prove: bad arguments");
    const PoseidonShape& s = c->shape;
    SWM_TRY(pw_check_elements(ctx, "poseidon_prove", s, input, 1));
    Fr* d_w = nullptr;
    uint8_t digest[32 * PC_MAX_OUT];
    {
        SWM_ON_DEVICE(ctx);
        SWM_TRY(drained(ctx, poseidon_witness_one(ctx, c, input, &d_w, digest)));
    }
    // public input: one, then the outputs (in the prover's Montgomery form)
    Fr inst[1 + PC_MAX_OUT];
    inst[0] = fp_one<Fr>();
    for (size_t j = 0; j < s.n_out; j++) {
        Fr v;
        (void)ps_load_std(digest + 32 * j, &v);  // canonical: the kernel wrote it
        inst[1 + j] = fp_from_std(v);
    }
    memcpy(outputs, digest, 32 * s.n_out);
    return prove_device_witness(ctx, pk, s.num_instance, s.num_witness, s.num_constraints, inst, d_w, rng, flags, proof_out, cap, len);
}

}  // extern "C"

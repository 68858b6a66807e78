// blake2s_witness.hip — the witness of the Blake2s hash circuit, synthesised on the GPU: the step between a byte string
// (blake2s.hip) and the proof that its digest is the public one (marlin.hip).
//
// What the reference does there: examples/simple-payments/random_oracle/blake2s/constraints.rs runs evaluate_blake2s over the
// input's UInt8 variables into a fresh constraint system, on one CPU thread.  The prover reads only the ASSIGNMENT and the
// circuit's shape depends on the input length alone, so what is left per proof is the witness vector.  Its order and values are
// those of simpleworks_amd/workloads.py, build_blake2s_hash: that function is the specification, host/blake2s_shape.h the
// offsets and host/schnorr_shape.h the schedule of a block.
//
// On the GPU.  Every witness is the element 0 or the Montgomery form of 1: a block of one item is 21 472 x 32 B = 687 KB of
// stores against some 3 000 integer instructions of compression, so the kernel is a store stream.  One workgroup of 256 lanes per
// item.  Per block, 16 lanes fetch the message words (bh_message_word: items lie back to back and need not be word-aligned), one
// lane runs the compression on plain words and records every sum (with its carries) and every xor into LDS
// (sv_b2s_compress_record, as schnorr_witness.hip does), and all lanes write the block's witnesses IN STORAGE ORDER: 16 bytes
// per lane, two lanes per element, consecutive lanes on consecutive addresses — 4 KB per workgroup instruction, every 16-byte
// chunk of the item written exactly once.  Which recorded word and bit a witness is comes from bh_b2s_source, a dozen integer
// instructions per store.  Several workgroups share a CU, so one item's compression runs under the others' stores.
#include <hip/hip_runtime.h>

#include <string.h>

#include "context.h"
#include "ff.cuh"
#include "host/blake2s_shape.h"
#include "swmarlin.h"
#include "witness_host.h"

namespace swm {

static constexpr unsigned BW_LANES = 256;

struct BwShared {
    uint64_t rec[SV_BLOCK_WORDS];
    uint32_t m[16], h[8];
};

struct BwArgs {
    size_t input_len, count, num_witness, b2s_at;
    uint32_t blocks;
};

// Workgroup p = item p.  in: count x input_len bytes (4-byte aligned base); witness: count x num_witness elements as 16-byte
// chunks; digests (may be NULL): count x 8 words.
__global__ void __launch_bounds__(BW_LANES) blake2s_witness_kernel(BwArgs A, const uint32_t* __restrict__ in, uint4* __restrict__ witness,
                                                                   uint32_t* __restrict__ digests) {
    __shared__ BwShared sh;
    const unsigned tid = threadIdx.x;
    const size_t item = blockIdx.x;
    uint4* w = witness + item * 2 * A.num_witness;
    const Fr f_one = fp_one<Fr>();
    // chunk c = tid + 256 k is half c & 1 = tid & 1 of element c >> 1: a lane writes the same half of `one` every time
    const uint4 zero = make_uint4(0, 0, 0, 0);
    const uint4 mine = tid & 1u ? make_uint4(f_one.v[4], f_one.v[5], f_one.v[6], f_one.v[7]) : make_uint4(f_one.v[0], f_one.v[1], f_one.v[2], f_one.v[3]);
    const size_t total = A.count * A.input_len, at = item * A.input_len, end = at + A.input_len;

    // bits
    const uint8_t* msg = reinterpret_cast<const uint8_t*>(in) + at;
    for (size_t c = tid; c < 16 * A.input_len; c += BW_LANES) {
        const size_t e = c >> 1;
        w[c] = (msg[e >> 3] >> (e & 7)) & 1u ? mine : zero;
    }

    // b2s
    if (tid == 0) sv_b2s_init(sh.h);
    for (uint32_t blk = 0; blk < A.blocks; blk++) {
        if (tid < 16) sh.m[tid] = bh_message_word(in, total, at + 64 * (size_t)blk + 4 * tid, end);
        __syncthreads();
        if (tid == 0) {
            const bool last = blk + 1 == A.blocks;
            sv_b2s_compress_record(sh.h, sh.m, last ? (uint64_t)A.input_len : (uint64_t)64 * (blk + 1), last, sh.rec);
        }
        __syncthreads();
        uint4* bw = w + 2 * (A.b2s_at + SV_BLOCK_WITNESSES * (size_t)blk);
        for (uint32_t c = tid; c < 2 * (uint32_t)SV_BLOCK_WITNESSES; c += BW_LANES) {
            const BhSource s = bh_b2s_source(c >> 1);
            bw[c] = (sh.rec[s.word] >> s.bit) & 1u ? mine : zero;
        }
        __syncthreads();  // rec[] and m[] are rewritten by the next block
    }
    if (digests && tid < 8) digests[8 * item + tid] = sh.h[tid];
}

// d_witness: count x num_witness elements, 16-byte aligned; d_digests (may be NULL): count x 32 bytes, 4-byte aligned
static int blake2s_witness_run(swm_ctx* ctx, const Blake2sShape& s, const void* d_in, size_t count, void* d_witness, void* d_digests) {
    if (!count) return SWM_OK;
    if (count > 0x7FFFFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "blake2s_witness: %zu items in one call", count);
    BwArgs A;
    A.input_len = s.input_len;
    A.count = count;
    A.num_witness = s.num_witness;
    A.b2s_at = s.b2s_at;
    A.blocks = (uint32_t)s.blocks;
    SWM_LAUNCH(ctx, "blake2s_witness", blake2s_witness_kernel, dim3((unsigned)count), dim3(BW_LANES), 0, A, (const uint32_t*)d_in,
               (uint4*)d_witness, (uint32_t*)d_digests);
    return SWM_OK;
}

static int blake2s_shape_or_err(swm_ctx* ctx, const char* what, size_t input_len, Blake2sShape* s) {
    if (!blake2s_shape(input_len, s))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: input_len %zu (at most %zu)", what, input_len, (size_t)BH_MAX_INPUT_LEN);
    return SWM_OK;
}

static int blake2s_witness_host(swm_ctx* ctx, const Blake2sShape& s, const uint8_t* inputs, size_t count, uint64_t* witness, uint8_t* digests) {
    const size_t item = s.num_witness * sizeof(Fr), len = s.input_len;
    for (const WitnessChunk ch : WitnessChunks(witness_stage_items(ctx, item), count)) {
        const size_t base = ch.base, n = ch.count;
        uint8_t *d_in = nullptr, *d_out = nullptr;
        SWM_TRY(scratch(ctx, "stage.a", n * len + 32, (void**)&d_in));
        SWM_TRY(scratch(ctx, "blake2s.w", n * item + 32 * n, (void**)&d_out));
        if (len) SWM_HIP(ctx, hipMemcpyAsync(d_in, inputs + base * len, n * len, hipMemcpyHostToDevice, ctx->stream));
        SWM_TRY(blake2s_witness_run(ctx, s, d_in, n, d_out, d_out + n * item));
        SWM_HIP(ctx, hipMemcpyAsync(reinterpret_cast<uint8_t*>(witness) + base * item, d_out, n * item, hipMemcpyDeviceToHost, ctx->stream));
        if (digests) SWM_HIP(ctx, hipMemcpyAsync(digests + 32 * base, d_out + n * item, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
        SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the staging buffers are reused by the next chunk
    }
    return SWM_OK;
}

// one witness into the scratch buffer "blake2s.w", its digest to the host
static int blake2s_witness_one(swm_ctx* ctx, const Blake2sShape& s, const uint8_t* input, Fr** d_w, uint8_t digest[32]) {
    const size_t item = s.num_witness * sizeof(Fr);
    uint8_t *d_in = nullptr, *d_out = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", s.input_len + 32, (void**)&d_in));
    SWM_TRY(scratch(ctx, "blake2s.w", item + 32, (void**)&d_out));
    if (s.input_len) SWM_HIP(ctx, hipMemcpyAsync(d_in, input, s.input_len, hipMemcpyHostToDevice, ctx->stream));
    SWM_TRY(blake2s_witness_run(ctx, s, d_in, 1, d_out, d_out + item));
    SWM_HIP(ctx, hipMemcpyAsync(digest, d_out + item, 32, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *d_w = (Fr*)d_out;
    return SWM_OK;
}

// 16 digest bytes as a little-endian integer (< 2^128: canonical), in the prover's Montgomery form
static Fr bw_half(const uint8_t* b) {
    Fr v = fp_zero<Fr>();
    for (int i = 0; i < 4; i++) v.v[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
    return fp_from_std(v);
}

}  // namespace swm

using namespace swm;

extern "C" {

int swm_blake2s_witness_dev(swm_ctx* ctx, const void* d_inputs, size_t input_len, size_t count, void* d_witness, void* d_digests) {
    if (!ctx) return set_err(ctx, SWM_ERR_INVALID_ARG, "blake2s_witness: bad arguments");
    Blake2sShape s;
    SWM_TRY(blake2s_shape_or_err(ctx, "blake2s_witness", input_len, &s));
    if (count && (!d_witness || (input_len && !d_inputs))) return set_err(ctx, SWM_ERR_INVALID_ARG, "blake2s_witness: bad arguments");
    if (((uintptr_t)d_witness & 15) || ((uintptr_t)d_inputs & 3) || ((uintptr_t)d_digests & 3))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "blake2s_witness: the witness must be 16-byte aligned, inputs and digests 4-byte aligned");
    SWM_ON_DEVICE(ctx);
    return drained(ctx, blake2s_witness_run(ctx, s, d_inputs, count, d_witness, d_digests));
}

int swm_blake2s_witness(swm_ctx* ctx, const uint8_t* inputs, size_t input_len, size_t count, uint64_t* witness, uint8_t* digests) {
    if (!ctx) return set_err(ctx, SWM_ERR_INVALID_ARG, "blake2s_witness: bad arguments");
    Blake2sShape s;
    SWM_TRY(blake2s_shape_or_err(ctx, "blake2s_witness", input_len, &s));
    if (count && (!witness || (input_len && !inputs))) return set_err(ctx, SWM_ERR_INVALID_ARG, "blake2s_witness: bad arguments");
    if (!count) return SWM_OK;
    if (count > 0x7FFFFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "blake2s_witness: %zu items in one call", count);
    SWM_ON_DEVICE(ctx);
    return drained(ctx, blake2s_witness_host(ctx, s, inputs, count, witness, digests));
}

int swm_blake2s_prove(swm_ctx* ctx, const swm_pk* pk, const uint8_t* input, size_t input_len, swm_rng* rng, unsigned flags,
                      uint8_t digest_out[32], uint8_t* proof_out, size_t cap, size_t* len) {
    if (!ctx || !pk || !rng || !digest_out || !proof_out || !len || (input_len && !input))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "blake2s_prove: bad arguments");
    Blake2sShape s;
    SWM_TRY(blake2s_shape_or_err(ctx, "blake2s_prove", input_len, &s));
    Fr* d_w = nullptr;
    uint8_t digest[32];
    {
        SWM_ON_DEVICE(ctx);
        SWM_TRY(drained(ctx, blake2s_witness_one(ctx, s, input, &d_w, digest)));
    }
    const Fr inst[3] = {fp_one<Fr>(), bw_half(digest), bw_half(digest + 16)};  // one, lo, hi
    memcpy(digest_out, digest, 32);
    return prove_device_witness(ctx, pk, s.num_instance, s.num_witness, s.num_constraints, inst, d_w, rng, flags, proof_out, cap, len);
}

}  // extern "C"

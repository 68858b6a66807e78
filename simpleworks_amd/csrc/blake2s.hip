// blake2s.hip — the reference's random oracle, batched: unkeyed BLAKE2s-256 (RFC 7693) of `count` byte strings of one length,
// one lane per string.
//
// What the reference does there (src/schnorr_signature/blake2s.rs and examples/simple-payments/random_oracle/blake2s/mod.rs,
// one call per input):
//   RO::setup      no parameters: ()
//   RO::evaluate   Blake2s::new(); update(input); finalize() -> [u8; 32]
//
// On the GPU.  The state (8 words), the working vector (16) and the message block (16) sit in registers; the compression is
// b2s.cuh's, shared with schnorr.hip.  The blocks of an item are streamed: every block but the last is compressed with
// t = 64 (b + 1), the last with t = input_len and the finalisation flag, its bytes past the end of the item zero.  The empty
// string is one block of zeros with t = 0.  The items lie back to back, item i at byte i input_len, which is word-aligned only
// when input_len is a multiple of 4: bh_message_word (host/blake2s_shape.h) reads aligned words and cuts an unaligned message
// word out of two of them, masks the item's last word, and touches no byte past the end of the buffer.
#include <hip/hip_runtime.h>

#include "b2s.cuh"
#include "context.h"
#include "host/blake2s_shape.h"
#include "swmarlin.h"

namespace swm {

// in: count x input_len bytes, 4-byte aligned base; out: count x 8 words
__global__ void __launch_bounds__(256) blake2s_hash_kernel(const uint32_t* __restrict__ in, size_t input_len, size_t count,
                                                           uint32_t* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= count) return;
    const size_t total = count * input_len, at = i * input_len, end = at + input_len;
    const size_t nblocks = b2s_blocks(input_len);
    uint32_t h[8];
    b2s_init(h);
#pragma unroll 1
    for (size_t b = 0; b < nblocks; b++) {
        uint32_t m[16];
#pragma unroll
        for (int j = 0; j < 16; j++) m[j] = bh_message_word(in, total, at + 64 * b + 4 * j, end);
        const bool last = b + 1 == nblocks;
        b2s_compress(h, m, last ? (uint64_t)input_len : (uint64_t)64 * (b + 1), last);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) out[8 * i + j] = h[j];
}

static int blake2s_hash_run(swm_ctx* ctx, const void* d_in, size_t input_len, size_t count, void* d_out) {
    if (!count) return SWM_OK;
    SWM_LAUNCH(ctx, "blake2s_hash", blake2s_hash_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (const uint32_t*)d_in, input_len,
               count, (uint32_t*)d_out);
    return SWM_OK;
}

// what both forms refuse; `inputs` may be NULL when there is nothing to read
static int blake2s_hash_check(swm_ctx* ctx, const void* inputs, size_t input_len, size_t count, const void* digests) {
    if (!ctx) return set_err(ctx, SWM_ERR_INVALID_ARG, "blake2s_hash: bad arguments");
    if (input_len > (size_t)BH_MAX_INPUT_LEN)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "blake2s_hash: input_len %zu (at most %zu)", input_len, (size_t)BH_MAX_INPUT_LEN);
    if (!digests) return set_err(ctx, SWM_ERR_INVALID_ARG, "blake2s_hash: NULL output");
    if (count && input_len && !inputs) return set_err(ctx, SWM_ERR_INVALID_ARG, "blake2s_hash: NULL input");
    if (count > 0x7FFFFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "blake2s_hash: %zu items in one call", count);
    return SWM_OK;
}

}  // namespace swm

using namespace swm;

extern "C" {

int swm_blake2s_hash_dev(swm_ctx* ctx, const void* d_inputs, size_t input_len, size_t count, void* d_digests) {
    SWM_TRY(blake2s_hash_check(ctx, d_inputs, input_len, count, d_digests));
    if (((uintptr_t)d_inputs | (uintptr_t)d_digests) & 3)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "blake2s_hash: inputs and digests must be 4-byte aligned");
    SWM_ON_DEVICE(ctx);
    return blake2s_hash_run(ctx, d_inputs, input_len, count, d_digests);
}

int swm_blake2s_hash(swm_ctx* ctx, const uint8_t* inputs, size_t input_len, size_t count, uint8_t* digests) {
    SWM_TRY(blake2s_hash_check(ctx, inputs, input_len, count, digests));
    if (!count) return SWM_OK;
    SWM_ON_DEVICE(ctx);
    const size_t n_in = input_len * count;  // < 2^47
    uint8_t *d_in = nullptr, *d_out = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", n_in + 32, (void**)&d_in));
    SWM_TRY(scratch(ctx, "stage.b", 32 * count, (void**)&d_out));
    if (n_in) SWM_HIP(ctx, hipMemcpyAsync(d_in, inputs, n_in, hipMemcpyHostToDevice, ctx->stream));
    SWM_TRY(blake2s_hash_run(ctx, d_in, input_len, count, d_out));
    SWM_HIP(ctx, hipMemcpyAsync(digests, d_out, 32 * count, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWM_OK;
}

}  // extern "C"

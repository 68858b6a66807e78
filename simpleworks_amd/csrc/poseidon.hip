// poseidon.hip — the reference's native Poseidon hash, batched: PoseidonSponge<Fq> of ark-sponge 0.3.0 over Fq of ed-on-BLS12-377,
// which is BLS12-377 Fr, the field this library multiplies everywhere.
//
// What the reference does there (on one CPU thread):
//   src/hash/mod.rs:30-43     poseidon2_hash(input): PoseidonSponge::new(&params), absorb(&input), squeeze_native_field_elements(1)
//   src/hash/helpers.rs       the parameters: 8 full + 29 partial rounds, alpha = 17, a 3 x 3 MDS matrix, 37 x 3 round keys
// The sponge [U] (ark-sponge 0.3.0, poseidon/mod.rs): rate 2, capacity 1, the state three zeros.  Round i: state[k] += ark[i][k];
// x -> x^alpha on all three entries in the first and last F / 2 rounds, on state[0] alone in the P rounds between;
// state = mds . state.  Absorbing e_0, e_1, ...: state[idx] += e, idx = 0, 1, with a permutation before every element that finds
// idx = 2 (no capacity offset in 0.3.0: the rate section is state[0..2]).  Squeezing: permute, copy state[0], state[1], permute
// again when more are asked for.  Bytes become elements as (length as 8 little-endian bytes || input) cut into chunks of 31 bytes,
// each a little-endian integer (Absorb for [u8], then to_field_elements: CAPACITY / 8 = 31).
//
// On the GPU.  One lane per hash, one wave per workgroup, the state in registers; a permutation is ~600 dependent products
// and the only parallelism is across hashes.  The parameters are launch-uniform: every workgroup copies the table (16 B
// aligned rows of 9 limbs) into LDS once and reads its rows from there, a broadcast read per operand.
// Arithmetic: fr29.cuh's 9 x 29-bit lazy limbs, 197 instructions per product against ~330 for ff.cuh's.  fr29_mul(a, b) is
// a b 2^-261, so state, round keys, matrix and absorbed elements all carry the factor 2^261 (Montgomery form of that radix):
// products keep it, an input takes it from a product with 2^522, an output loses it in a product with 1.
//
// Bounds (fr29.cuh's contract: fr29_mul(a, b) takes a lazy with limbs < 3 x 2^30 = 6 x 2^29, b normalised, a b < 2^261 r, and
// returns a normalised value < 2r).  r < 2^253.
//   table rows           canonical: < r, limbs < 2^29
//   absorbed element     a product: < 2r, limbs < 2^29
//   state after the matrix: a limb-wise sum of three products: < 6r, limbs < 3 x 2^29
//   state + absorbed element (each rate entry takes at most one between two permutations): < 8r, limbs < 4 x 2^29
//   t = that + round key: < 9r, limbs < 5 x 2^29                           -> a legal first operand as it stands
//   S-box: the base serves as second operand, so it is normalised ONCE (carry propagation; < 9r < 2^257 leaves limb 8 < 2^25);
//     the largest product is t t: 81 r^2 < 2^261 r since 81 r < 2^260; every later square is (2r)^2, every product by the base
//     2r x 9r
//   matrix row: sum_b mul(u_b, mds[a][b]), u_b an S-box output (< 2r) or, in a partial round, the lazy t itself (< 9r, limbs
//     < 5 x 2^29) against a canonical entry: 9 r^2.  The three products are added limb-wise and NOT normalised: the sum only
//     ever serves as a first operand again, or is normalised at the head of the next S-box.
// No 32-bit limb exceeds 5 x 2^29 < 2^32, and fr29_normalize's input limit (2^32 - 8) holds with room.
// Every lane of a launch takes the same path: the round kind, the bits of alpha and the item shape are launch-uniform.
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "context.h"
#include "ff.cuh"
#include "fr29.cuh"
#include "poseidon.h"
#include "poseidon_permute.cuh"
#include "swmarlin.h"
#include "witness_host.h"

namespace swm {

// `count` sponges.  BYTES: n_in is the input length in bytes, n_elems the chunks of (length || input); else n_in = n_elems.
// Steps: the absorbing blocks of two elements, then the squeezing blocks of two outputs; a permutation before every step but
// the first absorbing one.
template <bool BYTES>
__global__ void __launch_bounds__(PS_LANES) poseidon_hash_kernel(const uint4* __restrict__ table, unsigned rows, unsigned half_full,
                                                                 unsigned partial, unsigned alpha, const uint8_t* __restrict__ in,
                                                                 size_t n_in, size_t n_elems, size_t count, unsigned n_out,
                                                                 uint32_t* __restrict__ out, uint32_t* __restrict__ status) {
    SWM_LIGHT_KERNEL();
    extern __shared__ __align__(16) uint32_t ps_tab[];
    for (unsigned i = threadIdx.x; i < rows * (PS_ROW / 4); i += PS_LANES) reinterpret_cast<uint4*>(ps_tab)[i] = table[i];
    __syncthreads();
    const size_t item = blockIdx.x * (size_t)PS_LANES + threadIdx.x;
    if (item >= count) return;
    const int alpha_top = 31 - __clz((int)alpha);  // alpha >= 2
    const Fr29 to_mont = ps_row(ps_tab, 0);
    Fr29 one;
#pragma unroll
    for (int i = 0; i < 9; i++) one.l[i] = i == 0 ? 1u : 0u;
    Fr29 s0, s1, s2;
#pragma unroll
    for (int i = 0; i < 9; i++) s0.l[i] = s1.l[i] = s2.l[i] = 0;
    bool bad = false;
    const size_t in_blocks = (n_elems + 1) / 2, out_blocks = (n_out + 1u) / 2;
    uint32_t* o = out + 8 * item * n_out;
#pragma unroll 1
    for (size_t step = 0; step < in_blocks + out_blocks; step++) {
        if (step > 0 || in_blocks == 0) ps_permute(ps_tab, half_full, partial, alpha, alpha_top, s0, s1, s2);
        if (step < in_blocks) {
            // an element < 2^256 times 2^522 (canonical): < 2^261 r; the product is < 2r
            s0 = fr29_add(s0, fr29_mul_fenced(fr29_unpack(ps_fetch<BYTES>(in, item, n_in, 2 * step, bad)), to_mont));
            if (2 * step + 1 < n_elems)
                s1 = fr29_add(s1, fr29_mul_fenced(fr29_unpack(ps_fetch<BYTES>(in, item, n_in, 2 * step + 1, bad)), to_mont));
        } else {
            const unsigned j = 2 * (unsigned)(step - in_blocks);
            // out of the 2^261 form: (lazy state < 6r) x 1 -> < 2r -> canonical
            const Fr y0 = fr29_pack(fr29_canonical(fr29_mul_fenced(s0, one), true));
#pragma unroll
            for (int w = 0; w < 8; w++) o[8 * j + w] = y0.v[w];
            if (j + 1 < n_out) {
                const Fr y1 = fr29_pack(fr29_canonical(fr29_mul_fenced(s1, one), true));
#pragma unroll
                for (int w = 0; w < 8; w++) o[8 * (j + 1) + w] = y1.v[w];
            }
        }
    }
    if (!BYTES) {
        if (bad)
            for (unsigned w = 0; w < 8 * n_out; w++) o[w] = 0;
        if (status) status[item] = bad ? 1u : 0u;
    }
}

template <bool BYTES>
static int poseidon_run(swm_ctx* ctx, const swm_poseidon* p, const uint8_t* d_in, size_t n_in, size_t count, size_t n_out,
                        void* d_out, void* d_status) {
    if (!count) return SWM_OK;
    const size_t n_elems = BYTES ? (8 + n_in + 30) / 31 : n_in;
    const size_t lds = p->rows * PS_ROW * sizeof(uint32_t);
    SWM_LAUNCH(ctx, BYTES ? "poseidon_hash_bytes" : "poseidon_hash_fr", poseidon_hash_kernel<BYTES>,
               dim3((unsigned)((count + PS_LANES - 1) / PS_LANES)), dim3(PS_LANES), lds, reinterpret_cast<const uint4*>(p->d_table),
               (unsigned)p->rows, p->full_rounds / 2, p->partial_rounds, p->alpha, d_in, n_in, n_elems, count, (unsigned)n_out,
               (uint32_t*)d_out, (uint32_t*)d_status);
    return SWM_OK;
}

// v (standard form, < r) -> the nine 29-bit limbs of v 2^261 mod r
static void ps_table_row(const Fr& v_std, uint32_t* row) {
    const Fr m = fp_mul(fp_from_std(v_std), fp_from_u64<Fr>(32));  // the words of Montgomery(32 v) ARE 32 v 2^256 mod r
    for (int i = 0; i < 9; i++) {
        const int bit = 29 * i, w = bit >> 5, off = bit & 31;
        uint64_t v = m.v[w];
        if (w + 1 < 8) v |= (uint64_t)m.v[w + 1] << 32;
        row[i] = (uint32_t)(v >> off) & (i < 8 ? M29 : 0xFFFFFFFFu);
    }
    for (unsigned i = 9; i < PS_ROW; i++) row[i] = 0;
}

static int hash_args(swm_ctx* ctx, const char* what, const swm_poseidon* p, size_t count) {
    if (!ctx || !p) return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: bad arguments", what);
    if (count > 0x7FFFFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "%s: %zu items in one call", what, count);
    return SWM_OK;
}
static int fr_args(swm_ctx* ctx, const swm_poseidon* p, const void* elems, size_t n_in, size_t count, size_t n_out, const void* out) {
    SWM_TRY(hash_args(ctx, "poseidon_hash_fr", p, count));
    if (n_in > PS_MAX_IN || n_out < 1 || n_out > PS_MAX_OUT)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_hash_fr: %zu elements in, %zu out (at most %zu in, 1 to %zu out)", n_in, n_out,
                       PS_MAX_IN, PS_MAX_OUT);
    if (count && (!out || (n_in && !elems))) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_hash_fr: NULL buffer");
    return SWM_OK;
}
static int bytes_args(swm_ctx* ctx, const swm_poseidon* p, const void* inputs, size_t input_len, size_t count, const void* digests) {
    SWM_TRY(hash_args(ctx, "poseidon_hash_bytes", p, count));
    if (input_len > PS_MAX_BYTES)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_hash_bytes: inputs of %zu bytes (at most %zu)", input_len, PS_MAX_BYTES);
    if (count && (!digests || (input_len && !inputs))) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_hash_bytes: NULL buffer");
    return SWM_OK;
}

// host buffers through the context's staging areas; in_bytes may be 0
template <bool BYTES>
static int poseidon_host(swm_ctx* ctx, const swm_poseidon* p, const uint8_t* in, size_t in_bytes, size_t n_in, size_t count, size_t n_out,
                         uint8_t* out) {
    uint8_t *d_in = nullptr, *d_out = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", in_bytes + 32, (void**)&d_in));
    SWM_TRY(scratch(ctx, "stage.b", count * n_out * 32, (void**)&d_out));
    if (in_bytes) SWM_HIP(ctx, hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    SWM_TRY(poseidon_run<BYTES>(ctx, p, d_in, n_in, count, n_out, d_out, nullptr));
    SWM_HIP(ctx, hipMemcpyAsync(out, d_out, count * n_out * 32, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWM_OK;
}

}  // namespace swm

using namespace swm;

extern "C" {

int swm_poseidon_create(swm_ctx* ctx, size_t full_rounds, size_t partial_rounds, uint64_t alpha, const uint8_t* mds, const uint8_t* ark,
                        swm_poseidon** out) {
    if (!ctx || !mds || !ark || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_create: bad arguments");
    if (full_rounds < 2 || (full_rounds & 1) || partial_rounds > PS_MAX_ROUNDS || full_rounds + partial_rounds > PS_MAX_ROUNDS)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_create: %zu full and %zu partial rounds (full even and >= 2, at most %zu in all)",
                       full_rounds, partial_rounds, PS_MAX_ROUNDS);
    if (alpha < 2 || alpha > 65535)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_create: alpha = %llu (2 .. 65535)", (unsigned long long)alpha);
    const size_t rounds = full_rounds + partial_rounds, rows = PS_ARK + 3 * rounds;
    std::vector<uint32_t> table(rows * PS_ROW);
    Fr v = fp_from_u64<Fr>(32);  // its words: 2^261 mod r, read as a standard value -> row 0 = 2^522 mod r
    ps_table_row(v, table.data());
    for (size_t i = 0; i < 9 + 3 * rounds; i++) {
        if (!ps_load_std(i < 9 ? mds + 32 * i : ark + 32 * (i - 9), &v)) {
            if (i < 9) return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_create: mds[%zu][%zu] is not a canonical field element", i / 3, i % 3);
            return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_create: ark[%zu][%zu] is not a canonical field element", (i - 9) / 3, (i - 9) % 3);
        }
        ps_table_row(v, table.data() + PS_ROW * (PS_MDS + i));
    }
    SWM_ON_DEVICE(ctx);
    std::unique_ptr<swm_poseidon> p(new swm_poseidon);
    p->full_rounds = (unsigned)full_rounds;
    p->partial_rounds = (unsigned)partial_rounds;
    p->alpha = (unsigned)alpha;
    p->rows = rows;
    const size_t bytes = table.size() * sizeof(uint32_t);
    hipError_t e = hipMalloc(&p->d_table, bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_table, table.data(), bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // `table` goes out of scope
    if (e != hipSuccess) {
        if (p->d_table) (void)hipFree(p->d_table);
        (void)hipGetLastError();
        return set_err(ctx, e == hipErrorOutOfMemory ? SWM_ERR_OOM : SWM_ERR_HIP, "poseidon_create: %s", hipGetErrorString(e));
    }
    *out = p.release();
    return SWM_OK;
}

void swm_poseidon_destroy(swm_ctx* ctx, swm_poseidon* p) {
    if (!p) return;
    DeviceGuard guard(ctx);
    if (ctx) drain_streams(ctx);
    if (p->d_table) (void)hipFree(p->d_table);
    delete p;
}

int swm_poseidon_hash_fr_dev(swm_ctx* ctx, const swm_poseidon* p, const void* d_elems, size_t n_in, size_t count, size_t n_out, void* d_out,
                             void* d_status) {
    SWM_TRY(fr_args(ctx, p, d_elems, n_in, count, n_out, d_out));
    SWM_ON_DEVICE(ctx);
    return drained(ctx, poseidon_run<false>(ctx, p, (const uint8_t*)d_elems, n_in, count, n_out, d_out, d_status));
}

int swm_poseidon_hash_fr(swm_ctx* ctx, const swm_poseidon* p, const uint8_t* elems, size_t n_in, size_t count, size_t n_out, uint8_t* out) {
    SWM_TRY(fr_args(ctx, p, elems, n_in, count, n_out, out));
    if (!count) return SWM_OK;
    Fr v;
    for (size_t i = 0; i < count * n_in; i++)
        if (!ps_load_std(elems + 32 * i, &v))
            return set_err(ctx, SWM_ERR_INVALID_ARG, "poseidon_hash_fr: item %zu: element %zu is not a canonical field element", i / n_in, i % n_in);
    SWM_ON_DEVICE(ctx);
    return drained(ctx, poseidon_host<false>(ctx, p, elems, count * n_in * 32, n_in, count, n_out, out));
}

int swm_poseidon_hash_bytes_dev(swm_ctx* ctx, const swm_poseidon* p, const void* d_inputs, size_t input_len, size_t count, void* d_digests) {
    SWM_TRY(bytes_args(ctx, p, d_inputs, input_len, count, d_digests));
    SWM_ON_DEVICE(ctx);
    return drained(ctx, poseidon_run<true>(ctx, p, (const uint8_t*)d_inputs, input_len, count, 1, d_digests, nullptr));
}

int swm_poseidon_hash_bytes(swm_ctx* ctx, const swm_poseidon* p, const uint8_t* inputs, size_t input_len, size_t count, uint8_t* digests) {
    SWM_TRY(bytes_args(ctx, p, inputs, input_len, count, digests));
    if (!count) return SWM_OK;
    SWM_ON_DEVICE(ctx);
    return drained(ctx, poseidon_host<true>(ctx, p, inputs, count * input_len, input_len, count, 1, digests));
}

}  // extern "C"

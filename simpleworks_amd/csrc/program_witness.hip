// program_witness.hip — the witness of a batch of executions of one integer PROGRAM, synthesised on the GPU: the step between a
// caller's tape and input values and the proof that the program's outputs are the public ones (marlin.hip).
//
// What the reference does there: a caller writes the statement out of the gadgets of src/gadgets/ (UInt8 .. UInt128, Boolean behind
// the traits of traits.rs) and runs the synthesizer once per execution, on one CPU thread.  Here the statement is a tape
// (host/program_shape.h: format, validator, plan), its circuit and witness order are those of simpleworks_amd/workloads.py,
// build_program, and all executions of one program share the tape: only the register values differ per item.
//
// On the GPU, two kernels and a small third.
//   program_exec_kernel    one lane per item.  The plan's instructions are the same for every lane — wave-uniform reads, a
//                          wave-uniform switch — and every value an instruction produces (its register, and the carry, the high
//                          product half, the remainder, the comparison sum, the EQ inverse) goes to the VALUE TRACE in device memory,
//                          laid out [slot][item] in 16-byte cells: a wave reads and writes 64 consecutive cells.  A register is
//                          only ever a trace address, never an index into a per-lane array.  No branch depends on a value.
//   program_inverse_kernel one lane per item and EQ instruction: the inverse of a - b (frinv.cuh, data-dependent) into the trace.
//   program_expand_kernel  the store stream.  Every witness is written in storage order, 16 bytes per lane, two lanes per element,
//                          consecutive lanes on consecutive addresses, every chunk of an item exactly once.  A workgroup covers
//                          PG_BLOCK_WITNESSES witnesses of one item: it stages the descriptors between two entries of the plan's
//                          per-block index in LDS (at most 129), a lane finds its own by a binary search there (at most 8 steps),
//                          reads one word of the trace and stores 0 or its half of the Montgomery 1.  The EQ inverse is the only full field element.
// The validator has run on the host before anything was uploaded: the kernels check no index but the two grid tails.
#include <hip/hip_runtime.h>

#include <string.h>

#include <memory>
#include <vector>

#include "context.h"
#include "ff.cuh"
#include "frinv.cuh"
#include "host/program_shape.h"
#include "swmarlin.h"
#include "witness_host.h"

struct swm_program {
    swm::ProgramShape shape;
    swm::PgExec* d_exec = nullptr;
    swm::PgDesc* d_desc = nullptr;
    uint32_t* d_block_first = nullptr;
    uint32_t* d_eq_slots = nullptr;
};

namespace swm {

static constexpr unsigned PG_LANES = 256;
static_assert(PG_LANES == 2 * PG_BLOCK_WITNESSES, "the expand kernel writes two 16-byte chunks per witness");

struct PgVal {
    uint64_t lo, hi;
};
__device__ __forceinline__ PgVal pg_get(const ulonglong2* __restrict__ trace, size_t count, uint32_t slot, size_t item) {
    const ulonglong2 v = trace[(size_t)slot * count + item];
    return {v.x, v.y};
}
__device__ __forceinline__ void pg_put(ulonglong2* __restrict__ trace, size_t count, uint32_t slot, size_t item, PgVal v) {
    trace[(size_t)slot * count + item] = make_ulonglong2(v.lo, v.hi);
}
__device__ __forceinline__ PgVal pg_mask(unsigned W) {  // W: 1, 8, 16, 32, 64 or 128 (wave-uniform)
    PgVal m;
    m.lo = W >= 64 ? ~0ull : (1ull << W) - 1;
    m.hi = W > 64 ? ~0ull : 0ull;
    return m;
}
__device__ __forceinline__ PgVal pg_and(PgVal a, PgVal b) { return {a.lo & b.lo, a.hi & b.hi}; }
__device__ __forceinline__ bool pg_eq(PgVal a, PgVal b) { return ((a.lo ^ b.lo) | (a.hi ^ b.hi)) == 0; }
__device__ __forceinline__ bool pg_lt(PgVal a, PgVal b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
// a + b with the carry out of bit 127, a - b modulo 2^128: the carries by hand
__device__ __forceinline__ PgVal pg_add(PgVal a, PgVal b, unsigned* carry) {
    PgVal s;
    s.lo = a.lo + b.lo;
    const uint64_t c0 = s.lo < a.lo;
    const uint64_t h = a.hi + b.hi;
    s.hi = h + c0;
    *carry = (unsigned)((h < a.hi) | (s.hi < h));
    return s;
}
__device__ __forceinline__ PgVal pg_sub(PgVal a, PgVal b) {
    PgVal d;
    d.lo = a.lo - b.lo;
    d.hi = a.hi - b.hi - (a.lo < b.lo);
    return d;
}
// shifts by k = 0 .. 128 positions (wave-uniform k)
__device__ __forceinline__ PgVal pg_shl(PgVal a, unsigned k) {
    if (k == 0) return a;
    if (k >= 128) return {0, 0};
    if (k >= 64) return {0, a.lo << (k - 64)};
    return {a.lo << k, (a.hi << k) | (a.lo >> (64 - k))};
}
__device__ __forceinline__ PgVal pg_shr(PgVal a, unsigned k) {
    if (k == 0) return a;
    if (k >= 128) return {0, 0};
    if (k >= 64) return {a.hi >> (k - 64), 0};
    return {(a.lo >> k) | (a.hi << (64 - k)), a.hi >> k};
}

struct PgExecArgs {
    size_t count, input_bytes, output_bytes;
    uint32_t instructions;
};

// Lane p of the grid = item p.  in: count x input_bytes; trace: slots x count cells; out: count x output_bytes; status: count bytes.
__global__ void __launch_bounds__(PG_LANES) program_exec_kernel(PgExecArgs A, const PgExec* __restrict__ plan, const uint8_t* __restrict__ in,
                                                                ulonglong2* __restrict__ trace, uint8_t* __restrict__ out,
                                                                uint8_t* __restrict__ status) {
    const size_t item = (size_t)blockIdx.x * PG_LANES + threadIdx.x;
    if (item >= A.count) return;
    const size_t n = A.count;
    unsigned st = 0;
    for (uint32_t k = 0; k < A.instructions; k++) {
        const PgExec e = plan[k];  // the same address in every lane
        const unsigned W = e.width;
        const PgVal mask = pg_mask(W);
        switch (e.op) {
            case PG_INPUT_PUBLIC:
            case PG_INPUT_PRIVATE: {
                const uint8_t* src = in + item * A.input_bytes + e.imm_lo;
                const unsigned bytes = W == 1 ? 1u : W / 8u;
                PgVal v = {0, 0};
                for (unsigned j = 0; j < bytes && j < 8; j++) v.lo |= (uint64_t)src[j] << (8 * j);
                for (unsigned j = 8; j < bytes; j++) v.hi |= (uint64_t)src[j] << (8 * (j - 8));
                pg_put(trace, n, e.dst, item, pg_and(v, mask));
                break;
            }
            case PG_CONST: pg_put(trace, n, e.dst, item, {e.imm_lo, e.imm_hi}); break;
            case PG_AND:
            case PG_NAND:
            case PG_OR:
            case PG_NOR:
            case PG_XOR: {
                const PgVal a = pg_get(trace, n, e.a, item), b = pg_get(trace, n, e.b, item);
                PgVal r;
                if (e.op == PG_XOR) r = {a.lo ^ b.lo, a.hi ^ b.hi};
                else if (e.op == PG_AND || e.op == PG_NAND) r = pg_and(a, b);
                else r = {a.lo | b.lo, a.hi | b.hi};
                if (e.op == PG_NAND || e.op == PG_NOR) r = {~r.lo, ~r.hi};
                pg_put(trace, n, e.dst, item, pg_and(r, mask));
                break;
            }
            case PG_NOT: {
                const PgVal a = pg_get(trace, n, e.a, item);
                pg_put(trace, n, e.dst, item, pg_and({~a.lo, ~a.hi}, mask));
                break;
            }
            case PG_ADD: {
                const PgVal a = pg_get(trace, n, e.a, item), b = pg_get(trace, n, e.b, item);
                unsigned carry;
                const PgVal s = pg_add(a, b, &carry);
                if (W < 64) carry = (unsigned)(s.lo >> W) & 1u;
                else if (W == 64) carry = (unsigned)s.hi & 1u;
                pg_put(trace, n, e.dst, item, pg_and(s, mask));
                pg_put(trace, n, e.dst + 1, item, {carry, 0});
                break;
            }
            case PG_SUB: {
                const PgVal a = pg_get(trace, n, e.a, item), b = pg_get(trace, n, e.b, item);
                if (pg_lt(a, b)) st |= PG_STATUS_UNDERFLOW;
                pg_put(trace, n, e.dst, item, pg_and(pg_sub(a, b), mask));  // the wrapped difference when a < b
                break;
            }
            case PG_MUL: {  // W <= 64: the 64 x 64 -> 128 product
                const uint64_t a = pg_get(trace, n, e.a, item).lo, b = pg_get(trace, n, e.b, item).lo;
                const uint64_t lo = a * b;
                PgVal low, high;
                if (W == 64) {
                    low = {lo, 0};
                    high = {__umul64hi(a, b), 0};
                } else {  // the product is below 2^64
                    low = {lo & mask.lo, 0};
                    high = {(lo >> W) & mask.lo, 0};
                }
                pg_put(trace, n, e.dst, item, low);
                pg_put(trace, n, e.dst + 1, item, high);
                break;
            }
            case PG_DIV: {  // W <= 64
                const uint64_t a = pg_get(trace, n, e.a, item).lo, b = pg_get(trace, n, e.b, item).lo;
                uint64_t q = 0, rem = a;
                if (b == 0) {
                    st |= PG_STATUS_DIV_ZERO;
                } else {
                    q = a / b;
                    rem = a - q * b;
                }
                pg_put(trace, n, e.dst, item, {q, 0});
                pg_put(trace, n, e.dst + 1, item, {rem, 0});
                pg_put(trace, n, e.dst + 2, item, {(b - 1 - rem) & mask.lo, 0});  // wrapped when b = 0
                break;
            }
            case PG_SHL: pg_put(trace, n, e.dst, item, pg_and(pg_shl(pg_get(trace, n, e.a, item), (unsigned)e.imm_lo), mask)); break;
            case PG_SHR: pg_put(trace, n, e.dst, item, pg_shr(pg_get(trace, n, e.a, item), (unsigned)e.imm_lo)); break;
            case PG_ROTL: {
                const PgVal a = pg_get(trace, n, e.a, item), l = pg_shl(a, (unsigned)e.imm_lo), r = pg_shr(a, W - (unsigned)e.imm_lo);
                pg_put(trace, n, e.dst, item, pg_and({l.lo | r.lo, l.hi | r.hi}, mask));
                break;
            }
            case PG_GT:
            case PG_GTE:
            case PG_LT:
            case PG_LTE: {  // x > y is the top bit of x - y - 1 + 2^W
                const bool direct = e.op == PG_GT || e.op == PG_LTE;
                const PgVal x = pg_get(trace, n, direct ? e.a : e.b, item), y = pg_get(trace, n, direct ? e.b : e.a, item);
                const unsigned gt = pg_lt(y, x);
                const PgVal low = pg_and(pg_sub(pg_sub(x, y), {1, 0}), mask);
                pg_put(trace, n, e.dst, item, {(e.op == PG_GT || e.op == PG_LT) ? gt : gt ^ 1u, 0});
                pg_put(trace, n, e.dst + 1, item, low);
                break;
            }
            case PG_EQ: {
                const PgVal a = pg_get(trace, n, e.a, item), b = pg_get(trace, n, e.b, item);
                const bool same = pg_eq(a, b), neg = pg_lt(a, b);
                pg_put(trace, n, e.dst, item, {same ? 1u : 0u, 0});
                pg_put(trace, n, e.dst + 1, item, neg ? pg_sub(b, a) : pg_sub(a, b));  // |a - b| and its sign: program_inverse_kernel's input
                pg_put(trace, n, e.dst + 2, item, {neg ? 1u : 0u, 0});
                break;
            }
            case PG_SELECT: {
                const PgVal c = pg_get(trace, n, e.a, item), a = pg_get(trace, n, e.b, item), b = pg_get(trace, n, e.c, item);
                pg_put(trace, n, e.dst, item, (c.lo & 1) ? a : b);
                break;
            }
            case PG_ASSERT_EQ:
                if (!pg_eq(pg_get(trace, n, e.a, item), pg_get(trace, n, e.b, item))) st |= PG_STATUS_ASSERT;
                break;
            case PG_OUTPUT: {
                const PgVal a = pg_get(trace, n, e.a, item);
                uint8_t* dst = out + item * A.output_bytes + e.imm_lo;
                const unsigned bytes = W == 1 ? 1u : W / 8u;
                for (unsigned j = 0; j < bytes && j < 8; j++) dst[j] = (uint8_t)(a.lo >> (8 * j));
                for (unsigned j = 8; j < bytes; j++) dst[j] = (uint8_t)(a.hi >> (8 * (j - 8)));
                break;
            }
            default: break;
        }
    }
    if (status) status[item] = (uint8_t)st;
}

// The inverse behind every EQ: lane p of row j = item p of the j-th EQ instruction, whose answer sits in slot eq_slots[j].  Reads
// |a - b| and its sign from the two slots behind it and overwrites them with the halves of (a - b)^-1 in Montgomery form, 0 when
// a = b.  The binary Euclid's data-dependent branches (frinv.cuh) stay out of the exec kernel.
__global__ void __launch_bounds__(PG_LANES) program_inverse_kernel(size_t count, const uint32_t* __restrict__ eq_slots, ulonglong2* __restrict__ trace) {
    const size_t item = (size_t)blockIdx.x * PG_LANES + threadIdx.x;
    if (item >= count) return;
    const uint32_t slot = eq_slots[blockIdx.y];
    const PgVal mag = pg_get(trace, count, slot + 1, item);
    const bool neg = pg_get(trace, count, slot + 2, item).lo != 0;
    Fr inv = fp_zero<Fr>();
    if (mag.lo | mag.hi) {
        Fr z = fp_zero<Fr>();
        z.v[0] = (uint32_t)mag.lo;
        z.v[1] = (uint32_t)(mag.lo >> 32);
        z.v[2] = (uint32_t)mag.hi;
        z.v[3] = (uint32_t)(mag.hi >> 32);
        z = fp_from_std(z);
        if (neg) z = fp_neg(z);
        inv = fr_inv_single(z);
    }
    pg_put(trace, count, slot + 1, item, {(uint64_t)inv.v[0] | (uint64_t)inv.v[1] << 32, (uint64_t)inv.v[2] | (uint64_t)inv.v[3] << 32});
    pg_put(trace, count, slot + 2, item, {(uint64_t)inv.v[4] | (uint64_t)inv.v[5] << 32, (uint64_t)inv.v[6] | (uint64_t)inv.v[7] << 32});
}

struct PgExpandArgs {
    size_t count, num_witness;
    uint32_t blocks_per_item, descriptors;
};

// Workgroup g = block g % blocks_per_item of item g / blocks_per_item.  trace: the cells as 4 words each; witness: count x
// num_witness elements as 16-byte chunks.
__global__ void __launch_bounds__(PG_LANES) program_expand_kernel(PgExpandArgs A, const PgDesc* __restrict__ desc,
                                                                  const uint32_t* __restrict__ block_first, const uint32_t* __restrict__ trace,
                                                                  uint4* __restrict__ witness) {
    // the descriptors that meet this block's 128 witnesses: at most 129, since each holds a witness of its own
    __shared__ PgDesc sh[PG_BLOCK_WITNESSES + 1];
    const unsigned tid = threadIdx.x;
    const size_t item = blockIdx.x / A.blocks_per_item;
    const uint32_t blk = blockIdx.x % A.blocks_per_item;
    const uint32_t e = blk * PG_BLOCK_WITNESSES + (tid >> 1), half = tid & 1u;
    const uint32_t first = block_first[blk];
    uint32_t last = block_first[blk + 1];
    if (last >= A.descriptors) last = A.descriptors - 1;
    if (last - first > PG_BLOCK_WITNESSES) last = first + PG_BLOCK_WITNESSES;  // (cannot happen: program_shape_check holds the index to it)
    if (tid <= last - first) sh[tid] = desc[first + tid];  // one round of loads instead of a search through global memory
    __syncthreads();
    if (e >= A.num_witness) return;
    const Fr f_one = fp_one<Fr>();
    // chunk c = 2 e + half: a lane writes the same half of `one` whatever its witness
    const uint4 zero = make_uint4(0, 0, 0, 0);
    const uint4 mine = half ? make_uint4(f_one.v[4], f_one.v[5], f_one.v[6], f_one.v[7]) : make_uint4(f_one.v[0], f_one.v[1], f_one.v[2], f_one.v[3]);
    // the last of them that starts at or before e
    uint32_t lo = 0, hi = last - first;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (sh[mid].at <= e) lo = mid;
        else hi = mid - 1;
    }
    const PgDesc d = sh[lo];
    const uint32_t i = e - d.at;
    uint4 v;
    if (d.kind == PG_DESC_FIELD) {
        v = reinterpret_cast<const uint4*>(trace)[(size_t)(d.slot + half) * A.count + item];
    } else {
        const uint32_t word = trace[((size_t)d.slot * A.count + item) * 4 + (i >> 5)];
        v = (((word >> (i & 31u)) & 1u) ^ d.kind) ? mine : zero;
    }
    witness[item * 2 * A.num_witness + 2 * (size_t)e + half] = v;
}

// d_witness: count x num_witness elements, 16-byte aligned; d_in: count x input_bytes; d_out: count x output_bytes; d_status (may
// be NULL): count bytes.  The trace lives in the scratch buffer "program.trace".
static int program_run(swm_ctx* ctx, const swm_program* p, const uint8_t* d_in, size_t count, void* d_witness, uint8_t* d_out, uint8_t* d_status) {
    const ProgramShape& s = p->shape;
    if (!count) return SWM_OK;
    const size_t blocks_per_item = (s.num_witness + PG_BLOCK_WITNESSES - 1) / PG_BLOCK_WITNESSES;
    if (count > 0x7FFFFFFFu || count * (blocks_per_item ? blocks_per_item : 1) > 0x7FFFFFFFu)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "program_witness: %zu items of %zu witnesses in one call", count, s.num_witness);
    ulonglong2* d_trace = nullptr;
    SWM_TRY(scratch(ctx, "program.trace", (s.slots ? s.slots : 1) * count * sizeof(ulonglong2), (void**)&d_trace));
    PgExecArgs E;
    E.count = count;
    E.input_bytes = s.input_bytes;
    E.output_bytes = s.output_bytes;
    E.instructions = (uint32_t)s.instructions;
    SWM_LAUNCH(ctx, "program_exec", program_exec_kernel, dim3((unsigned)((count + PG_LANES - 1) / PG_LANES)), dim3(PG_LANES), 0, E, p->d_exec, d_in,
               d_trace, d_out, d_status);
    if (!s.num_witness) return SWM_OK;
    if (!s.eq_slots.empty())
        SWM_LAUNCH(ctx, "program_inverse", program_inverse_kernel, dim3((unsigned)((count + PG_LANES - 1) / PG_LANES), (unsigned)s.eq_slots.size()),
                   dim3(PG_LANES), 0, count, p->d_eq_slots, d_trace);
    PgExpandArgs X;
    X.count = count;
    X.num_witness = s.num_witness;
    X.blocks_per_item = (uint32_t)blocks_per_item;
    X.descriptors = (uint32_t)s.desc.size();
    SWM_LAUNCH(ctx, "program_expand", program_expand_kernel, dim3((unsigned)(count * blocks_per_item)), dim3(PG_LANES), 0, X, p->d_desc,
               p->d_block_first, (const uint32_t*)d_trace, (uint4*)d_witness);
    return SWM_OK;
}

// items per chunk; a program with no witnesses has nothing to fit the stage: 2^20 items at a time
static size_t pg_items_per_chunk(const swm_ctx* ctx, const ProgramShape& s) {
    const size_t fit = witness_stage_items(ctx, s.num_witness * sizeof(Fr));
    return fit ? fit : (size_t)1 << 20;
}

struct PgOut {  // "program.w": witnesses | outputs | status
    uint8_t *w, *out, *status;
};

// n items staged and run; the results stay in "program.w"
static int pg_chunk(swm_ctx* ctx, const swm_program* p, const uint8_t* inputs, size_t n, PgOut* o) {
    const ProgramShape& s = p->shape;
    const size_t item = s.num_witness * sizeof(Fr);
    uint8_t *d_in = nullptr, *d_w = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", n * s.input_bytes + 32, (void**)&d_in));
    SWM_TRY(scratch(ctx, "program.w", n * (item + s.output_bytes + 1) + 32, (void**)&d_w));
    if (s.input_bytes) SWM_HIP(ctx, hipMemcpyAsync(d_in, inputs, n * s.input_bytes, hipMemcpyHostToDevice, ctx->stream));
    o->w = d_w;
    o->out = d_w + n * item;
    o->status = o->out + n * s.output_bytes;
    return program_run(ctx, p, d_in, n, o->w, o->out, o->status);
}

static int program_witness_host(swm_ctx* ctx, const swm_program* p, const uint8_t* inputs, size_t count, uint64_t* witness, uint8_t* outputs,
                                uint8_t* status) {
    const ProgramShape& s = p->shape;
    const size_t item = s.num_witness * sizeof(Fr);
    for (const WitnessChunk ch : WitnessChunks(pg_items_per_chunk(ctx, s), count)) {
        const size_t base = ch.base, n = ch.count;
        PgOut o;
        SWM_TRY(pg_chunk(ctx, p, inputs ? inputs + base * s.input_bytes : nullptr, n, &o));
        if (item) SWM_HIP(ctx, hipMemcpyAsync(reinterpret_cast<uint8_t*>(witness) + base * item, o.w, n * item, hipMemcpyDeviceToHost, ctx->stream));
        if (outputs && s.output_bytes)
            SWM_HIP(ctx, hipMemcpyAsync(outputs + base * s.output_bytes, o.out, n * s.output_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (status) SWM_HIP(ctx, hipMemcpyAsync(status + base, o.status, n, hipMemcpyDeviceToHost, ctx->stream));
        SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the staging buffers are reused by the next chunk
    }
    return SWM_OK;
}

// `width` bits of a little-endian value as field elements 0 / 1 in Montgomery form, appended to inst
static void pg_push_bits(std::vector<Fr>& inst, const uint8_t* bytes, unsigned width) {
    for (unsigned i = 0; i < width; i++) inst.push_back((bytes[i >> 3] >> (i & 7)) & 1u ? fp_one<Fr>() : fp_zero<Fr>());
}

// the prover over one item's device witnesses; instance: one, the bits of the public inputs, the bits of the outputs
static int pg_prove_item(swm_ctx* ctx, const swm_pk* pk, const ProgramShape& s, const uint8_t* input, const uint8_t* output, const Fr* d_w,
                         swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len) {
    std::vector<Fr> inst;
    inst.reserve(s.num_instance);
    inst.push_back(fp_one<Fr>());
    for (uint8_t t : s.public_types) {
        pg_push_bits(inst, input, pg_width(t));
        input += pg_bytes(t);
    }
    for (uint8_t t : s.output_types) {
        pg_push_bits(inst, output, pg_width(t));
        output += pg_bytes(t);
    }
    return prove_device_witness(ctx, pk, s.num_instance, s.num_witness, s.num_constraints, inst.data(), d_w, rng, flags, proof_out, cap, len);
}

}  // namespace swm

using namespace swm;

extern "C" {

int swm_program_create(swm_ctx* ctx, const uint8_t* tape, size_t len, swm_program** out) {
    if (!ctx || !tape || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "program_create: bad arguments");
    std::unique_ptr<swm_program> p(new swm_program);
    const char* why = "";
    if (!program_shape(tape, len, &p->shape, &why)) return set_err(ctx, SWM_ERR_INVALID_ARG, "program_create: %s", why);
    const ProgramShape& s = p->shape;
    SWM_ON_DEVICE(ctx);
    // (an empty vector still gets a one-entry allocation: the kernels' pointers are never NULL)
    const size_t exec_bytes = (s.exec.size() + 1) * sizeof(PgExec), desc_bytes = (s.desc.size() + 1) * sizeof(PgDesc);
    const size_t first_bytes = s.block_first.size() * sizeof(uint32_t);
    hipError_t e = hipMalloc((void**)&p->d_exec, exec_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_desc, desc_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_block_first, first_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_eq_slots, (s.eq_slots.size() + 1) * sizeof(uint32_t));
    if (e == hipSuccess && !s.eq_slots.empty())
        e = hipMemcpyAsync(p->d_eq_slots, s.eq_slots.data(), s.eq_slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && !s.exec.empty())
        e = hipMemcpyAsync(p->d_exec, s.exec.data(), s.exec.size() * sizeof(PgExec), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && !s.desc.empty())
        e = hipMemcpyAsync(p->d_desc, s.desc.data(), s.desc.size() * sizeof(PgDesc), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_block_first, s.block_first.data(), first_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        if (p->d_exec) (void)hipFree(p->d_exec);
        if (p->d_desc) (void)hipFree(p->d_desc);
        if (p->d_block_first) (void)hipFree(p->d_block_first);
        if (p->d_eq_slots) (void)hipFree(p->d_eq_slots);
        (void)hipGetLastError();
        return set_err(ctx, e == hipErrorOutOfMemory ? SWM_ERR_OOM : SWM_ERR_HIP, "program_create: %s", hipGetErrorString(e));
    }
    *out = p.release();
    return SWM_OK;
}

void swm_program_destroy(swm_ctx* ctx, swm_program* p) {
    destroy_circuit(ctx, p, [](swm_program* q) {
        if (q->d_exec) (void)hipFree(q->d_exec);
        if (q->d_desc) (void)hipFree(q->d_desc);
        if (q->d_block_first) (void)hipFree(q->d_block_first);
        if (q->d_eq_slots) (void)hipFree(q->d_eq_slots);
    });
}

int swm_program_witness(swm_ctx* ctx, const swm_program* p, const uint8_t* inputs, size_t count, uint64_t* witness, uint8_t* outputs,
                        uint8_t* status) {
    if (!ctx || !p) return set_err(ctx, SWM_ERR_INVALID_ARG, "program_witness: bad arguments");
    const ProgramShape& s = p->shape;
    if (count && ((s.num_witness && !witness) || (s.input_bytes && !inputs) || (s.output_bytes && !outputs) || !status))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "program_witness: bad arguments");
    if (!count) return SWM_OK;
    if (count > 0x7FFFFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "program_witness: %zu items in one call", count);
    SWM_ON_DEVICE(ctx);
    return drained(ctx, program_witness_host(ctx, p, inputs, count, witness, outputs, status));
}

int swm_program_witness_dev(swm_ctx* ctx, const swm_program* p, const void* d_inputs, size_t count, void* d_witness, void* d_outputs,
                            void* d_status) {
    if (!ctx || !p) return set_err(ctx, SWM_ERR_INVALID_ARG, "program_witness_dev: bad arguments");
    const ProgramShape& s = p->shape;
    if (count && ((s.num_witness && !d_witness) || (s.input_bytes && !d_inputs) || (s.output_bytes && !d_outputs)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "program_witness_dev: bad arguments");
    if ((uintptr_t)d_witness & 15) return set_err(ctx, SWM_ERR_INVALID_ARG, "program_witness_dev: the witness must be 16-byte aligned");
    SWM_ON_DEVICE(ctx);
    return drained(ctx, program_run(ctx, p, (const uint8_t*)d_inputs, count, d_witness, (uint8_t*)d_outputs, (uint8_t*)d_status));
}

int swm_program_prove(swm_ctx* ctx, const swm_pk* pk, const swm_program* p, const uint8_t* input, swm_rng* rng, unsigned flags,
                      uint8_t* output, uint8_t* status_out, uint8_t* proof_out, size_t cap, size_t* len) {
    if (!ctx || !pk || !p || !rng || !proof_out || !len) return set_err(ctx, SWM_ERR_INVALID_ARG, "program_prove: bad arguments");
    const ProgramShape& s = p->shape;
    if ((s.input_bytes && !input) || (s.output_bytes && !output)) return set_err(ctx, SWM_ERR_INVALID_ARG, "program_prove: bad arguments");
    PgOut o;
    std::vector<uint8_t> host(s.output_bytes + 1);
    {
        SWM_ON_DEVICE(ctx);
        SWM_TRY(drained(ctx, pg_chunk(ctx, p, input, 1, &o)));
        SWM_HIP(ctx, hipMemcpyAsync(host.data(), o.out, s.output_bytes + 1, hipMemcpyDeviceToHost, ctx->stream));  // outputs | status
        SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    const uint8_t st = host[s.output_bytes];
    if (s.output_bytes) memcpy(output, host.data(), s.output_bytes);
    if (status_out) *status_out = st;
    if (st) return set_err(ctx, SWM_ERR_UNSATISFIED, "program_prove: status %u (1 SUB underflow, 2 DIV by zero, 4 ASSERT_EQ)", (unsigned)st);
    return pg_prove_item(ctx, pk, s, input, host.data(), (const Fr*)o.w, rng, flags, proof_out, cap, len);
}

int swm_program_prove_many(swm_ctx* ctx, const swm_pk* pk, const swm_program* p, const uint8_t* inputs, size_t count, swm_rng* rng,
                           unsigned flags, uint8_t* outputs, uint8_t* status, uint8_t* proofs_out, size_t proof_cap, size_t* lens) {
    if (!ctx || !pk || !p || !rng) return set_err(ctx, SWM_ERR_INVALID_ARG, "program_prove_many: bad arguments");
    const ProgramShape& s = p->shape;
    if (count && ((s.input_bytes && !inputs) || (s.output_bytes && !outputs) || !status || !proofs_out || !lens))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "program_prove_many: bad arguments");
    if (!count) return SWM_OK;
    for (size_t i = 0; i < count; i++) {  // whatever ends the call, every entry of the two arrays has been written
        lens[i] = 0;
        status[i] = 0;
    }
    if (count > 0x7FFFFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "program_prove_many: %zu items in one call", count);
    for (const WitnessChunk ch : WitnessChunks(pg_items_per_chunk(ctx, s), count)) {
        const size_t base = ch.base, n = ch.count;
        PgOut o;
        {
            SWM_ON_DEVICE(ctx);
            SWM_TRY(drained(ctx, pg_chunk(ctx, p, inputs ? inputs + base * s.input_bytes : nullptr, n, &o)));
            if (s.output_bytes)
                SWM_HIP(ctx, hipMemcpyAsync(outputs + base * s.output_bytes, o.out, n * s.output_bytes, hipMemcpyDeviceToHost, ctx->stream));
            SWM_HIP(ctx, hipMemcpyAsync(status + base, o.status, n, hipMemcpyDeviceToHost, ctx->stream));
            SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        for (size_t i = 0; i < n; i++) {
            if (status[base + i]) continue;  // reported, not proved: its system is unsatisfied
            size_t len = 0;
            SWM_TRY(pg_prove_item(ctx, pk, s, inputs ? inputs + (base + i) * s.input_bytes : nullptr,
                                  outputs ? outputs + (base + i) * s.output_bytes : nullptr,
                                  reinterpret_cast<const Fr*>(o.w) + i * s.num_witness, rng, flags, proofs_out + (base + i) * proof_cap, proof_cap,
                                  &len));
            lens[base + i] = len;
        }
    }
    return SWM_OK;
}

}  // extern "C"

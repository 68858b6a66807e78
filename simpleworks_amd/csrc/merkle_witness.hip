// merkle_witness.hip — the witness of the Pedersen Merkle-membership circuit, synthesised on the GPU: the step between
// swm_merkle_tree_build (pedersen.hip) and swm_generate_proof (marlin.hip).
//
// What the reference does there: SimpleMerkleTree::prove (src/merkle_tree/simple_merkle_tree.rs:105-123) builds a
// MerkleTreeVerificationU8 and MarlinInst::prove runs its generate_constraints into a fresh constraint system — the whole
// circuit, on one CPU thread, per proof.  The prover reads only the ASSIGNMENT of that system (the matrices are the key's), and
// the circuit's shape depends on the tree height alone, so what is left per proof is the witness vector.  Its order and values
// are those of simpleworks_amd/workloads.py, build_merkle_membership (digest_bits = 256): that function is the specification,
// host/merkle_shape.h the offsets.
//
// On the GPU: one workgroup of 128 lanes per path, one lane per 4-bit window of a two-to-one hash (the leaf hash uses two).
// Every witness of a hash is a pointwise function of the affine prefix sums P_k = sum_{i <= k} bit_i G_i:
//   1. lane w looks its window's point up in the resident table of swm_pedersen (one mixed addition from the identity);
//   2. an exclusive scan of the 128 window points with the unified addition: shuffles inside a wave, LDS between the two;
//   3. from its prefix each lane walks its four bits with mixed additions against the rows 1 << j: the 512 running sums;
//   4. ONE inversion normalises all 512: products of four Z per lane, a prefix and a suffix product scan over the lanes, the
//      inverse of the total on one lane (frinv.cuh), three multiplications back to each lane's product and six to its four Z;
//   5. the six witnesses of step k — t = X Y, b t, m1, m2, X3, Y3 — from P_{k-1}, P_k and the generator's (cx, cy), which the
//      table row 1 << j gives as ((y + x) -+ (y - x)) / 2.
// The law is complete (ed.cuh): identity windows, zero bits and repeated points take the same path and no Z is zero.
// Only the levels of a path are sequential (a level hashes the digest of the one below).  The byte-operation block is a
// table-driven walk over plain bytes in LDS — its schedule depends on (levels, operations) only — expanded to 0/1 elements.
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "context.h"
#include "ed.cuh"
#include "ff.cuh"
#include "frinv.cuh"
#include "host/merkle_shape.h"
#include "pedersen.h"
#include "swmarlin.h"

struct swm_merkle_circuit {
    const swm_pedersen* leaf = nullptr;
    const swm_pedersen* inner = nullptr;
    swm::MerkleShape shape;
    swm::MerkleByteOp* d_ops = nullptr;  // shape.ops entries (null when there are none)
};

namespace swm {

static constexpr unsigned MW_LANES = 128;  // = windows of a two-to-one hash

struct MwShared {
    EdExt wave_total;             // sum of wave 0's window points
    Fr cross[2];                  // wave 0's Z product | wave 1's; then the inverse of the total
    Fr last_x[MW_LANES], last_y[MW_LANES];  // each lane's last affine running sum (the next lane's P_{k-1})
    MerkleByteOp stage[MW_LANES];
    uint32_t bits[16];            // left || right of the level, canonical little-endian words
    uint32_t cur[8];              // the running digest, canonical
    uint32_t bad;
};

__device__ __forceinline__ Fr fr_shfl_up(const Fr& a, unsigned d) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)__shfl_up((int)a.v[i], d, 64);
    return r;
}
__device__ __forceinline__ Fr fr_shfl_down(const Fr& a, unsigned d) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)__shfl_down((int)a.v[i], d, 64);
    return r;
}
__device__ __forceinline__ EdExt ed_shfl_up(const EdExt& p, unsigned d) {
    EdExt r;
    r.x = fr_shfl_up(p.x, d);
    r.y = fr_shfl_up(p.y, d);
    r.t = fr_shfl_up(p.t, d);
    r.z = fr_shfl_up(p.z, d);
    return r;
}

// One Pedersen hash of `nbits` bits (4 per lane; `nib` is zero on the lanes past the input) with the witnesses of its
// conditional additions: step k = 1 .. nbits - 1 at out[6 (k - 1) .. + 6).  Leaves the digest, canonical, in sh.cur (the caller
// synchronises before reading it).  Called by all 128 lanes.
__device__ __noinline__ void mw_hash_stage(const EdRow* __restrict__ table, unsigned nib, unsigned nbits, Fr* __restrict__ out,
                                           const Fr k2d, const Fr half, MwShared& sh) {
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const EdRow* rows = table + ((size_t)tid << 4);  // only read where nib has a bit: never past the windows the input fills
    // 1. + 2.
    EdExt acc = ed_identity();
    if (nib) ed_madd(acc, rows[nib]);
#pragma unroll 1
    for (unsigned d = 1; d < 64; d <<= 1) {
        const EdExt o = ed_shfl_up(acc, d);
        if (lane >= d) acc = ed_add(o, acc, k2d);
    }
    if (tid == 63) sh.wave_total = acc;
    __syncthreads();
    if (wave) acc = ed_add(sh.wave_total, acc, k2d);
    EdExt q = ed_shfl_up(acc, 1);
    if (lane == 0) q = wave ? sh.wave_total : ed_identity();
    // 3.
    Fr px[4], py[4], pz[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if ((nib >> j) & 1u) ed_madd(q, rows[1u << j]);
        px[j] = q.x;
        py[j] = q.y;
        pz[j] = q.z;
    }
    // 4.
    const Fr a1 = fp_mul(pz[0], pz[1]), a2 = fp_mul(a1, pz[2]), prod = fp_mul(a2, pz[3]);
    Fr pre = prod, suf = prod;  // inclusive products over the lanes below / above
#pragma unroll 1
    for (unsigned d = 1; d < 64; d <<= 1) {
        const Fr o = fr_shfl_up(pre, d);
        const Fr u = fr_shfl_down(suf, d);
        if (lane >= d) pre = fp_mul(o, pre);
        if (lane + d < 64) suf = fp_mul(u, suf);
    }
    if (tid == 63) sh.cross[0] = pre;
    if (tid == 64) sh.cross[1] = suf;
    __syncthreads();
    if (wave) pre = fp_mul(sh.cross[0], pre);
    else suf = fp_mul(suf, sh.cross[1]);
    Fr below = fr_shfl_up(pre, 1), above = fr_shfl_down(suf, 1);  // exclusive
    if (lane == 0) below = wave ? sh.cross[0] : fp_one<Fr>();
    if (lane == 63) above = wave ? fp_one<Fr>() : sh.cross[1];
    __syncthreads();  // cross[] has been read
    if (tid == MW_LANES - 1) sh.cross[0] = fr_inv_single(pre);  // the total: no Z is zero
    __syncthreads();
    const Fr inv_prod = fp_mul(fp_mul(below, above), sh.cross[0]);
    Fr iz[4];
    iz[3] = fp_mul(inv_prod, a2);
    const Fr inv_a2 = fp_mul(inv_prod, pz[3]);
    iz[2] = fp_mul(inv_a2, a1);
    const Fr inv_a1 = fp_mul(inv_a2, pz[2]);
    iz[1] = fp_mul(inv_a1, pz[0]);
    iz[0] = fp_mul(inv_a1, pz[1]);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        px[j] = fp_mul(px[j], iz[j]);
        py[j] = fp_mul(py[j], iz[j]);
    }
    sh.last_x[tid] = px[3];
    sh.last_y[tid] = py[3];
    __syncthreads();
    // 5.
    Fr X = tid ? sh.last_x[tid - 1] : fp_zero<Fr>();
    Fr Y = tid ? sh.last_y[tid - 1] : fp_one<Fr>();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned k = 4 * tid + j;
        if (k >= 1 && k < nbits) {  // the first bit of a hash is linear in the bit: no witness
            Fr* o = out + MW_COND_ADD * (size_t)(k - 1);
            const Fr t = fp_mul(X, Y);
            o[0] = t;
            if ((nib >> j) & 1u) {
                const EdRow g = rows[1u << j];
                const Fr cx = fp_mul(half, fp_sub(g.ypx, g.ymx)), cy = fp_mul(half, fp_add(g.ypx, g.ymx));
                const Fr cym1 = fp_sub(cy, fp_one<Fr>());
                o[1] = t;
                o[2] = fp_add(fp_mul(cym1, X), fp_mul(cx, Y));
                o[3] = fp_add(fp_mul(cym1, Y), fp_mul(cx, X));
            } else {
                o[1] = fp_zero<Fr>();
                o[2] = fp_zero<Fr>();
                o[3] = fp_zero<Fr>();
            }
            o[4] = px[j];
            o[5] = py[j];
        }
        X = px[j];
        Y = py[j];
    }
    if (tid == MW_LANES - 1) {  // lanes past the input carry the total along: the last lane always holds the hash
        const Fr x = fp_to_std(px[3]);
#pragma unroll
        for (int i = 0; i < 8; i++) sh.cur[i] = x.v[i];
    }
}

// Block p = path p.  pool (dynamic LDS): 64 levels + ops bytes.
__global__ void __launch_bounds__(MW_LANES) merkle_witness_kernel(const EdRow* __restrict__ leaf_table, const EdRow* __restrict__ inner_table,
                                                                  unsigned levels, unsigned ops, const MerkleByteOp* __restrict__ op_table,
                                                                  size_t num_witness, size_t ops_at, const uint8_t* __restrict__ leaves,
                                                                  const uint64_t* __restrict__ indices, const uint8_t* __restrict__ siblings,
                                                                  Fr* __restrict__ witness, uint8_t* __restrict__ roots,
                                                                  uint32_t* __restrict__ status, Fr k2d, Fr half) {
    extern __shared__ __align__(16) uint8_t pool[];
    __shared__ MwShared sh;
    const unsigned tid = threadIdx.x;
    const size_t path = blockIdx.x;
    Fr* w = witness + path * num_witness;
    const uint32_t* sib = reinterpret_cast<const uint32_t*>(siblings + path * (size_t)levels * 32);
    const uint64_t index = indices[path];
    const Fr one = fp_one<Fr>(), zero = fp_zero<Fr>();

    // what the host form refuses: a sibling that is no canonical field element, an index beyond the leaves
    if (tid == 0) sh.bad = (index >> levels) ? 2u : 0u;  // levels <= 63
    __syncthreads();
    for (unsigned lvl = tid; lvl < levels; lvl += MW_LANES) {
        Fr s, r;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            s.v[i] = sib[8 * lvl + i];
            r.v[i] = FrParams::P[i];
        }
        if (fp_cmp_std(s, r) >= 0) atomicOr(&sh.bad, 1u);
    }
    __syncthreads();
    const uint32_t bad = sh.bad;
    if (bad) {
        uint4* wz = reinterpret_cast<uint4*>(w);
        for (size_t i = tid; i < 2 * num_witness; i += MW_LANES) wz[i] = make_uint4(0, 0, 0, 0);
        if (roots && tid < 8) reinterpret_cast<uint32_t*>(roots + 32 * path)[tid] = 0;
        if (status && tid == 0) status[path] = (bad & 1u) ? 1u : 2u;
        return;
    }
    if (status && tid == 0) status[path] = 0;

    // leaf hash: 8 bits, two windows
    const unsigned leaf = leaves[path];
    mw_hash_stage(leaf_table, tid < 2 ? (leaf >> (4 * tid)) & 15u : 0u, (unsigned)MW_LEAF_BITS, w, k2d, half, sh);
    __syncthreads();

    for (unsigned lvl = 0; lvl < levels; lvl++) {
        const unsigned dir = (unsigned)(index >> lvl) & 1u;
        if (tid < 8) {  // left = dir ? sibling : cur, right = the other one
            const uint32_t s = sib[8 * lvl + tid], c = sh.cur[tid];
            sh.bits[tid] = dir ? s : c;
            sh.bits[8 + tid] = dir ? c : s;
        }
        __syncthreads();
        Fr* lw = w + MW_LEAF_WITNESSES + MW_LEVEL_WITNESSES * (size_t)lvl;
        if (tid == 0) {
            Fr s, l;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                s.v[i] = sib[8 * lvl + i];
                l.v[i] = sh.bits[i];
            }
            lw[0] = dir ? one : zero;
            lw[1] = fp_from_std(s);
            lw[2] = fp_from_std(l);
        }
        for (unsigned i = tid; i < 2 * MW_DIGEST_BITS; i += MW_LANES) lw[MW_LEVEL_BITS_AT + i] = (sh.bits[i >> 5] >> (i & 31)) & 1u ? one : zero;
        if (tid < 16) reinterpret_cast<uint32_t*>(pool)[16 * lvl + tid] = sh.bits[tid];
        const unsigned nib = (sh.bits[tid >> 3] >> (4 * (tid & 7))) & 15u;
        mw_hash_stage(inner_table, nib, 2 * (unsigned)MW_DIGEST_BITS, lw + MW_LEVEL_ADDS_AT, k2d, half, sh);
        __syncthreads();
    }
    if (roots && tid < 8) reinterpret_cast<uint32_t*>(roots + 32 * path)[tid] = sh.cur[tid];

    // byte operations: results depend on earlier results, so one lane walks the schedule; the table comes in by 128 entries
    const unsigned base_len = 64 * levels;
    for (unsigned base = 0; base < ops; base += MW_LANES) {
        if (base + tid < ops) sh.stage[tid] = op_table[base + tid];
        __syncthreads();
        if (tid == 0) {
            const unsigned n = min(MW_LANES, ops - base);
            for (unsigned i = 0; i < n; i++) {
                const MerkleByteOp e = sh.stage[i];
                const unsigned a = pool[e.a], b = pool[e.b];
                const unsigned r = e.kind == 0 ? (a << e.shift) & 0xFFu : e.kind == 1 ? a ^ b : a & b;
                pool[base_len + base + i] = (uint8_t)r;
            }
        }
        __syncthreads();
    }
    Fr* ow = w + ops_at;
    for (unsigned i = tid; i < 8 * ops; i += MW_LANES) ow[i] = (pool[base_len + (i >> 3)] >> (i & 7)) & 1u ? one : zero;
}

static bool std_canonical(const uint8_t* b) {  // 32 little-endian bytes < r
    Fr s, r;
    for (int i = 0; i < 8; i++) {
        s.v[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
        r.v[i] = FrParams::P[i];
    }
    return fp_cmp_std(s, r) < 0;
}

static int merkle_witness_run(swm_ctx* ctx, const swm_merkle_circuit* c, const uint8_t* d_leaves, const uint64_t* d_indices,
                              const uint8_t* d_siblings, size_t count, Fr* d_witness, uint8_t* d_roots, uint32_t* d_status) {
    if (!count) return SWM_OK;
    if (count > 0x7FFFFFFFu) return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_witness: %zu paths in one call", count);
    const MerkleShape& s = c->shape;
    const size_t lds = (64 * s.levels + s.ops + 15) & ~(size_t)15;
    SWM_LAUNCH(ctx, "merkle_witness", merkle_witness_kernel, dim3((unsigned)count), dim3(MW_LANES), lds,
               reinterpret_cast<const EdRow*>(c->leaf->d_table), reinterpret_cast<const EdRow*>(c->inner->d_table), (unsigned)s.levels,
               (unsigned)s.ops, c->d_ops, s.num_witness, s.ops_at, d_leaves, d_indices, d_siblings, d_witness, d_roots, d_status,
               fp_from_u64<Fr>(2 * ED_D), fp_inv(fp_from_u64<Fr>(2)));
    return SWM_OK;
}

// the host form's checks: what the device form reports per path
static int merkle_check_paths(swm_ctx* ctx, const swm_merkle_circuit* c, const uint64_t* indices, const uint8_t* siblings, size_t count) {
    const size_t L = c->shape.levels;
    for (size_t p = 0; p < count; p++) {
        if (indices[p] >> L) return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_witness: path %zu: leaf index %llu in a tree of 2^%zu leaves", p,
                                            (unsigned long long)indices[p], L);
        for (size_t l = 0; l < L; l++)
            if (!std_canonical(siblings + 32 * (p * L + l)))
                return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_witness: path %zu: the sibling of level %zu is not a canonical field element", p, l);
    }
    return SWM_OK;
}

// inputs of `count` paths into one staging buffer: indices | siblings | leaves
static int merkle_stage_inputs(swm_ctx* ctx, const swm_merkle_circuit* c, const uint8_t* leaves, const uint64_t* indices,
                               const uint8_t* siblings, size_t count, const uint8_t** d_leaves, const uint64_t** d_indices,
                               const uint8_t** d_siblings) {
    const size_t L = c->shape.levels;
    uint8_t* d_in = nullptr;
    SWM_TRY(scratch(ctx, "stage.a", count * (8 + 32 * L + 1), (void**)&d_in));
    SWM_HIP(ctx, hipMemcpyAsync(d_in, indices, 8 * count, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(d_in + 8 * count, siblings, 32 * L * count, hipMemcpyHostToDevice, ctx->stream));
    SWM_HIP(ctx, hipMemcpyAsync(d_in + (8 + 32 * L) * count, leaves, count, hipMemcpyHostToDevice, ctx->stream));
    *d_indices = reinterpret_cast<const uint64_t*>(d_in);
    *d_siblings = d_in + 8 * count;
    *d_leaves = d_in + (8 + 32 * L) * count;
    return SWM_OK;
}

}  // namespace swm

using namespace swm;

extern "C" {

int swm_merkle_circuit_create(swm_ctx* ctx, const swm_pedersen* leaf, const swm_pedersen* inner, size_t height, size_t gadget_byte_ops,
                              swm_merkle_circuit** out) {
    if (!ctx || !leaf || !inner || !out) return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_circuit_create: bad arguments");
    MerkleShape shape;
    if (!merkle_shape(height, gadget_byte_ops, &shape))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_circuit_create: height %zu (2 <= height <= %zu)", height, (size_t)MW_MAX_HEIGHT);
    if (leaf->window_size != 4 || inner->window_size != 4)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_circuit_create: windows of %u and %u bits (4 is required)", leaf->window_size,
                       inner->window_size);
    if (leaf->num_windows < 2 || inner->num_windows < 128)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_circuit_create: %u leaf and %u two-to-one windows (at least 2 and 128 are required)",
                       leaf->num_windows, inner->num_windows);
    std::vector<MerkleByteOp> table;
    if (!merkle_op_table(shape.levels, shape.ops, &table))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_circuit_create: %zu byte operations over %zu levels exceed the pool of %zu bytes",
                       gadget_byte_ops, shape.levels, (size_t)MW_MAX_POOL);
    SWM_ON_DEVICE(ctx);
    std::unique_ptr<swm_merkle_circuit> c(new swm_merkle_circuit);
    c->leaf = leaf;
    c->inner = inner;
    c->shape = shape;
    if (!table.empty()) {
        hipError_t e = hipMalloc((void**)&c->d_ops, table.size() * sizeof(MerkleByteOp));
        if (e == hipSuccess) e = hipMemcpyAsync(c->d_ops, table.data(), table.size() * sizeof(MerkleByteOp), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // `table` goes out of scope
        if (e != hipSuccess) {
            if (c->d_ops) (void)hipFree(c->d_ops);
            (void)hipGetLastError();
            return set_err(ctx, e == hipErrorOutOfMemory ? SWM_ERR_OOM : SWM_ERR_HIP, "merkle_circuit_create: %s", hipGetErrorString(e));
        }
    }
    *out = c.release();
    return SWM_OK;
}

void swm_merkle_circuit_destroy(swm_ctx* ctx, swm_merkle_circuit* c) {
    if (!c) return;
    DeviceGuard guard(ctx);
    if (ctx) drain_streams(ctx);
    if (c->d_ops) (void)hipFree(c->d_ops);
    delete c;
}

int swm_merkle_witness_dev(swm_ctx* ctx, const swm_merkle_circuit* c, const void* d_leaves, const void* d_indices, const void* d_siblings,
                           size_t count, void* d_witness, void* d_roots, void* d_status) {
    if (!ctx || !c || (count && (!d_leaves || !d_indices || !d_siblings || !d_witness)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_witness: bad arguments");
    SWM_ON_DEVICE(ctx);
    return merkle_witness_run(ctx, c, (const uint8_t*)d_leaves, (const uint64_t*)d_indices, (const uint8_t*)d_siblings, count, (Fr*)d_witness,
                              (uint8_t*)d_roots, (uint32_t*)d_status);
}

int swm_merkle_witness(swm_ctx* ctx, const swm_merkle_circuit* c, const uint8_t* leaves, const uint64_t* indices, const uint8_t* siblings,
                       size_t count, uint64_t* witness, uint8_t* roots) {
    if (!ctx || !c || (count && (!leaves || !indices || !siblings || !witness)))
        return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_witness: bad arguments");
    if (!count) return SWM_OK;
    SWM_TRY(merkle_check_paths(ctx, c, indices, siblings, count));
    SWM_ON_DEVICE(ctx);
    const uint8_t *d_leaves, *d_siblings;
    const uint64_t* d_indices;
    SWM_TRY(merkle_stage_inputs(ctx, c, leaves, indices, siblings, count, &d_leaves, &d_indices, &d_siblings));
    const size_t wbytes = count * c->shape.num_witness * sizeof(Fr);
    uint8_t* d_out = nullptr;
    SWM_TRY(scratch(ctx, "merkle.w", wbytes + 32 * count, (void**)&d_out));
    SWM_TRY(merkle_witness_run(ctx, c, d_leaves, d_indices, d_siblings, count, (Fr*)d_out, d_out + wbytes, nullptr));
    SWM_HIP(ctx, hipMemcpyAsync(witness, d_out, wbytes, hipMemcpyDeviceToHost, ctx->stream));
    if (roots) SWM_HIP(ctx, hipMemcpyAsync(roots, d_out + wbytes, 32 * count, hipMemcpyDeviceToHost, ctx->stream));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWM_OK;
}

int swm_merkle_prove(swm_ctx* ctx, const swm_pk* pk, const swm_merkle_circuit* c, const uint8_t root[32], uint8_t leaf, uint64_t index,
                     const uint8_t* siblings, swm_rng* rng, unsigned flags, uint8_t* proof_out, size_t cap, size_t* len) {
    if (!ctx || !pk || !c || !root || !siblings || !rng || !proof_out || !len)
        return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_prove: bad arguments");
    if (!std_canonical(root)) return set_err(ctx, SWM_ERR_INVALID_ARG, "merkle_prove: the root is not a canonical field element");
    SWM_TRY(merkle_check_paths(ctx, c, &index, siblings, 1));
    const MerkleShape& s = c->shape;
    Fr* d_w = nullptr;
    {
        SWM_ON_DEVICE(ctx);
        const uint8_t *d_leaves, *d_siblings;
        const uint64_t* d_indices;
        SWM_TRY(scratch(ctx, "merkle.w", s.num_witness * sizeof(Fr) + 32, (void**)&d_w));
        SWM_TRY(merkle_stage_inputs(ctx, c, &leaf, &index, siblings, 1, &d_leaves, &d_indices, &d_siblings));
        SWM_TRY(merkle_witness_run(ctx, c, d_leaves, d_indices, d_siblings, 1, d_w, nullptr, nullptr));
        SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `leaf` and `index` were staged from this frame
    }
    // public input: one, root, the 8 leaf bits (src/merkle_tree/simple_merkle_tree.rs:129-143)
    Fr inst[MW_NUM_INSTANCE];
    inst[0] = fp_one<Fr>();
    Fr r;
    for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)root[4 * i] | (uint32_t)root[4 * i + 1] << 8 | (uint32_t)root[4 * i + 2] << 16 | (uint32_t)root[4 * i + 3] << 24;
    inst[1] = fp_from_std(r);
    for (int i = 0; i < 8; i++) inst[2 + i] = (leaf >> i) & 1 ? fp_one<Fr>() : fp_zero<Fr>();
    swm_r1cs cs = {};
    cs.num_instance = s.num_instance;
    cs.num_witness = s.num_witness;
    cs.num_constraints = s.num_constraints;
    cs.instance = reinterpret_cast<const uint64_t*>(inst);
    cs.witness = reinterpret_cast<const uint64_t*>(d_w);  // never read on the host: the context carries the device source
    struct DevWitnessScope {
        swm_ctx* c;
        ~DevWitnessScope() { c->witness_dev = nullptr; }
    } scope{ctx};
    ctx->witness_dev = d_w;
    return swm_generate_proof_ex(ctx, pk, &cs, rng, flags, proof_out, cap, len);
}

}  // extern "C"

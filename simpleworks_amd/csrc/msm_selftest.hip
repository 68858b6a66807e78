// msm_selftest.hip — the point-layer self-test of the G1 MSM (msm.h: selftest_p28_run; include/swmarlin.h: swm_selftest_p28): test
// surface, kept out of the units that hold the hot kernels.  (The sort stage's self-test, msm_selftest_sort, is the driver's own
// path and lives in msm.hip.)
#include "context.h"
#include "fq28.cuh"
#include "fq29.cuh"
#include "g1.cuh"
#include "msm_points.cuh"
#include "msm_stages.h"

namespace swm {

// ---------------------------------------------------------------------------------------------- point-layer self-test
// The routines of the 28-bit point layer (fq28.cuh and the streamed forms of msm_points.cuh), one call per element on operands the CALLER
// chose limb for limb (include/swmarlin.h: swm_selftest_p28 names the ops).  a, b, out: raw slots of the 28-bit domain (a row
// operand: the 192 bytes of a G1TE); flags: bit 0 = the sign / `act` bit of the element, bit 1 = the sign of madd28's second point.
enum : int {
    P28T_DBL = 0, P28T_ADD, P28T_ADD_OOL, P28T_SLOT_ADD, P28T_SLOT_ADD_INPLACE, P28T_SLOT_DBL, P28T_STORE_384, P28T_MADD28,
    P28T_ROWS, P28T_TE_FROM_ROW, P28T_TE_MADD_ROW, P28T_TE_SLOT_ADD, P28T_TE_SLOT_ADD_INPLACE, P28T_TE_SLOT_ADD_SELF,
    P28T_TE_SLOT_ADD_SYNC, P28T_TE_STORE_384, P28T_QUAD_FROM_ROW, P28T_QUAD_MADD_ROW, P28T_QUAD_ADD, P28T_QUAD_ADD_SELF,
    P28T_QUAD_STORE_IDENTITY, P28T_ROWS29, P28T_TE29_FROM_ROW, P28T_TE29_MADD_ROW, P28T_TE29_QUAD_FROM_ROW, P28T_TE29_QUAD_MADD_ROW,
    P28T_TE29_TO_SLOT,
    // the general addition of the 29-bit domain (fq29.cuh): a, b, out are raw points in the transport form of the te29_* ops above
    // (twelve words per coordinate, fq29_unpack_raw / fq29_pack), moved into TE29Pt memory for the routine under test
    P28T_TE29_SLOT_ADD, P28T_TE29_SLOT_ADD_INPLACE_A, P28T_TE29_SLOT_ADD_INPLACE_Q, P28T_TE29_SLOT_ADD_SELF, P28T_TE29_SLOT_ADD_SYNC,
    P28T_TE29_QUAD_ADD, P28T_TE29_QUAD_ADD_SELF, P28T_TE29_STORE_IDENTITY, P28T_TE29_QUAD_STORE_IDENTITY, P28T_TE29_STORE_384, P28T_COUNT
};
// The te29 ops (fq29.cuh) take and return RAW accumulators of the 29-bit domain: four 12-word integers, a field element times
// 2^406 each, any representative whose thirteenth limb (bits 348 ..) fits 32 bits.
__device__ __forceinline__ Fq29 fq29_unpack_raw(const Fq& a) {
    Fq29 r = fq29_unpack(a);
    r.l[12] = (a.v[10] >> 28) | (a.v[11] << 4);
    return r;
}
__device__ __forceinline__ T29 t29_load(const G1XYZZ& m) {
    T29 r;
    r.x = fq29_unpack_raw(m.x);
    r.y = fq29_unpack_raw(m.y);
    r.t = fq29_unpack_raw(m.zz);
    r.z = fq29_unpack_raw(m.zzz);
    return r;
}
__device__ __forceinline__ void t29_store(G1XYZZ& m, const T29& p) {  // (fq29_pack keeps a top limb above 2^29: it is shifted, not masked)
    m.x = fq29_pack(p.x);
    m.y = fq29_pack(p.y);
    m.zz = fq29_pack(p.t);
    m.zzz = fq29_pack(p.z);
}
__device__ __forceinline__ T28 t28_load(const G1XYZZ& m) {
    T28 r;
    r.x = fq28_unpack(m.x);
    r.y = fq28_unpack(m.y);
    r.t = fq28_unpack(m.zz);
    r.z = fq28_unpack(m.zzz);
    return r;
}
__device__ __forceinline__ void t28_store(G1XYZZ& m, const T28& p) {
    m.x = fq28_pack(p.x);
    m.y = fq28_pack(p.y);
    m.zz = fq28_pack(p.t);
    m.zzz = fq28_pack(p.z);
}
__global__ void __launch_bounds__(256) selftest_p28_kernel(int op, const G1XYZZ* a, const G1XYZZ* b, const uint32_t* flags, G1XYZZ* out,
                                                           uint32_t* status, size_t n) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    const bool live = i < n;
    const uint32_t fl = live ? flags[i] : 0u;
    if (op == P28T_TE_SLOT_ADD_SYNC) {  // every lane of the workgroup reaches the barrier; the lanes past n and those without the bit sit out
        const size_t j = live ? i : 0;
        te28_slot_add_sync(&out[j], &a[j], &b[j], live && (fl & 1u) != 0, true);
        return;
    }
    if (!live) return;
    const bool neg = (fl & 1u) != 0;
    switch (op) {
    case P28T_DBL:
        p28_store(out[i], p28_dbl<MulInline>(p28_load(a[i])));
        break;
    case P28T_ADD: {
        P28 p = p28_load(a[i]);
        p28_add<MulInline>(p, p28_load(b[i]));
        p28_store(out[i], p);
        break;
    }
    case P28T_ADD_OOL: {
        P28 p = p28_load(a[i]);
        p28_add_ool(p, p28_load(b[i]));
        p28_store(out[i], p);
        break;
    }
    case P28T_SLOT_ADD:
        p28_slot_add(&out[i], &a[i], &b[i]);
        break;
    case P28T_SLOT_ADD_INPLACE:
        out[i] = a[i];
        p28_slot_add(&out[i], &out[i], &b[i]);
        break;
    case P28T_SLOT_DBL:
        p28_slot_dbl(&out[i], &a[i]);
        break;
    case P28T_STORE_384:
        p28_store_384(out[i], p28_load(a[i]));
        break;
    case P28T_MADD28: {
        // the first entry of a segment and the operand of every later one, as msm_accumulate forms them: slots x, y of a and of b
        // hold two affine points of the scaled base set
        Acc28 acc;
        acc.x = fq28_unpack(a[i].x);
        Fq28 y = fq28_unpack(a[i].y);
        if (neg) {
            Fq28 z;
#pragma unroll
            for (int k = 0; k < 14; k++) z.l[k] = Fq28Consts::SPREAD4[k] - y.l[k];
            y = fq28_normalize(z);
        }
        acc.y = y;
        acc.zz = fq28_const(Fq28Consts::ONE);
        acc.zzz = acc.zz;
        Fq28 x2 = fq28_unpack(b[i].x), y2 = fq28_unpack(b[i].y);
        if (fl & 2u) {
#pragma unroll
            for (int k = 0; k < 14; k++) y2.l[k] = Fq28Consts::SPREAD4[k] - y2.l[k];
        }
        status[i] = madd28(acc, x2, y2) ? 1u : 0u;
        P28 o{acc.x, acc.y, acc.zz, acc.zzz};
        p28_store(out[i], o);
        break;
    }
    case P28T_TE_FROM_ROW: {
        const G1TE* row = reinterpret_cast<const G1TE*>(&a[i]);
        t28_store(out[i], te28_from_row(te28_load_coord(row->ymx), te28_load_coord(row->ypx), te28_load_coord(row->kt), neg));
        break;
    }
    case P28T_TE_MADD_ROW: {
        T28 acc = t28_load(a[i]);
        te28_madd_row(acc, reinterpret_cast<const G1TE*>(&b[i]), neg);
        t28_store(out[i], acc);
        break;
    }
    case P28T_TE_SLOT_ADD:
        te28_slot_add(&out[i], &a[i], &b[i]);
        break;
    case P28T_TE_SLOT_ADD_INPLACE:
        out[i] = a[i];
        te28_slot_add(&out[i], &out[i], &b[i]);
        break;
    case P28T_TE_SLOT_ADD_SELF:
        te28_slot_add(&out[i], &a[i], &a[i]);
        break;
    case P28T_TE_STORE_384:
        te28_store_384(out[i], a[i]);
        break;
    case P28T_TE29_FROM_ROW: {
        const G1TE* row = reinterpret_cast<const G1TE*>(&a[i]);
        t29_store(out[i], te29_from_row(te29_load_coord(row->ymx), te29_load_coord(row->ypx), te29_load_coord(row->kt), neg));
        break;
    }
    case P28T_TE29_MADD_ROW: {
        T29 acc = t29_load(a[i]);
        te29_madd_row(acc, reinterpret_cast<const G1TE*>(&b[i]), neg);
        t29_store(out[i], acc);
        break;
    }
    case P28T_TE29_TO_SLOT: {  // the epilogue of msm_accumulate_te
        const T29 acc = t29_load(a[i]);
        out[i].x = te29_to_slot(acc.x);
        out[i].y = te29_to_slot(acc.y);
        out[i].zz = te29_to_slot(acc.t);
        out[i].zzz = te29_to_slot(acc.z);
        break;
    }
    default:
        break;
    }
}
// the quad forms: four lanes per element, every lane handed the same pointers
__global__ void __launch_bounds__(256) selftest_p28_quad_kernel(int op, const G1XYZZ* a, const G1XYZZ* b, const uint32_t* flags,
                                                                G1XYZZ* out, size_t n) {
    const size_t i = (blockIdx.x * (size_t)256 + threadIdx.x) >> 2;
    const unsigned q = threadIdx.x & 3u;
    if (i >= n) return;  // (uniform over a quad)
    const bool neg = (flags[i] & 1u) != 0;
    switch (op) {
    case P28T_QUAD_FROM_ROW:
        reinterpret_cast<Fq*>(&out[i])[q] = fq28_pack(te28_quad_from_row(reinterpret_cast<const G1TE*>(&a[i]), neg, q));
        break;
    case P28T_QUAD_MADD_ROW: {
        Fq28 own = fq28_unpack(reinterpret_cast<const Fq*>(&a[i])[q]);
        te28_quad_madd_row(own, reinterpret_cast<const G1TE*>(&b[i]), neg, q);
        reinterpret_cast<Fq*>(&out[i])[q] = fq28_pack(own);
        break;
    }
    case P28T_QUAD_ADD:
        te28_quad_add(&out[i], &a[i], &b[i], q);
        break;
    case P28T_QUAD_ADD_SELF:
        te28_quad_add(&out[i], &a[i], &a[i], q);
        break;
    case P28T_QUAD_STORE_IDENTITY:
        te28_quad_store_identity(&out[i], q);
        break;
    case P28T_TE29_QUAD_FROM_ROW:
        reinterpret_cast<Fq*>(&out[i])[q] = fq29_pack(te29_quad_from_row(reinterpret_cast<const G1TE*>(&a[i]), neg, q));
        break;
    case P28T_TE29_QUAD_MADD_ROW: {
        Fq29 own = fq29_unpack_raw(reinterpret_cast<const Fq*>(&a[i])[q]);
        te29_quad_madd_row(own, reinterpret_cast<const G1TE*>(&b[i]), neg, q);
        reinterpret_cast<Fq*>(&out[i])[q] = fq29_pack(own);
        break;
    }
    default:
        break;
    }
}
// The general addition of the 29-bit domain on points at rest: ws holds 3 n TE29Pt (a | b | out).  Four lanes per element: each moves
// one coordinate in and out; lane 0 of the quad runs the one-lane routines, all four the quad ones.  Workgroup barriers separate the
// three steps (the routines read what other lanes wrote), so every lane stays to the end.
__global__ void __launch_bounds__(256) selftest_te29_tail_kernel(int op, const G1XYZZ* a, const G1XYZZ* b, const uint32_t* flags, G1XYZZ* out,
                                                                 TE29Pt* ws, size_t n) {
    const size_t i = (blockIdx.x * (size_t)256 + threadIdx.x) >> 2;
    const unsigned q = threadIdx.x & 3u;
    const bool live = i < n;
    const size_t j = live ? i : 0;
    TE29Pt *pa = ws + j, *pb = ws + n + j, *po = ws + 2 * n + j;
    if (live) {
        if (a) te29_pt_store_coord(pa, q, fq29_unpack_raw(reinterpret_cast<const Fq*>(&a[j])[q]));
        if (b) te29_pt_store_coord(pb, q, fq29_unpack_raw(reinterpret_cast<const Fq*>(&b[j])[q]));
        for (int k = 0; k < 13; k++) po->w[13 * q + k] = 0xA5A5A5A5u;
    }
    __syncthreads();
    const bool one = live && q == 0;
    switch (op) {
    case P28T_TE29_SLOT_ADD:
        if (one) te29_slot_add(po, pa, pb);
        break;
    case P28T_TE29_SLOT_ADD_INPLACE_A:
        if (one) te29_slot_add(pa, pa, pb), *po = *pa;
        break;
    case P28T_TE29_SLOT_ADD_INPLACE_Q:
        if (one) te29_slot_add(pb, pa, pb), *po = *pb;
        break;
    case P28T_TE29_SLOT_ADD_SELF:
        if (one) te29_slot_add(po, pa, pa);
        break;
    case P28T_TE29_SLOT_ADD_SYNC:  // every lane of the workgroup reaches the barrier inside; flag bit 0 = the element takes part
        te29_slot_add_sync(po, pa, pb, one && (flags[j] & 1u) != 0, true);
        break;
    case P28T_TE29_QUAD_ADD:
        if (live) te29_quad_add(po, pa, pb, q);
        break;
    case P28T_TE29_QUAD_ADD_SELF:
        if (live) te29_quad_add(po, pa, pa, q);
        break;
    case P28T_TE29_STORE_IDENTITY:
        if (one) te29_store_identity(po);
        break;
    case P28T_TE29_QUAD_STORE_IDENTITY:
        if (live) te29_quad_store_identity(po, q);
        break;
    case P28T_TE29_STORE_384:
        if (one) te29_store_384(out[j], *pa);
        break;
    default:
        break;
    }
    __syncthreads();
    const bool sat_out = op == P28T_TE29_SLOT_ADD_SYNC && (flags[j] & 1u) == 0;  // its slot keeps what the caller filled it with
    if (live && !sat_out && op != P28T_TE29_STORE_384) reinterpret_cast<Fq*>(&out[j])[q] = fq29_pack(te29_pt_load_coord(po, q));
}
// a twisted Edwards slot of the 28-bit domain -> the Weierstrass point it stands for, by the maps the bucket stage and the host
// fold apply to a total (te28_store_384, g1te_to_xyzz), as a Jacobian point in the memory form
// (from29: the slots hold a raw accumulator of the 29-bit domain, taken through the accumulation's epilogue first)
__global__ void __launch_bounds__(256) selftest_p28_backmap_kernel(const G1XYZZ* slots, G1Jac* out, size_t n, bool from29) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= n) return;
    G1XYZZ m, s = slots[i];
    if (from29) {
        const T29 acc = t29_load(s);
        s.x = te29_to_slot(acc.x);
        s.y = te29_to_slot(acc.y);
        s.zz = te29_to_slot(acc.t);
        s.zzz = te29_to_slot(acc.z);
    }
    te28_store_384(m, s);
    out[i] = g1_to_jacobian(g1te_to_xyzz(m));
}
int selftest_p28_run(swm_ctx* ctx, int op, const void* da, const void* db, const uint32_t* d_flags, void* d_out, void* d_jac,
                     void* d_pref, uint32_t* d_status, size_t n) {
    if (op < 0 || op >= P28T_COUNT) return set_err(ctx, SWM_ERR_INVALID_ARG, "selftest_p28: no such op");
    const unsigned grid = (unsigned)((n + 255) / 256);
    const bool quad = (op >= P28T_QUAD_FROM_ROW && op <= P28T_QUAD_STORE_IDENTITY) || op == P28T_TE29_QUAD_FROM_ROW ||
                      op == P28T_TE29_QUAD_MADD_ROW;
    if (op == P28T_ROWS || op == P28T_ROWS29) {
        SWM_TRY(msm_te_convert_run(ctx, op == P28T_ROWS29, (const G1Affine*)da, n, (Fq*)d_pref, (G1TE*)d_out, d_status));
    } else if (op >= P28T_TE29_SLOT_ADD) {
        TE29Pt* ws = nullptr;
        SWM_TRY(scratch(ctx, "stage.t29", 3 * n * sizeof(TE29Pt) + 64, (void**)&ws));
        SWM_LAUNCH(ctx, "selftest_te29_tail", selftest_te29_tail_kernel, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, op,
                   (const G1XYZZ*)da, (const G1XYZZ*)db, d_flags, (G1XYZZ*)d_out, ws, n);
    } else if (quad) {
        SWM_LAUNCH(ctx, "selftest_p28_quad", selftest_p28_quad_kernel, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, op,
                   (const G1XYZZ*)da, (const G1XYZZ*)db, d_flags, (G1XYZZ*)d_out, n);
    } else {
        SWM_LAUNCH(ctx, "selftest_p28", selftest_p28_kernel, dim3(grid), dim3(256), 0, op, (const G1XYZZ*)da, (const G1XYZZ*)db, d_flags,
                   (G1XYZZ*)d_out, d_status, n);
    }
    if (d_jac)
        SWM_LAUNCH(ctx, "selftest_p28_backmap", selftest_p28_backmap_kernel, dim3(grid), dim3(256), 0, (const G1XYZZ*)d_out, (G1Jac*)d_jac, n,
                   (op >= P28T_TE29_FROM_ROW && op <= P28T_TE29_QUAD_MADD_ROW) ||
                       (op >= P28T_TE29_SLOT_ADD && op <= P28T_TE29_QUAD_STORE_IDENTITY));
    return SWM_OK;
}

}  // namespace swm

// msm_stages.hip — the point stages of the G1 MSM (stages 4 - 6 of msm.hip's list): the accumulation of the ordered segments into
// partial sums (msm_accumulate, msm_accumulate_te, msm_accumulate_te_quad), the fold of oversized buckets (msm_big_bucket_sum) and
// the bucket stage (msm_bucket_reduce, msm_bucket_reduce_low).  The point routines and slot types are msm_points.cuh's; the driver
// (msm.hip) shapes the stages, fills the TailBatch and owns streams, events and result slots; the two functions at the end of this
// file launch on the context's stream.
#include <algorithm>
#include "context.h"
#include "fq28.cuh"
#include "fq29.cuh"
#include "g1.cuh"
#include "msm_points.cuh"
#include "msm_stages.h"

namespace swm {

// ---------------------------------------------------------------------------------------------- accumulation
// Dominant kernel: one lane per segment, XYZZ accumulator in registers, affine bases gathered from HBM/L2.
// (The inner loop, its 28-bit representation and its bounds: madd28, msm_points.cuh.)
__global__ void __launch_bounds__(256, 3) msm_accumulate(const G1Affine* __restrict__ bases,
                                                      const G1Affine* __restrict__ bases28,
                                                      const uint32_t* __restrict__ sorted,
                                                      const uint32_t* __restrict__ seg_start,
                                                      const uint32_t* __restrict__ seg_len,
                                                      const uint32_t* __restrict__ order,
                                                      const uint32_t* __restrict__ nseg_ptr,
                                                      G1XYZZ* __restrict__ partial) {
    // grid-stride over the length-sorted segments: the host may launch fewer workgroups than segments (SWM_ACC_WGS) so that
    // the kernel leaves register-file room on every SIMD for the kernels that run beside it
    const uint32_t nseg_total = *nseg_ptr;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < nseg_total; t += gridDim.x * blockDim.x) {
    uint32_t seg = order[t];
    const uint32_t k0 = seg_start[seg], e = k0 + seg_len[seg];
    if (k0 >= e) {
        p28_store(partial[seg], p28_identity());
        continue;
    }
    bool ok = true;
    Acc28 acc;
    {
        uint32_t ent = sorted[k0];
        G1Affine p = bases28[ent & 0x7fffffffu];
        acc.x = fq28_unpack(p.x);
        Fq28 y = fq28_unpack(p.y);
        if (ent >> 31) {  // -y = 4p - y, brought back to normalised limbs (value < 4p < 6p)
            Fq28 z;
#pragma unroll
            for (int i = 0; i < 14; i++) z.l[i] = Fq28Consts::SPREAD4[i] - y.l[i];
            y = fq28_normalize(z);
        }
        acc.y = y;
        acc.zz = fq28_const(Fq28Consts::ONE);
        acc.zzz = acc.zz;
    }
    for (uint32_t k = k0 + 1; k < e && ok; k++) {
        uint32_t ent = sorted[k];
        G1Affine p = bases28[ent & 0x7fffffffu];
        Fq28 x2 = fq28_unpack(p.x), y2 = fq28_unpack(p.y);
        if (ent >> 31) {
#pragma unroll
            for (int i = 0; i < 14; i++) y2.l[i] = Fq28Consts::SPREAD4[i] - y2.l[i];  // limbs < 2^29, value < 4p
        }
        ok = madd28(acc, x2, y2);
    }
    if (ok) {
        // partial sums stay in the 28-bit domain (radix 2^392, "point form" of fq28.cuh) for the bucket stage
        P28 out{acc.x, acc.y, acc.zz, acc.zzz};
        p28_store(partial[seg], out);
        continue;
    }
    // cold path: a point met +-(the running sum); redo this segment with the fully reducing adder, then move the
    // result into the 28-bit domain (coordinates x 2^8)
    G1XYZZ acc32 = g1_xyzz_identity();
    for (uint32_t k = k0; k < e; k++) {
        uint32_t ent = sorted[k];
        G1Affine p;
        if (bases) {
            p = bases[ent & 0x7fffffffu];
        } else {  // table rows exist only in the scaled form: x 2^-8 (a Montgomery product with the integer 2^376)
            p = bases28[ent & 0x7fffffffu];
            Fq d256 = fp_zero<Fq>();
            d256.v[11] = 0x01000000u;
            if (!g1_is_inf(p)) {
                p.x = fp_mul(p.x, d256);
                p.y = fp_mul(p.y, d256);
            }
        }
        if (ent >> 31) p.y = fp_neg(p.y);
        g1_add_mixed(acc32, p);
    }
    const uint32_t k256[12] = SWM_FQ_SCALE256_MONT;
    Fq c;
#pragma unroll
    for (int j = 0; j < 12; j++) c.v[j] = k256[j];
    acc32.x = fp_mul(acc32.x, c);
    acc32.y = fp_mul(acc32.y, c);
    acc32.zz = fp_mul(acc32.zz, c);   // identity (zz = 0) stays exactly zero
    acc32.zzz = fp_mul(acc32.zzz, c);
    partial[seg] = acc32;
    }
}

// The same kernel over a twisted Edwards table (msm_table_build_te): rows are the affine triples (y - x, y + x, 2 d x y), each
// coordinate as the thirteen 29-bit limbs the multiplier takes (fq29.cuh), in a 64-byte sector of its own (192 B per row, consumed
// as loaded); the accumulator is an extended point and every addition is the UNIFIED 7-product law of te29_madd_row — no doubling /
// cancellation test, no cold path: 2 359 of its instructions are multiply-adds (7 x 337; on fourteen 28-bit limbs, r04: 3 223 VALU
// instructions of which 2 646 multiply-adds, SQ pass profiles/r04_pmc_sq_msm_accumulate.json; XYZZ: 4 817), no scratch.  Rows go
// HBM -> registers, not through LDS: the kernel is issue-bound, a row is read once by one lane.  It is the
// one kernel of a proof WITHOUT an issue priority (ff.cuh SWM_LIGHT_KERNEL): the filler everything else runs beside.  Algorithmic
// bytes per point: 96 B base + 32 B scalar.  Partial sums leave as extended points in the form of the job's bucket stage
// (MsmShape::raw).  RAW: the accumulator as it stands, a TE29Pt of thirteen 128-bit words, no arithmetic — the one-lane stages add
// in the same domain.  Otherwise (a quad stage) X, Y, T, Z in the four slots of a G1XYZZ, each coordinate taken into the 28-bit
// domain by te29_to_slot: four products per segment.
template <bool RAW>
__global__ void __launch_bounds__(256, SWM_TE_EARLY_LOADS ? 3 : 4) msm_accumulate_te(const G1TE* __restrict__ rows,
                                                           const uint32_t* __restrict__ sorted,
                                                           const uint32_t* __restrict__ seg_start,
                                                           const uint32_t* __restrict__ seg_len,
                                                           const uint32_t* __restrict__ order,
                                                           const uint32_t* __restrict__ nseg_ptr,
                                                           void* __restrict__ partial_) {
    G1XYZZ* __restrict__ partial = reinterpret_cast<G1XYZZ*>(partial_);
    TE29Pt* __restrict__ partial29 = reinterpret_cast<TE29Pt*>(partial_);
    const uint32_t nseg_total = *nseg_ptr;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < nseg_total; t += gridDim.x * blockDim.x) {
        const uint32_t seg = order[t];
        // entries of the segment: sorted[k0 + j * stride], j < len (stride 1 unless the bucket's segments interleave)
        const uint32_t k0 = seg_start[seg], sl = seg_len[seg], len = sl & 0xffu, stride = max(1u, sl >> 8);
        if (len == 0) {
            if constexpr (RAW) te29_store_identity(&partial29[seg]);
            else te28_store_identity(partial[seg]);
            continue;
        }
        T29 acc;
        {
            const uint32_t ent = sorted[k0];
            const G1TE* row = rows + (ent & 0x7fffffffu);
            acc = te29_from_row(te29_load_coord(row->ymx), te29_load_coord(row->ypx), te29_load_coord(row->kt), (ent >> 31) != 0);
        }
        // the entry of the NEXT addition is read while this one computes (index clamped to the segment: no branch), so that an
        // addition waits for one memory round trip — its row — and not for two in a row
        uint32_t ent = sorted[k0 + min(1u, len - 1) * stride];
        for (uint32_t j = 1; j < len; j++) {
            const uint32_t next = sorted[k0 + min(j + 1, len - 1) * stride];
            te29_madd_row(acc, rows + (ent & 0x7fffffffu), (ent >> 31) != 0);
            ent = next;
        }
        if constexpr (RAW) {
            te29_pt_store(&partial29[seg], acc);
        } else {
            partial[seg].x = te29_to_slot(acc.x);
            partial[seg].y = te29_to_slot(acc.y);
            partial[seg].zz = te29_to_slot(acc.t);
            partial[seg].zzz = te29_to_slot(acc.z);
        }
    }
}

// The accumulation of SMALL MSMs (low-latency schedule, r04): four lanes per segment, the accumulator one coordinate per lane
// (te29_quad_madd_row): the chain of a segment of 8 entries is 16 products long instead of 50, on a chip that such a job
// cannot fill anyway.  Same partial sums, bit for bit.
template <bool RAW>
__global__ void __launch_bounds__(256) msm_accumulate_te_quad(const G1TE* __restrict__ rows, const uint32_t* __restrict__ sorted,
                                                              const uint32_t* __restrict__ seg_start,
                                                              const uint32_t* __restrict__ seg_len,
                                                              const uint32_t* __restrict__ order,
                                                              const uint32_t* __restrict__ nseg_ptr, void* __restrict__ partial_) {
    G1XYZZ* __restrict__ partial = reinterpret_cast<G1XYZZ*>(partial_);
    TE29Pt* __restrict__ partial29 = reinterpret_cast<TE29Pt*>(partial_);
    const uint32_t nseg_total = *nseg_ptr;
    const unsigned q = threadIdx.x & 3u;
    for (uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) >> 2; t < nseg_total; t += (gridDim.x * blockDim.x) >> 2) {
        const uint32_t seg = order[t];
        const uint32_t k0 = seg_start[seg], sl = seg_len[seg], len = sl & 0xffu, stride = max(1u, sl >> 8);
        if (len == 0) {
            if constexpr (RAW) te29_quad_store_identity(&partial29[seg], q);
            else te28_quad_store_identity(&partial[seg], q);
            continue;
        }
        uint32_t ent = sorted[k0];
        Fq29 own = te29_quad_from_row(rows + (ent & 0x7fffffffu), (ent >> 31) != 0, q);
        ent = sorted[k0 + min(1u, len - 1) * stride];
        for (uint32_t j = 1; j < len; j++) {
            const uint32_t next = sorted[k0 + min(j + 1, len - 1) * stride];
            te29_quad_madd_row(own, rows + (ent & 0x7fffffffu), (ent >> 31) != 0, q);
            ent = next;
        }
        if constexpr (RAW) te29_pt_store_coord(&partial29[seg], q, own);
        else reinterpret_cast<Fq*>(&partial[seg])[q] = te29_to_slot(own);  // X, Y, T (slot zz), Z (slot zzz)
    }
}

// ---------------------------------------------------------------------------------------------- bucket stage
// (XYZZ and the quad twisted Edwards form add in the 28-bit domain, fq28.cuh; the one-lane twisted Edwards stages in the 29-bit
// domain of the accumulation, fq29.cuh "the general addition": FormTE29 of msm_points.cuh, which also gives the stage's register budget and LDS slots)
// Oversized buckets (> BIG_NSEG segments: structured scalars) are folded first, one workgroup each: strided partial
// sums + LDS tree; the result replaces the bucket's first partial.
template <class Form>
__global__ void __launch_bounds__(RED_BLOCK) msm_big_bucket_sum(void* __restrict__ partial_,
                                                                const uint32_t* __restrict__ seg_off,
                                                                const uint32_t* __restrict__ hist, uint32_t SEG,
                                                                const uint32_t* __restrict__ big_count,
                                                                const uint32_t* __restrict__ big_list, unsigned log_g) {
    SWM_TAIL_KERNEL();
    using Pt = typename Form::Pt;
    Pt* __restrict__ partial = reinterpret_cast<Pt*>(partial_);  // the job's partial sums in the form's point (MsmShape::raw)
    extern __shared__ __align__(16) unsigned char smem_raw[];
    Pt* sm = reinterpret_cast<Pt*>(smem_raw);
    const uint32_t nbig = *big_count;
    // 2^log_g lanes per listed bucket (a whole workgroup for the oversized buckets of structured scalars; 4 .. 64 lanes
    // in the low-latency schedule of small MSMs, where EVERY bucket with more than two segments is folded here)
    const uint32_t G = 1u << log_g, per = RED_BLOCK >> log_g, g = threadIdx.x & (G - 1);
    for (uint32_t j0 = blockIdx.x * per; j0 < nbig; j0 += gridDim.x * per) {
        const uint32_t j = j0 + (threadIdx.x >> log_g);
        uint32_t s = 0, e = 0;
        if (j < nbig) {
            uint32_t b = big_list[j];
            s = seg_off[b];
            e = s + nseg_of(hist[b], SEG);
        }
        Form::store_identity(sm[threadIdx.x]);
#pragma unroll 1
        for (uint32_t k = s + g; k < e; k += G) Form::slot_add(&sm[threadIdx.x], &sm[threadIdx.x], &partial[k]);
        __syncthreads();
#pragma unroll 1
        for (uint32_t stride = G / 2; stride > 0; stride >>= 1) {
            if (g < stride) Form::slot_add(&sm[threadIdx.x], &sm[threadIdx.x], &sm[threadIdx.x + stride]);
            __syncthreads();
        }
        if (g == 0 && j < nbig) partial[s] = sm[threadIdx.x];
        __syncthreads();
    }
}

// Per window: sum_b (b+1) S_b with S_b = sum of the bucket's partials, fused in one kernel.
// grid = (nblk, nwin), RED_BLOCK lanes, lane t owns the m = 2^log_m buckets [lo, lo+m), lo = (blk RED_BLOCK + t) m:
//     acc_t = sum_j (j+1) S_{lo+j},  run_t = sum_j S_{lo+j}                 (running sums, 2m adds)
//     sum over the workgroup of (lo - lo_blk) run_t = m sum_{t>=1} Suffix_t,  Suffix_t = sum_{u>=t} run_u   (LDS suffix scan)
//     A_blk = sum_t acc_t + m sum_{t>=1} Suffix_t  (one LDS tree),  R_blk = Suffix_0
// The host finishes with sum_blk [A_blk + blk (RED_BLOCK m) R_blk] — a handful of additions per window.
// No scalar multiplication by the bucket offset is needed: the serial chain is ~3m + 20 group operations.
//
// Code layout matters as much as the arithmetic here.  A general addition is ~6 k instructions (48 KB); with one
// inlined copy per use (running sums, scan, tree: five sites) the kernel was 480 KB of straight-line code executed
// once per step at one wave per SIMD, i.e. every instruction came from L2 through a 64 KB instruction cache shared by
// two CUs (measured ~32 us per addition).  So every step of every phase is expressed as the same micro-operation
//     slot[dst] <- slot[dst] + *src          (dst: an LDS slot; src: an LDS slot or a partial sum in HBM)
// issued from ONE loop around ONE copy of the adder; the phases only differ in how (dst, src, active) are chosen.
// LDS: two packed slots per lane (running sum, weighted sum) + one for R = 96 KB per workgroup.
//
// Batch form: the bucket stages of up to TAIL_MAX MSMs (the commitments of one prover round) run as ONE launch,
// blockIdx.z = job.  The stage is a ~25-deep chain of ~20 us group operations whatever the number of buckets, so the
// jobs of a round share one chain latency instead of paying it one after the other.
// (RB = chains per workgroup; a chain is one lane, or Form::LANES of them: RB x LANES threads)
template <int RB, class Form>
__global__ void __launch_bounds__(RB * Form::LANES) msm_bucket_reduce(TailBatch batch) {
    SWM_TAIL_KERNEL();
    using Slot = typename Form::Slot;
    using Pt = typename Form::Pt;
    const TailJob& job = batch.j[blockIdx.z];
    if (blockIdx.x >= job.red_blocks || blockIdx.y >= job.L.nwin) return;
    const Pt* __restrict__ partial = reinterpret_cast<const Pt*>(job.partial);
    const uint32_t* __restrict__ seg_off = job.seg_off;
    const WinLayout& L = job.L;
    const unsigned log_m = job.log_m;
    G1XYZZ* __restrict__ out = job.out;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // LDS: three packed slots per lane — the running sum in two copies (the scan and the shift read a NEIGHBOUR's slot
    // while every lane rewrites its own, so those steps go from one copy to the other) and the weighted sum — plus one
    // slot for R_blk: (3 x 256 + 1) x 192 B = 144 KB per workgroup.
    Slot* sm_run = reinterpret_cast<Slot*>(smem_raw);
    Slot* sm_alt = sm_run + RB;
    Slot* sm_acc = sm_alt + RB;
    Slot* sm_r = sm_acc + RB;
    constexpr unsigned Q = Form::LANES;
    const uint32_t w = blockIdx.y, t = threadIdx.x / Q, q = threadIdx.x % Q;
    if (!((blockIdx.x >= job.blk_lo && blockIdx.x < job.blk_hi) || blockIdx.x < job.blk_low)) {
        // not a workgroup of this rank's bucket share: its buckets are empty here, the host fold sees the identity
        if (threadIdx.x < Q) Form::store_identity(sm_run[0].p, q);
        __syncthreads();
        if (threadIdx.x == 0) {
            size_t o = ((size_t)w * job.red_blocks + blockIdx.x) * 2;
            Form::store_384(out[o], sm_run[0].p);
            Form::store_384(out[o + 1], sm_run[0].p);
            if (blockIdx.x == 0 && w == 0 && job.host_flags) {
                job.host_flags[0] = job.status[0];
                job.host_flags[1] = *job.entries;
                job.host_flags[2] = job.status[1];
            }
        }
        return;
    }
    const uint32_t B = 1u << (L.c[w] - 1), m = 1u << log_m;
    const uint32_t lo = (blockIdx.x * RB + t) << log_m;
    const uint32_t base = L.boff[w];
    Form::store_identity(sm_run[t].p, q);
    Form::store_identity(sm_acc[t].p, q);
    // phase-1 sequencer of this lane: buckets b = hi-1 .. lo; per bucket "run += partial[s]" for its segments, then
    // "acc += run"
    uint32_t b = min(lo + m, B), s = 0, e = 0;
    bool walking = lo < B;
    if (walking) {
        b--;
        s = seg_off[base + b];
        e = s + nseg_of(job.hist[base + b], job.seg);
        if (e - s > job.big_nseg) e = s + 1;  // already folded into the first partial
    }
    enum { WALK = 0, SCAN = 1, SHIFT = 2, FOLD = 3, TREE = 4 };
    int phase = WALK;
    uint32_t d = 1;  // scan distance / tree stride
    __syncthreads();
#pragma unroll 1
    for (;;) {
        // one micro-operation per iteration: *dst = *pa + *pq (act), or *dst = *pa (copy: inactive lane of a scan step)
        Pt* dst = &sm_run[t].p;
        const Pt* pa = &sm_run[t].p;
        const Pt* pq = &sm_run[t].p;
        bool act = false, copy = false;
        if (phase == WALK) {
            // (r06) the walk has no meeting point but its end: a lane works on slots of its own, so every WAVE walks at its own
            // pace — its LDS traffic no longer in step with the other three waves' — and meets the workgroup once, when none of
            // its lanes has a bucket left (until r05: a workgroup-wide vote, three barriers, in front of every step)
            if (__ballot(walking) == 0) {
                __syncthreads();
                phase = SCAN;
                continue;
            }
            if (walking) {
                act = true;
                if (s < e) {
                    pq = &partial[s++];
                } else {
                    dst = &sm_acc[t].p;
                    pa = &sm_acc[t].p;
                    if (b == lo) {
                        walking = false;
                    } else {
                        b--;
                        s = seg_off[base + b];
                        e = s + nseg_of(job.hist[base + b], job.seg);
                        if (e - s > job.big_nseg) e = s + 1;
                    }
                }
            }
        } else if (phase == SCAN) {  // inclusive suffix scan of run over the workgroup (Hillis-Steele), copy to copy
            if (d >= RB) {
                phase = SHIFT;
                continue;
            }
            dst = &sm_alt[t].p;
            act = t + d < RB;
            copy = !act;
            if (act) pq = &sm_run[t + d].p;
            d <<= 1;
        } else if (phase == SHIFT) {  // run_t <- m Suffix_{t+1} (into the other copy); R_blk = Suffix_0 is parked
            if (t + 1 < RB) Form::copy(&sm_alt[t].p, &sm_run[t + 1].p, q);
            else Form::store_identity(sm_alt[t].p, q);
            if (t == 0) Form::copy(&sm_r[0].p, &sm_run[0].p, q);
#pragma unroll 1
            for (unsigned i = 0; i < log_m; i++) Form::slot_dbl(&sm_alt[t].p, &sm_alt[t].p, q);
            __syncthreads();
            Slot* x = sm_run;
            sm_run = sm_alt;
            sm_alt = x;
            phase = FOLD;
            continue;
        } else if (phase == FOLD) {  // acc_t += m Suffix_{t+1}; summed over t this is A_blk
            dst = &sm_acc[t].p;
            pa = &sm_acc[t].p;
            act = true;
            phase = TREE;
            d = RB / 2;
        } else {
            if (d == 0) break;
            if constexpr (Form::QUAD_TREE) {
                // a tree step with at most RB / 4 sums left: four lanes per sum (te29_quad_add), a third of the step's latency
                if (d <= RB / 4) {
                    const uint32_t c = threadIdx.x >> 2;
                    if (c < d) Form::quad_add(&sm_acc[c].p, &sm_acc[c].p, &sm_acc[c + d].p, threadIdx.x & 3u);
                    __syncthreads();
                    d >>= 1;
                    continue;
                }
            }
            dst = &sm_acc[t].p;
            pa = &sm_acc[t].p;
            act = t < d;
            if (act) pq = &sm_acc[t + d].p;  // the lanes t + d .. are idle in this step: nobody rewrites what is read
            d >>= 1;
        }
        if (act) Form::slot_add(dst, pa, pq, q);
        else if (copy) Form::copy(dst, pa, q);
        if (phase != WALK) __syncthreads();  // (a walk step touches the lane's own slots only)
        if (dst == &sm_alt[t].p) {  // a scan step went from one copy of the running sums to the other (uniform per step)
            Slot* x = sm_run;
            sm_run = sm_alt;
            sm_alt = x;
        }
    }
    if (threadIdx.x == 0) {
        // `out` is the job's PINNED host slot (zero-copy: 384 B per workgroup over the fabric instead of three
        // stream-ordered copies per job after the kernel — ~25 us per job between a round's last kernel and its challenge)
        size_t o = ((size_t)w * job.red_blocks + blockIdx.x) * 2;
        Form::store_384(out[o], sm_acc[0].p);
        Form::store_384(out[o + 1], sm_r[0].p);
        if (blockIdx.x == 0 && w == 0 && job.host_flags) {
            job.host_flags[0] = job.status[0];
            job.host_flags[1] = *job.entries;
            job.host_flags[2] = job.status[1];  // points with a zero scalar / identity base
        }
    }
}

// The bucket stage of twisted Edwards jobs with a THIRD of the LDS (r05).  msm_bucket_reduce keeps three slots per lane in LDS
// (running sum twice — the scan goes from one copy to the other — and the weighted sum): 144 KB per 256-lane workgroup, i.e.
// ONE workgroup per CU and one wave per SIMD, where a lone wave issues an instruction every ~5.5 cycles (SQ utilisation 0.62,
// profiles/r04_pmc_sq_msm_bucket_reduce_and_sort.json) and nothing else that wants LDS fits beside it.  Here
//   * the running sum is ONE slot per lane: the suffix scan works in place, every lane's loads ahead of a barrier and its
//     stores behind it (te29_slot_add_sync) — the unified law reads all eight input coordinates before it writes any;
//   * the weighted sum of a lane lives in HBM / L2 (job.acc: touched once per bucket, 384 B per step against ~4 400
//     instructions) and moves into the lane's LDS slot with the step that folds the suffix into it; the tree runs there;
// (256 + 1) x 208 B = 53 KB per workgroup, 164 VGPRs: two workgroups per CU by registers (three: 35 spills, slower), and a stage
// no longer owns its CU.  Same micro-operations in the same order per lane as msm_bucket_reduce<RB, FormTE29>: the same limbs, the
// same workgroup results.
// Where it is used (measured, CHANGELOG r05): in the JOINT stage of a round's deferred jobs (up to 10^6 points each), one
// workgroup per CU — 0.1 - 0.3 ms per mid-size proof; NOT for the thin stages that run beside the accumulations of large jobs
// (two workgroups per CU there: each step 2.2x slower, +0.8 ms at 2^20).  SWM_MSM_LOW = 2 (default) / 1 (everywhere) / 0 (never).
#ifndef SWM_LOW_WAVES
#define SWM_LOW_WAVES 2  // waves per SIMD the register budget allows (3: 168 VGPRs, spills 37 of them)
#endif
template <int RB>
__global__ void __launch_bounds__(RB, SWM_LOW_WAVES) msm_bucket_reduce_low(TailBatch batch) {
    SWM_TAIL_KERNEL();
    const TailJob& job = batch.j[blockIdx.z];
    if (blockIdx.x >= job.red_blocks || blockIdx.y >= job.L.nwin) return;
    using Form = FormTE29;  // (one-lane twisted Edwards jobs only: raw partial sums, 29-bit slots)
    using Slot = Form::Slot;
    using Pt = Form::Pt;
    const Pt* __restrict__ partial = reinterpret_cast<const Pt*>(job.partial);
    const uint32_t* __restrict__ seg_off = job.seg_off;
    const WinLayout& L = job.L;
    const unsigned log_m = job.log_m;
    G1XYZZ* __restrict__ out = job.out;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    Slot* sm_run = reinterpret_cast<Slot*>(smem_raw);  // RB + 1 slots of 208 B (Red29Slot: no bank conflicts)
    Slot* sm_tree = sm_run + 1;
    const uint32_t w = blockIdx.y, t = threadIdx.x;
    if (!((blockIdx.x >= job.blk_lo && blockIdx.x < job.blk_hi) || blockIdx.x < job.blk_low)) {
        if (t == 0) {
            Form::store_identity(sm_run[0].p);
            size_t o = ((size_t)w * job.red_blocks + blockIdx.x) * 2;
            Form::store_384(out[o], sm_run[0].p);
            Form::store_384(out[o + 1], sm_run[0].p);
            if (blockIdx.x == 0 && w == 0 && job.host_flags) {
                job.host_flags[0] = job.status[0];
                job.host_flags[1] = *job.entries;
                job.host_flags[2] = job.status[1];
            }
        }
        return;
    }
    Pt* __restrict__ my_acc = reinterpret_cast<Pt*>(job.acc) + ((size_t)w * job.red_blocks + blockIdx.x) * RB + t;
    const uint32_t B = 1u << (L.c[w] - 1), m = 1u << log_m;
    const uint32_t lo = (blockIdx.x * RB + t) << log_m;
    const uint32_t base = L.boff[w];
    Form::store_identity(sm_run[t].p);
    if (t == 0) Form::store_identity(sm_run[RB].p);
    Form::store_identity(*my_acc);
    uint32_t b = min(lo + m, B), s = 0, e = 0;
    bool walking = lo < B;
    if (walking) {
        b--;
        s = seg_off[base + b];
        e = s + nseg_of(job.hist[base + b], job.seg);
        if (e - s > job.big_nseg) e = s + 1;  // already folded into the first partial
    }
    enum { WALK = 0, SCAN = 1, SHIFT = 2, FOLD = 3, TREE = 4 };
    int phase = WALK;
    uint32_t d = 1;
    __syncthreads();
#pragma unroll 1
    for (;;) {
        Pt* dst = &sm_run[t].p;
        const Pt* pa = &sm_run[t].p;
        const Pt* pq = &sm_run[t].p;
        bool act = false;
        if (phase == WALK) {
            // (r06) the walk has no meeting point but its end: a lane works on slots of its own, so every WAVE walks at its own
            // pace — its LDS traffic no longer in step with the other three waves' — and meets the workgroup once, when none of
            // its lanes has a bucket left (until r05: a workgroup-wide vote, three barriers, in front of every step)
            if (__ballot(walking) == 0) {
                __syncthreads();
                phase = SCAN;
                continue;
            }
            if (walking) {
                act = true;
                if (s < e) {
                    pq = &partial[s++];
                } else {  // acc += run
                    dst = my_acc;
                    pa = my_acc;
                    if (b == lo) {
                        walking = false;
                    } else {
                        b--;
                        s = seg_off[base + b];
                        e = s + nseg_of(job.hist[base + b], job.seg);
                        if (e - s > job.big_nseg) e = s + 1;
                    }
                }
            }
        } else if (phase == SCAN) {  // inclusive suffix scan of run over the workgroup (Hillis-Steele), IN PLACE
            if (d >= RB) {
                phase = SHIFT;
                continue;
            }
            act = t + d < RB;
            if (act) pq = &sm_run[t + d].p;
            d <<= 1;
        } else if (phase == SHIFT) {  // slot_t <- m Suffix_t for t >= 1, in place; slot 0 keeps R_blk = Suffix_0 (m Suffix_0 is never needed)
#pragma unroll 1
            for (unsigned i = 0; i < log_m; i++) Form::slot_add_sync(&sm_run[t].p, &sm_run[t].p, &sm_run[t].p, t >= 1, false);
            __syncthreads();  // the fold reads the NEIGHBOUR's doubled slot
            phase = FOLD;
            continue;
        } else if (phase == FOLD) {
            // slot_{t+1} <- acc_t + m Suffix_{t+1}: lane t reads and rewrites slot t + 1 alone (slot RB holds the identity for the
            // last lane), the weighted sums move into LDS, slot 0 is left alone; summed over t this is A_blk
            dst = &sm_run[t + 1].p;
            pa = my_acc;
            pq = &sm_run[t + 1].p;
            act = true;
            phase = TREE;
            d = RB / 2;
        } else {  // tree over the slots 1 .. RB
            if (d == 0) break;
            if (d <= RB / 4) {  // narrow tree steps: four lanes per sum (te29_quad_add)
                const uint32_t c = threadIdx.x >> 2;
                if (c < d) Form::quad_add(&sm_tree[c].p, &sm_tree[c].p, &sm_tree[c + d].p, threadIdx.x & 3u);
                __syncthreads();
                d >>= 1;
                continue;
            }
            dst = &sm_tree[t].p;
            pa = &sm_tree[t].p;
            act = t < d;
            if (act) pq = &sm_tree[t + d].p;
            d >>= 1;
        }
        // barriers: the in-place scan needs its loads ahead of one and its stores behind it; a tree step and the fold are read by
        // other lanes in the NEXT step (trailing barrier); a walk step touches the lane's own slots only (the vote at the top
        // of the loop is the workgroup's only meeting point there)
        const bool walk = phase == WALK;
        Form::slot_add_sync(dst, pa, pq, act, phase == SCAN);
        if (!walk) __syncthreads();
    }
    if (threadIdx.x == 0) {
        size_t o = ((size_t)w * job.red_blocks + blockIdx.x) * 2;
        Form::store_384(out[o], sm_tree[0].p);
        Form::store_384(out[o + 1], sm_run[0].p);
        if (blockIdx.x == 0 && w == 0 && job.host_flags) {
            job.host_flags[0] = job.status[0];
            job.host_flags[1] = *job.entries;
            job.host_flags[2] = job.status[1];
        }
    }
}

// ---------------------------------------------------------------------------------------------- launches
// Stage A of the driver's msm_accumulate_stage, after the segments were ordered: one partial sum per segment, then the oversized
// buckets folded ahead of the bucket stage.
int msm_accumulate_launch(swm_ctx* ctx, const MsmShape& s, const MsmBuffers& b, const MsmTable& tab, const G1Affine* d_bases,
                          const G1Affine* d_bases28) {
    const uint32_t* nseg_live = msm_nseg_live(b);
    unsigned acc_grid = (unsigned)((s.nseg_max + 255) / 256);
    const dim3 big_grid(std::min<unsigned>((s.pl.NB + (RED_BLOCK >> s.log_g) - 1) / (RED_BLOCK >> s.log_g), s.lat ? 2048 : 512));
    if (s.te) {
        // (either kernel can feed either tail: the epilogue follows the form of the job's partial sums, not the kernel)
        if (s.quad_acc)
            SWM_LAUNCH(ctx, "msm_accumulate", s.raw ? msm_accumulate_te_quad<true> : msm_accumulate_te_quad<false>,
                       dim3((unsigned)((s.nseg_max + 63) / 64)), dim3(256), 0, tab.te, b.sorted, b.seg_start, b.seg_len, b.order, nseg_live,
                       b.partial);
        else
            SWM_LAUNCH(ctx, "msm_accumulate", s.raw ? msm_accumulate_te<true> : msm_accumulate_te<false>, dim3(acc_grid), dim3(256), 0,
                       tab.te, b.sorted, b.seg_start, b.seg_len, b.order, nseg_live, b.partial);
    } else {
        SWM_LAUNCH(ctx, "msm_accumulate", msm_accumulate, dim3(acc_grid), dim3(256), 0,
                   s.flat ? (const G1Affine*)nullptr : d_bases, s.flat ? tab.t28 : d_bases28, b.sorted, b.seg_start, b.seg_len, b.order,
                   nseg_live, (G1XYZZ*)b.partial);
    }
    SWM_LAUNCH(ctx, "msm_big_bucket_sum",
               s.raw ? msm_big_bucket_sum<FormTE29> : (s.te ? msm_big_bucket_sum<FormTEFold28> : msm_big_bucket_sum<FormXYZZ>), big_grid,
               dim3(RED_BLOCK), RED_BLOCK * (s.raw ? sizeof(TE29Pt) : sizeof(G1XYZZ)), b.partial, b.seg_off, b.hist, s.SEG, b.big_count,
               b.big_list, s.log_g);
    return SWM_OK;
}
// The bucket stage of the k jobs the driver's msm_launch_tails put into `batch`, by the kernel it chose for them.
int msm_tail_launch(swm_ctx* ctx, const TailBatch& batch, int k, MsmTailKernel kernel, unsigned rb, unsigned max_red, unsigned max_win) {
    if (kernel == TAIL_QUAD) {
        const size_t lds = (3 * (size_t)rb + 1) * sizeof(PlainSlot);
        const dim3 grid(max_red, max_win, (unsigned)k);
        if (rb == 256) {
            SWM_TRY(allow_big_lds(ctx, LDS_REDUCE_QUAD_256, (const void*)msm_bucket_reduce<256, FormTEQuad>, lds));
            SWM_LAUNCH(ctx, "msm_bucket_reduce", (msm_bucket_reduce<256, FormTEQuad>), grid, dim3(1024), lds, batch);
        } else {
            SWM_TRY(allow_big_lds(ctx, LDS_REDUCE_QUAD_128, (const void*)msm_bucket_reduce<128, FormTEQuad>, lds));
            SWM_LAUNCH(ctx, "msm_bucket_reduce", (msm_bucket_reduce<128, FormTEQuad>), grid, dim3(512), lds, batch);
        }
    } else if (kernel == TAIL_LOW) {
        SWM_LAUNCH(ctx, "msm_bucket_reduce", (msm_bucket_reduce_low<256>), dim3(max_red, max_win, (unsigned)k), dim3(RED_BLOCK),
                   (RED_BLOCK + 1) * sizeof(Red29Slot), batch);
    } else if (kernel == TAIL_TE29) {
        SWM_TRY(allow_big_lds(ctx, LDS_REDUCE_TE29,(const void*)msm_bucket_reduce<256, FormTE29>, (3 * RED_BLOCK + 1) * sizeof(Red29Slot)));
        SWM_LAUNCH(ctx, "msm_bucket_reduce", (msm_bucket_reduce<256, FormTE29>), dim3(max_red, max_win, (unsigned)k), dim3(RED_BLOCK),
                   (3 * RED_BLOCK + 1) * sizeof(Red29Slot), batch);
    } else {
        SWM_TRY(allow_big_lds(ctx, LDS_REDUCE_XYZZ,(const void*)msm_bucket_reduce<256, FormXYZZ>, (3 * RED_BLOCK + 1) * sizeof(RedSlot)));
        SWM_LAUNCH(ctx, "msm_bucket_reduce", (msm_bucket_reduce<256, FormXYZZ>), dim3(max_red, max_win, (unsigned)k), dim3(RED_BLOCK),
                   (3 * RED_BLOCK + 1) * sizeof(RedSlot), batch);
    }
    return SWM_OK;
}

}  // namespace swm

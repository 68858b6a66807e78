// msm.hip — K1: G1 multi-scalar multiplication on BLS12-377 for gfx950 (MI355X).
//
// Replaces ark_ec::msm::VariableBaseMSM::multi_scalar_mul (ark-ec 0.3.0), reached from
// /root/reference/src/marlin/mod.rs:75,92 through KZG10::commit/open.  arkworks runs an unsigned-window Pippenger
// with one rayon task per window; the MI355X design is different on purpose (the sum is a canonical group element,
// so only the result has to agree).  Two schedules: per-window buckets (msm_plan) for table-less base sets, and the
// precomputed-window ("flat") schedule, where a resident set's window multiples (msm_table_build[_te]) let all windows
// share ONE bucket set.  The stages of one MSM (msm_enqueue; msm_shape decides their geometry), with the unit that holds each:
//   1. msm_digits        signed-digit recoding, window-major (digits in [-2^(c-1), 2^(c-1)] halve the bucket count)
//                        [msm_sort.hip]
//   2. sort by bucket    per-window: msm_hist, msm_scan_totals / _mid / _final, msm_scatter (large MSMs also msm_bin_check,
//                        msm_partition, msm_bin_sort); flat: msm_flat_coarse_hist, msm_flat_scan_bins, msm_flat_partition,
//                        msm_flat_bin_sort, which also writes the segment descriptors.  The second job of a twin pair copies
//                        the first one's sort instead (msm_twin_copy).  [msm_sort.hip]
//   3. msm_seg_desc / msm_seg_order   buckets cut into segments of at most SEG entries, ordered by length  [msm_sort.hip]
//   4. msm_accumulate[_te, _te_quad]  one lane (or four) per segment: gathered bases or table rows, mixed additions
//                        (XYZZ or twisted Edwards, no MFMA) -> one partial sum per segment.  The dominant kernel.
//                        [msm_stages.hip, point routines in msm_points.cuh]
//   5. msm_big_bucket_sum  buckets with many segments folded by a lane group ahead of the bucket stage  [msm_stages.hip]
//   6. msm_bucket_reduce[_low]  the bucket stage: sum_b (b+1) S_b per window into (A, R) pairs per workgroup, written to a
//                        pinned host slot; deferred jobs of a prover round share one launch (msm_flush_tails)  [msm_stages.hip]
//   7. host              per-workgroup pairs and the Horner fold over the windows (msm_finish)  [this file]
// This file is the driver: shape, streams, scratch, result slots, the order of the stages, the tails and the host fold.  The
// base sets and their tables are msm_table.hip's, the point-layer self-test msm_selftest.hip's; msm_stages.h is what the units
// share.
//
// Algorithmic bytes per point: 96 B base + 32 B scalar = 128 B.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "context.h"
#include "fill.cuh"
#include "fq29.cuh"
#include "g1.cuh"
#include "msm_stages.h"
#include <atomic>
#include <chrono>

namespace swm {

// ---------------------------------------------------------------------------------------------- host driver
// Kernels that want more than 64 KB of dynamic LDS need the attribute raised once per device; `slot` names the kernel
// (MsmLdsSlot, msm_stages.h) in a small process-wide cache so that the runtime call is not repeated per MSM.
int allow_big_lds(swm_ctx* ctx, MsmLdsSlot slot, const void* fn, size_t bytes) {
    static std::atomic<size_t> granted[64][LDS_SLOTS];
    if (bytes <= 64 * 1024) return SWM_OK;
    const int dev = ctx->device & 63;
    if (granted[dev][slot].load(std::memory_order_acquire) >= bytes) return SWM_OK;
    SWM_HIP(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    size_t cur = granted[dev][slot].load(std::memory_order_relaxed);
    while (cur < bytes && !granted[dev][slot].compare_exchange_weak(cur, bytes)) {}
    return SWM_OK;
}

// ---------------------------------------------------------------------------------------------- hardware-queue probe
// Do two streams execute concurrently, i.e. sit on different hardware queues?  One single-lane kernel per stream that
// spins ~60 us on the constant-rate clock and records when it started and ended: on one queue the second starts after
// the first has ended.  ~0.15 ms per probe, used once per context while the stage streams are set up.
__global__ void msm_probe_spin(unsigned long long* out, long long ticks) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) {}
    out[0] = (unsigned long long)t0;
    out[1] = (unsigned long long)wall_clock64();
}
static int streams_concurrent(swm_ctx* ctx, hipStream_t x, hipStream_t y, bool* concurrent) {
    unsigned long long* d = nullptr;
    SWM_TRY(scratch(ctx, "msm.probe", 64, (void**)&d));
    hipLaunchKernelGGL(msm_probe_spin, dim3(1), dim3(1), 0, x, d, (long long)6000);  // 100 MHz clock: 60 us
    hipLaunchKernelGGL(msm_probe_spin, dim3(1), dim3(1), 0, y, d + 2, (long long)6000);
    SWM_HIP(ctx, hipGetLastError());
    SWM_HIP(ctx, hipStreamSynchronize(x));
    SWM_HIP(ctx, hipStreamSynchronize(y));
    unsigned long long h[4];
    SWM_HIP(ctx, hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
    *concurrent = h[2] < h[1];  // y started before x ended
    return SWM_OK;
}


// ---- asynchronous form -------------------------------------------------------------------------------------
// msm_enqueue launches every kernel of one MSM plus the download of its window sums WITHOUT host synchronisation (shape,
// result slot, streams, scratch, the stages, the tail hand-off); msm_finish waits for that download and does the host fold.
// `lane` selects the streams and the device scratch set: lane < 0, the context's own stream (the K1 ABI entry points);
// lane >= 0, the auxiliary streams, after everything enqueued on the context's stream so far.  The prover alternates lanes, so
// that the tail of one MSM and the sort of the next overlap with the VALU-bound accumulation.  Results land in pinned host slots.
// Stream of one of the roles main / sort / accumulation / tail: non-blocking, default priority (stream priorities per role were
// measured in r04 / r05 — every assignment slower, CHANGELOG.md — and are gone; what orders the kernels on the chip is s_setprio).
hipError_t msm_create_stream(hipStream_t* out) { return hipStreamCreateWithFlags(out, hipStreamNonBlocking); }
bool msm_flat_applies(const MsmTable& tab, size_t n) {
    static const bool no_table = sw(SW_MSM_NO_TABLE) != 0;  // the per-window schedule for every set (what table-less sets run)
    return tab.any() && !no_table && n >= ((size_t)1 << (tab.c > 8 ? tab.c - 8 : 0)) &&
           (uint64_t)tab.stride * msm_table_windows(tab.c) < (1ull << 31);
}
// Makes `st` the context's stream for a scope, so that launches, memsets, scratch growth and the profiling events all refer to it.
struct StreamSwap {
    swm_ctx* c;
    hipStream_t old;
    StreamSwap(swm_ctx* ctx, hipStream_t st) : c(ctx), old(ctx->stream) { ctx->stream = st; }
    ~StreamSwap() { c->stream = old; }
};
// Bucket stage of maxB buckets on workgroups of rb chains: *log_m (log2 buckets per lane) raised until the stage fits in max_blocks
// workgroups per window; returns the workgroups per window.
static unsigned bucket_blocks(uint32_t maxB, unsigned rb, unsigned max_blocks, unsigned* log_m) {
    while (((maxB >> *log_m) + rb - 1) / rb > max_blocks) (*log_m)++;
    return std::max(1u, ((maxB >> *log_m) + rb - 1) / rb);
}
// A job's pinned result slot: up to 1024 (A, R) pairs, the last 16 bytes carry the status words of the job.
static constexpr size_t SLOT_BYTES = (size_t)MAX_WIN * 32 * sizeof(G1XYZZ) + 64;
static constexpr size_t SLOT_FLAGS_OFF = SLOT_BYTES - 16;

// Fills *out for an MSM of n points on `tab`.  Launches and allocates nothing: reads ctx->msm_pipe_min and the switches only.
static int msm_shape(swm_ctx* ctx, size_t n, const MsmTable& tab, int lane, bool defer_tail, MsmShape* out) {
    MsmShape& s = *out = MsmShape();
    // flat schedule: the base set comes with its precomputed window multiples and the MSM is large enough to populate the
    // shared bucket set (below ~2^(c-4) points the per-window schedule with its small windows wins)
    s.flat = msm_flat_applies(tab, n);
    s.te = s.flat && tab.te != nullptr;
    if (!tab.contiguous() && !s.flat)
        return set_err(ctx, SWM_ERR_INTERNAL, "msm: a strided base layout needs the precomputed-window schedule");
    if (tab.scalar_stride != 1 && !s.flat) return set_err(ctx, SWM_ERR_INTERNAL, "msm: strided scalars need the table schedule");
    if (tab.shard_world > 1 && (!s.flat || !tab.contiguous()))
        return set_err(ctx, SWM_ERR_INTERNAL, "msm: a bucket-range split needs the table schedule");
    // low-latency schedule (flat MSMs below ~2^18 points, where a proof is a chain of dependent additions rather than
    // a throughput problem): short segments (8 points), every bucket with more than two segments folded by a lane
    // group in msm_big_bucket_sum (a tree instead of the serial walk of the bucket stage), one bucket per lane in the
    // bucket stage
    static constexpr size_t lat_below = 262144;
    s.lat = s.flat && n < lat_below;
    const WinLayout& pl = s.pl = s.flat ? msm_table_layout(tab.c) : msm_plan(n);
    // rl: the layout the bucket stage and the host fold see — one window of 2^(c-1) buckets in the flat schedule
    s.rl = pl;
    if (s.flat) {
        s.rl.nwin = 1;
        s.rl.boff[1] = s.rl.NB;
    }
    s.total = n * (size_t)pl.nwin;
    if (s.total >= (1ull << 32)) return set_err(ctx, SWM_ERR_INVALID_ARG, "msm: n * windows must be < 2^32");
    // buckets per lane in the reduction: at most 16 workgroups per window (the host folds one (A, R) pair per workgroup)
    // small windows: one bucket per lane shortens the serial walk of a lone MSM (r01 sweep); inside a round's batch the
    // workgroups of all jobs have to be resident together (one per CU: 96 KB of LDS each), which four buckets per lane allow
    unsigned log_m = pl.maxB <= 2048 ? (defer_tail ? 2 : 0) : 2;
    if (s.lat) log_m = 0;
    // (A, R) pairs per window that fit a result slot and that the host folds: 16 per window, or 256 for the single
    // window of the flat schedule (one workgroup per CU either way)
    // workgroup width of the bucket stage: 256 lanes (single-wave workgroups of 64 lanes were measured in r02: the stage 1.00
    // instead of 0.72 ms, a 2^20 proof 82.7 instead of 77.4 ms).
    // Low-latency schedule on twisted Edwards rows: every chain of the bucket stage is worked by a quad of lanes (FormTEQuad;
    // SWM_MSM_QUAD=0: one lane per chain as for large jobs): 128 chains per workgroup (512 threads), at most 64 workgroups per
    // job, bucket sets up to 2^15 (r04 sweeps, CHANGELOG.md).
    static const bool quad_on = sw(SW_MSM_QUAD) != 0;
    static constexpr unsigned quad_rb = 128u, quad_blocks = 64u, quad_maxb = 32768u;
    s.quad = s.lat && s.te && quad_on && pl.maxB <= quad_maxb;
    s.rb = s.quad ? quad_rb : 256u;
    // One-lane twisted Edwards stages may take the low-LDS kernel (msm_bucket_reduce_low: 49 KB per workgroup);
    // SWM_MSM_LOW=0: always the 144-KB kernel of r02 - r04.  SWM_MSM_LOW_BLOCKS: workgroups a stage may be cut into (result slot:
    // up to 1024 (A, R) pairs; the host folds them in groups of 16).
    // r05, last collection: in the JOINT stage of deferred jobs (shaped by msm_joint_shape) it is worth 0.1 - 0.3 ms per mid-size
    // proof (2^16 7.2 -> 7.07, 2^18 17.2 -> 16.9, Merkle circuit 15.0 -> 14.7 ms); for the thin stages of large jobs it costs
    // 0.8 ms at 2^20 (two workgroups per CU).  SWM_MSM_LOW: 2 (default) = joint stages only, 1 = every one-lane stage, 0 = never.
    static const long low_mode = sw(SW_MSM_LOW);
    const bool low_on = low_mode == 1 || (low_mode == 2 && defer_tail);
    static constexpr unsigned low_blocks = 256u;
    // (joint stages of small jobs: SWM_MSM_JOINT_BLOCKS workgroups per job — with the low-LDS kernel twelve waves per CU are resident)
    // 64 per job: the four stages of a round's launch are resident together, one workgroup per CU — in the low-latency schedule
    // (r02) and for the larger jobs that join a round's launch since r05 (up to 10^6 points: 2^19 buckets -> 32 per lane).  With the
    // low-LDS kernel 128 per job (two workgroups per CU) measured SLOWER per launch: 1.43 against 1.06 ms for four 2^19-bucket jobs.
    static constexpr unsigned joint_blocks = 64u;
    s.low = s.te && !s.quad && s.rb == 256 && low_on;
    // Form of the job's partial sums: raw points of the 29-bit domain (TE29Pt, 208 B) when its bucket stage is a one-lane twisted
    // Edwards one (msm_bucket_reduce<256, FormTE29> or msm_bucket_reduce_low, whichever a later re-shaping picks); the 28-bit slots
    // of the accumulation's epilogue for a quad stage (FormTEQuad), and XYZZ points otherwise.
    s.raw = s.te && !s.quad;
    // (low-latency schedule: the bucket stages of a round's four MSMs run in one launch and have to be resident together)
    const unsigned max_blocks = s.quad ? quad_blocks : (s.flat ? (defer_tail ? joint_blocks : (s.low ? low_blocks : 256u)) : 16u);
    s.max_blocks = s.low ? std::max(max_blocks, low_blocks) : std::max(max_blocks, 256u);
    s.red_blocks = bucket_blocks(pl.maxB, s.rb, max_blocks, &log_m);
    s.log_m = log_m;
    s.wpart_n = (size_t)s.rl.nwin * std::max(s.red_blocks, s.flat ? s.max_blocks : 0u) * 2;
    if (s.wpart_n * sizeof(G1XYZZ) > SLOT_FLAGS_OFF) return set_err(ctx, SWM_ERR_INTERNAL, "msm: result slot too small");
    // Small MSMs keep a single stream: the extra event hops cost more than they hide.
    // r05: a proof whose commitments fall on both sides of the bound ran them on streams that alias (a small job's lane stream is
    // a large job's accumulation or bucket-stage stream): at 2^16 constraints — 65 535-point and 196 608-point commitments — the
    // opening's second sort waited for the first accumulation.  The prover therefore sets ctx->msm_pipe_min per proof (every
    // commitment of a proof up to 2^19 constraints on one stream of its lane, four lanes: 2^16 7.05 -> 6.5 ms, 2^19 29.4 -> 28.6 ms;
    // from 2^20 on the three-stage pipeline is ahead).
    const size_t pipe_min = ctx->msm_pipe_min ? ctx->msm_pipe_min : (size_t)131072;
    s.one_stream = n < pipe_min;
    // small MSMs: four single-stream lanes (scratch sets 0 .. 3 on the streams 1, 2, 3, 0), so that the launch chains of
    // all four commitments of a prover round proceed side by side; sets 0 and 1 are shared with the pipelined form,
    // whose accumulations run on the same streams 1 and 2 (stream order covers the reuse)
    static constexpr int small_lanes = 4;
    // scratch sets of the pipelined form: two — the sort of job k + 2 waits for the accumulation of job k (four sets, the
    // sorts running further ahead, measured nothing in r04; memory: ~110 B per digit and set)
    static constexpr int sets = 2;
    s.lane = lane < 0 ? lane : lane % (s.one_stream ? small_lanes : sets);
    s.blk_hi = s.red_blocks;  // (blk_lo = blk_low = 0: no bucket-range split)
    if (tab.shard_world > 1) {
        const unsigned G = tab.shard_world, g = tab.shard_rank;
        const uint64_t span = (uint64_t)s.rb << s.log_m;  // buckets per bucket-stage workgroup
        s.blk_lo = (unsigned)((uint64_t)s.red_blocks * g / G);
        s.blk_hi = (unsigned)((uint64_t)s.red_blocks * (g + 1) / G);
        unsigned cfull = 0, cnarrow = 0;
        for (unsigned w = 0; w < pl.nwin; w++) cfull = std::max<unsigned>(cfull, pl.c[w]);
        for (unsigned w = 0; w < pl.nwin; w++)
            if (pl.c[w] < cfull) cnarrow = std::max<unsigned>(cnarrow, pl.c[w]);
        if (cnarrow) s.blk_low = (unsigned)((((uint64_t)1 << (cnarrow - 1)) + span - 1) / span);  // digits of a narrow window: buckets < 2^(c - 1)
        s.dshard.on = 1;
        s.dshard.cfull = cfull;
        s.dshard.blo = (uint32_t)std::min<uint64_t>(s.blk_lo * span, pl.NB);
        s.dshard.bhi = (uint32_t)std::min<uint64_t>(s.blk_hi * span, pl.NB);
        s.dshard.plo = (uint64_t)(((unsigned __int128)n * g) / G);
        s.dshard.phi = (uint64_t)(((unsigned __int128)n * (g + 1)) / G);
    }

    // Segment bound.  Long segments mean one partial sum per bucket (the bucket stage walks fewer partials) but fewer,
    // longer lanes in the accumulation; they pay once the buckets alone oversubscribe the chip (r01 sweep: 128 beats
    // 32 by 10 % at 2^20 and 2^22, loses at 2^16 where 45 k buckets cannot fill 196 k lane slots).
    s.SEG = pl.NB >= 262144 ? SEG_MAX : 32;  // smaller bounds for small MSMs measured within run-to-run noise
    if (s.lat) s.SEG = 16;  // (8 below 2^16 points until r04: with four lanes per segment the chain per entry is 2 products, not 7)
    // (r05, prefix tables: a job of |H| points on a table one bit narrower than before has ~14 entries per bucket — with 16-point
    // segments a quarter of the buckets would split in two and the bucket stage walk 2.3 instead of 2 steps per bucket)
    if (s.lat && s.total / pl.NB >= 10) s.SEG = 32;
    // segments per bucket above which a bucket is folded ahead of the bucket stage, and the lanes that fold one
    s.big_nseg = BIG_NSEG;
    s.log_g = 8;
    if (s.lat) {
        // every bucket with more than two segments below 2^16 points; from there (16-point segments, 1 - 2 per bucket) only
        // the rare long ones: listing ~2 % of the buckets cost a ~120-us launch per MSM for a two-step shorter walk
        // (r02: 2^16 proofs 11.5 -> 10.8 ms)
        s.big_nseg = n < 65536 ? 4 : 6;  // (2 with 8-point segments, until r04)
        const size_t per_bucket = s.total / ((size_t)pl.NB * s.SEG) + 1;  // expected segments per bucket
        s.log_g = 2;
        while (s.log_g < 6 && ((size_t)1 << s.log_g) < 2 * per_bucket) s.log_g++;
    }
    // small jobs (up to 2^20 digits: r04 sweep): four lanes per segment
    static constexpr size_t quad_acc = 1048576;
    s.quad_acc = s.te && s.lat && s.total <= quad_acc && quad_on;
    // every bucket adds at most one short segment; the flat schedule hands out segment indices per coarse bin with the bin's
    // capacity (msm_flat_scan_bins): at most one more per bucket slot of the (padded) bins
    s.nseg_max = s.total / s.SEG + pl.NB + 1 + (s.flat ? FLAT_MAX_FINE + FLAT_MAX_BINS : 0);
    s.scan_tiles = (pl.NB + SCAN_TILE - 1) / SCAN_TILE;
    // two-level scatter for large MSMs (see msm_partition): bins of ~8 k entries, sized per window
    s.two_level = !s.flat && n >= 262144 && pl.maxB >= 8192;
    if (s.two_level) {
        uint32_t target = 64;  // bins per full window: next power of two >= n / 8192, within [64, PART_MAX_BINS]
        while (target < PART_MAX_BINS && (size_t)target * 8192 < n) target <<= 1;
        for (unsigned w = 0; w < pl.nwin; w++) {
            uint32_t B = 1u << (pl.c[w] - 1), beff = B;
            if (w + 1 == pl.nwin) {  // top window: digits only reach (r - 1) >> bit (+ 1 for the carry), never negative
                uint64_t top = 0;
                for (int i = 7; i >= 0; i--) {
                    int sh = 32 * i - (int)pl.bit[w];
                    if (sh >= 0 && sh < 64) top |= (uint64_t)FrParams::P[i] << sh;
                    else if (sh < 0 && sh > -32) top |= (uint64_t)FrParams::P[i] >> (-sh);
                }
                beff = (uint32_t)std::min<uint64_t>(B, top + 2);
            }
            unsigned lb = 0;
            while ((1u << lb) < beff) lb++;
            unsigned lt = 0;
            while ((1u << lt) < target) lt++;
            // a window with 2^lb possible buckets out of the nominal 2^(c-1) holds 2^(c-1-lb) times denser buckets:
            // give it proportionally more bins so that a bin still holds ~n / target entries
            unsigned fb = lb > lt ? lb - lt : 0;
            if (fb > 7) fb = 7;
            uint32_t nb = (beff + (1u << fb) - 1) >> fb;
            if (nb > PART_MAX_BINS) {
                s.two_level = false;
                break;
            }
            s.bp.fb[w] = (uint8_t)fb;
            s.bp.nbins[w] = (uint16_t)nb;
            s.bp.max_nbins = std::max(s.bp.max_nbins, nb);
        }
    }
    if (s.flat) {
        // flat schedule: coarse bins of the shared bucket set (<= 4096 bins, <= 512 buckets each, ~8 k entries per bin)
        // as few bins as the LDS of msm_flat_bin_sort allows (FLAT_BIN_CAP entries): every (tile, bin) run of the partition
        // costs one global atomic, and with ~2 entries per run those atomics (27 M at 2^22 points) were the whole kernel
        static constexpr size_t bin_target = 28000;  // (14 000: 52.3 - 52.5 vs 51.4 ms at 2^20, r04)
        // (small MSMs: at least ~1024 bins as long as a bin keeps 1024 entries — 64 bins meant 64 workgroups in the bin
        // sort and 1024 lanes contending for 64 LDS counters in the coarse histogram)
        const size_t target = std::min(bin_target, std::max<size_t>(1024, s.total / 1024));
        uint32_t want = 64;
        while (want < FLAT_MAX_BINS && (size_t)want * target < s.total) want <<= 1;
        while ((pl.NB >> s.flat_fb) > want) s.flat_fb++;
        while ((1u << s.flat_fb) > FLAT_MAX_FINE) s.flat_fb--;  // keeps the fine-count arrays of msm_flat_bin_sort within LDS
        s.flat_bins = (pl.NB + (1u << s.flat_fb) - 1) >> s.flat_fb;
        if (s.flat_bins > FLAT_MAX_BINS) return set_err(ctx, SWM_ERR_INTERNAL, "msm: too many coarse bins");
        if (pl.nwin > FLAT_CUR_STRIDE) return set_err(ctx, SWM_ERR_INTERNAL, "msm: too many windows for the flat sort");
    }
    return SWM_OK;
}

// SWM_TRACE: one line per MSM with the decisions above — which schedule, which sort, which geometry (tests/test_gpu_msm_schedules.py
// holds every case to the schedule it names).  c / c_top: widths of the widest and of the top window; fb0 / nbins0 and fb_top /
// nbins_top: the bin plan of the first and of the top window of a two-level sort (0 otherwise).
static void msm_trace_shape(size_t n, const MsmShape& s) {
    const unsigned top = s.pl.nwin - 1;
    fprintf(stderr,
            "[swm] msm shape: n=%zu flat=%d te=%d lat=%d two_level=%d c=%u c_top=%u nwin=%u SEG=%u big_nseg=%u flat_fb=%u flat_bins=%u "
            "fb0=%u nbins0=%u fb_top=%u nbins_top=%u\n",
            n, (int)s.flat, (int)s.te, (int)s.lat, (int)s.two_level, (unsigned)s.pl.c[0], (unsigned)s.pl.c[top], s.pl.nwin, s.SEG,
            s.big_nseg, s.flat_fb, s.flat_bins, s.two_level ? (unsigned)s.bp.fb[0] : 0u, s.two_level ? (unsigned)s.bp.nbins[0] : 0u,
            s.two_level ? (unsigned)s.bp.fb[top] : 0u, s.two_level ? (unsigned)s.bp.nbins[top] : 0u);
}

// ---- scratch of a job
static MsmZeroLayout msm_zero_layout(const MsmShape& s) {
    MsmZeroLayout z = MsmZeroLayout();
    const size_t lens = (size_t)(SEG_MAX + 1) * LEN_STRIDE, bins = (size_t)FLAT_CUR_STRIDE * FLAT_MAX_BINS;
    z.hist = 0;
    z.cursor = z.hist + s.pl.NB + 1;
    z.big_count = z.cursor + s.pl.NB + 1;
    z.len_hist = z.big_count + 4;
    z.len_cursor = z.len_hist + lens;
    z.two_level_bad = z.len_cursor + lens;
    z.bin_cursor = z.two_level_bad + MAX_WIN;
    size_t end = z.bin_cursor + (size_t)s.pl.nwin * (s.two_level ? PART_MAX_BINS : 0);
    if (s.flat) {
        z.flat_cnt = (end + 31) & ~(size_t)31;
        z.flat_win_off = z.flat_cnt + bins;
        z.flat_cur = z.flat_win_off + bins;
        z.flat_off = z.flat_cur + bins;
        z.flat_seg_off = z.flat_off + FLAT_MAX_BINS + 2;
        end = z.flat_seg_off + FLAT_MAX_BINS + 2;
    }
    z.words = (end + 63) & ~(size_t)63;
    return z;
}
// The named device buffers of a job.  What the deferred bucket stage of a job still reads (the zeroed block with the status words,
// bucket / segment offsets, big-bucket list, partial sums, the low-LDS stage's sums) is kept per result SLOT ("msmS<slot>.<name>",
// `kind`: its entry in ctx->msm_slot_bytes); the rest is per lane ("msm<lane>.<name>", lane 9 for lane < 0: stream-ordered reuse).
enum MsmBuf { BUF_HIST, BUF_SEGS, BUF_BUCKET_OFF, BUF_SEG_OFF, BUF_DIGITS, BUF_SORTED, BUF_SCAN_TOT, BUF_BIG_LIST, BUF_POINTS, BUF_PAIRS, BUF_ACC };
static const struct {
    const char* name;
    int kind;  // -1: per lane
} msm_bufs[] = {{"hist", 0},    {"segs", -1},     {"bucket_off", 1}, {"seg_off", 2}, {"digits", -1}, {"sorted", -1},
                {"scan_tot", -1}, {"big_list", 3}, {"points", 4},     {"pairs", -1},  {"acc", 5}};
static int msm_buffer(swm_ctx* ctx, MsmBuf id, int slot, int lane, size_t bytes, void** out) {
    const int kind = msm_bufs[id].kind;
    char nm[32];
    snprintf(nm, sizeof(nm), kind >= 0 ? "msmS%d.%s" : "msm%d.%s", kind >= 0 ? slot : (lane < 0 ? 9 : lane), msm_bufs[id].name);
    // Per-slot buffers are sized by the LARGEST request any slot has seen, not by the job at hand (r05): the eight result slots
    // rotate through the jobs of successive proofs (15 jobs per Merkle-circuit proof: a slot meets a different commitment every
    // proof), and a slot that had only held 131 072-point jobs grew — all streams synchronised, hipFree, hipMalloc: 2.4 ms with
    // the GPU idle — when a 786 432-point job reached it, somewhere in each of the first dozen proofs of a key.
    if (kind >= 0) bytes = ctx->msm_slot_bytes[kind] = std::max(ctx->msm_slot_bytes[kind], bytes);
    return scratch(ctx, nm, bytes, out);
}
// follow: the segment descriptors are the twin pair's own ("msmT.segs"), not the lane's
static int msm_buffers(swm_ctx* ctx, const MsmShape& s, const MsmZeroLayout& z, int slot, bool follow, MsmBuffers* out) {
    MsmBuffers& b = *out = MsmBuffers();
    SWM_TRY(msm_buffer(ctx, BUF_HIST, slot, s.lane, z.words * 4, (void**)&b.hist));
    b.cursor = b.hist + z.cursor;
    b.big_count = b.hist + z.big_count;
    b.len_hist = b.hist + z.len_hist;
    b.len_cursor = b.hist + z.len_cursor;
    b.two_level_bad = b.hist + z.two_level_bad;
    b.bin_cursor = b.hist + z.bin_cursor;
    b.flat_cnt = b.hist + z.flat_cnt;
    b.flat_win_off = b.hist + z.flat_win_off;
    b.flat_cur = b.hist + z.flat_cur;
    b.flat_off = b.hist + z.flat_off;
    b.flat_seg_off = b.hist + z.flat_seg_off;
    if (s.two_level || s.flat) SWM_TRY(msm_buffer(ctx, BUF_PAIRS, slot, s.lane, s.total * sizeof(uint2), (void**)&b.pairs));
    if (follow) SWM_TRY(scratch(ctx, "msmT.segs", s.nseg_max * 12, (void**)&b.seg_start));
    else SWM_TRY(msm_buffer(ctx, BUF_SEGS, slot, s.lane, s.nseg_max * 12, (void**)&b.seg_start));
    b.seg_len = b.seg_start + s.nseg_max;
    b.order = b.seg_len + s.nseg_max;
    SWM_TRY(msm_buffer(ctx, BUF_BUCKET_OFF, slot, s.lane, (s.pl.NB + 1) * 4ull, (void**)&b.bucket_off));
    SWM_TRY(msm_buffer(ctx, BUF_SEG_OFF, slot, s.lane, (s.pl.NB + 1) * 4ull, (void**)&b.seg_off));
    SWM_TRY(msm_buffer(ctx, BUF_DIGITS, slot, s.lane, s.total * 4, (void**)&b.digits));
    SWM_TRY(msm_buffer(ctx, BUF_SORTED, slot, s.lane, s.total * 4, (void**)&b.sorted));
    SWM_TRY(msm_buffer(ctx, BUF_SCAN_TOT, slot, s.lane, (size_t)(s.scan_tiles + 1) * 8, (void**)&b.tot_cnt));
    b.tot_seg = b.tot_cnt + s.scan_tiles + 1;
    SWM_TRY(msm_buffer(ctx, BUF_BIG_LIST, slot, s.lane, (size_t)s.pl.NB * 4, (void**)&b.big_list));
    const size_t pt = s.raw ? sizeof(TE29Pt) : sizeof(G1XYZZ);  // stride of the job's points at rest (208 B raw, 192 B slots)
    SWM_TRY(msm_buffer(ctx, BUF_POINTS, slot, s.lane, (s.nseg_max + s.wpart_n) * pt, &b.partial));
    if (s.low) SWM_TRY(msm_buffer(ctx, BUF_ACC, slot, s.lane, (size_t)s.rl.nwin * s.max_blocks * 256 * pt, &b.acc));
    return SWM_OK;
}

// ---- twin roles (msm.h).  *lead: this job writes the sorted array of twin.tab2 beside its own.  Returns the lead whose sort this
// job takes over, or null.  Any mismatch of the shapes leaves both on the ordinary schedule.  SWM_MSM_TWIN=0: never.
static MsmJob* msm_twin_match(const MsmJob* job, const MsmShape& s, const MsmSortGeom& geom, const void* d_scalars, size_t n, int mont,
                              const MsmInfMask& inf, const MsmTable& tab, const MsmTwin& twin, bool* lead) {
    static const bool twin_on = sw(SW_MSM_TWIN) != 0;
    // (from 2^15 points: below, a proof is a chain of launches and the follower's wait for the lead's sort costs more than its own
    // sort beside it — 2^14 constraints 3.88 -> 4.0 ms, 2^16 6.58 -> 6.49 ms, r06)
    static constexpr size_t twin_min = 32768;
    const bool twin_shape = twin_on && n >= twin_min && s.lane >= 0 && s.flat && s.te && tab.contiguous() && tab.scalar_stride == 1 &&
                            tab.shard_world <= 1 && !inf.mask;
    *lead = twin_shape && twin.role == MsmTwin::LEAD && twin.tab2.te && twin.tab2.c == tab.c && twin.tab2.contiguous() &&
             twin.tab2.scalar_stride == 1 && twin.tab2.shard_world <= 1 && msm_flat_applies(twin.tab2, n) &&
             twin.tab2.offset + n <= twin.tab2.stride && tab.offset + n <= tab.stride;
    MsmJob* const l = twin_shape && twin.role == MsmTwin::FOLLOW ? twin.lead : nullptr;
    // the lead's job, scalars and table rows are this one's, and so is the geometry of its arrays
    const bool same = l && l != job && l->active && l->twin.ready && l->twin.scalars == d_scalars && l->n == n && l->twin.mont == mont &&
                      l->twin.tab2.c == tab.c && l->twin.tab2.te == tab.te && l->twin.tab2.stride == tab.stride &&
                      l->twin.tab2.offset == tab.offset && l->twin.geom == geom;
    return same ? l : nullptr;
}

// ---- streams.  Hardware-queue placement, once per context.  ROCm 7 hands its hardware queues (four by default) to streams in creation order,
// bouncing: 1, 2, 3, 4, 4, 3, 2, 1, ... (rocprofv3 Queue_Id, r02).  With the context's stream and the null stream
// first, four auxiliary streams created in a row put the sort and the tail stream on ONE queue: tail(k) and
// sort(k+1) — the two phases that run between consecutive accumulations — executed one after the other
// (2^20 proofs: 73.0 instead of 70.1 ms).  Wanted: the context's stream, the sort stream, the first accumulation
// stream and the tail stream on four different queues (the second accumulation stream may share: accumulations
// cannot overlap, each fills the register files).  A placeholder stream before the tail stream gives that in the
// usual creation history; the result is PROBED (streams_concurrent) and a stream that shares a queue with an
// earlier role is replaced by a fresh one, a few times at most — whatever streams the host application created
// before.
static int msm_setup_streams(swm_ctx* ctx) {
    if (ctx->aux_stream[0]) return SWM_OK;
    const hipStream_t main_stream = ctx->stream;
    // The four streams are created and probed into locals and published to the context only when all of it
    // succeeded: a failure half way must not leave aux_stream[0] set with the later entries null (every later MSM
    // would skip this set-up and silently run its tail on the legacy default stream).
    hipStream_t aux[swm_ctx::MSM_LANES] = {nullptr, nullptr, nullptr, nullptr};
    auto setup = [&]() -> int {
        for (int i = 0; i < 3; i++) SWM_HIP(ctx, msm_create_stream(&aux[i]));
        hipStream_t ph = nullptr;
        SWM_HIP(ctx, hipStreamCreateWithFlags(&ph, hipStreamNonBlocking));
        ctx->spare_streams.push_back(ph);
        SWM_HIP(ctx, msm_create_stream(&aux[3]));
        SWM_HIP(ctx, hipStreamSynchronize(main_stream));
        const int roles[3] = {0, 1, 3};  // sort, accumulation 0, tail
        std::vector<hipStream_t> fixed = {main_stream};
        int budget = 8;  // replacement streams at most
        for (int r : roles) {
            for (;;) {
                bool conc = true;  // with every earlier role
                for (size_t f = 0; f < fixed.size() && conc; f++) SWM_TRY(streams_concurrent(ctx, fixed[f], aux[r], &conc));
                if (conc || budget-- <= 0) break;
                ctx->spare_streams.push_back(aux[r]);  // kept alive: destroying it would free its slot
                aux[r] = nullptr;
                SWM_HIP(ctx, msm_create_stream(&aux[r]));
            }
            fixed.push_back(aux[r]);
        }
        if (!ctx->fork_event) SWM_HIP(ctx, hipEventCreateWithFlags(&ctx->fork_event, hipEventDisableTiming));
        return SWM_OK;
    };
    const int rc = setup();
    if (rc != SWM_OK) {
        for (hipStream_t a : aux)
            if (a) ctx->spare_streams.push_back(a);  // destroyed with the context
        return rc;
    }
    for (int i = 0; i < swm_ctx::MSM_LANES; i++) ctx->aux_stream[i] = aux[i];
    return SWM_OK;
}
// The next pinned result slot for `job`, with its events.
static int msm_take_slot(swm_ctx* ctx, MsmJob* job) {
    if (!ctx->pinned) {  // coherent + mapped: the bucket stage writes its results straight into the slots
        SWM_HIP(ctx, hipHostMalloc(&ctx->pinned, SLOT_BYTES * swm_ctx::MSM_SLOTS, hipHostMallocCoherent | hipHostMallocMapped));
        SWM_HIP(ctx, hipHostGetDevicePointer(&ctx->pinned_dev, ctx->pinned, 0));
    }
    const int slot = ctx->next_slot;
    if (ctx->slot_busy[slot])  // its previous job has not been collected: the download would overwrite live results
        return set_err(ctx, SWM_ERR_INTERNAL, "msm: more than %d jobs in flight", swm_ctx::MSM_SLOTS);
    ctx->next_slot = (ctx->next_slot + 1) % swm_ctx::MSM_SLOTS;
    if (!ctx->slot_event[slot]) SWM_HIP(ctx, hipEventCreateWithFlags(&ctx->slot_event[slot], hipEventDisableTiming));
    job->slot = slot;
    job->host = reinterpret_cast<G1XYZZ*>((char*)ctx->pinned + SLOT_BYTES * slot);
    job->host_flags = reinterpret_cast<const uint32_t*>((char*)job->host + SLOT_FLAGS_OFF);
    job->host_dev = reinterpret_cast<G1XYZZ*>((char*)ctx->pinned_dev + SLOT_BYTES * slot);
    job->host_flags_dev = reinterpret_cast<uint32_t*>((char*)job->host_dev + SLOT_FLAGS_OFF);
    // the bucket stage writes its results straight into the pinned slot (see msm_bucket_reduce; against stream-ordered copies,
    // r02 on one box: 2^16 proofs 11.4 vs 11.8 ms, 2^20 75.1 vs 75.7 ms)
    job->done = ctx->slot_event[slot];
    if (!ctx->acc_event[slot]) SWM_HIP(ctx, hipEventCreateWithFlags(&ctx->acc_event[slot], hipEventDisableTiming));
    job->acc_done = ctx->acc_event[slot];
    if (!ctx->sort_event[slot]) SWM_HIP(ctx, hipEventCreateWithFlags(&ctx->sort_event[slot], hipEventDisableTiming));
    return SWM_OK;
}

// ---- stages (each enqueues on the context's stream)
// FOLLOW: the second sorted array the lead's bin sort wrote; the descriptors: counts, first segments, the list of oversized buckets,
// status words, length histogram, the bins' entry and segment totals, the segments.  Not the cursors and the count of live
// segments, which the lead's msm_seg_order may be advancing at this moment: this job's own stay zero for its own.  The lead's
// zeroed block has this job's layout (msm_twin_match: same geometry).
static int msm_twin_copy_stage(swm_ctx* ctx, const MsmShape& s, const MsmZeroLayout& z, MsmBuffers* b, MsmJob* lead, int slot) {
    const MsmTwinSrc& t = lead->twin;
    SWM_TRY(scratch(ctx, "msmT.sorted", s.total * 4, (void**)&b->sorted));
    SWM_HIP(ctx, hipStreamWaitEvent(ctx->stream, t.sorted, 0));
    TwinCopy tc = TwinCopy();
    auto range = [&](const uint32_t* from, uint32_t* to, size_t words) {
        tc.src[tc.k] = from, tc.dst[tc.k] = to, tc.words[tc.k++] = (uint32_t)words;
    };
    range(t.block + z.hist, b->hist, s.pl.NB + 1);
    range(t.block + z.big_count, b->big_count, 3);
    range(t.block + z.len_hist, b->len_hist, (size_t)(SEG_MAX + 1) * LEN_STRIDE);
    range(t.block + z.flat_off, b->flat_off, 2 * (size_t)FLAT_MAX_BINS + 4);  // flat_off | flat_seg_off
    range(t.seg_off, b->seg_off, s.pl.NB + 1);
    range(t.big_list, b->big_list, s.pl.NB);
    range(t.seg_start, b->seg_start, 2 * s.nseg_max);  // seg_start | seg_len
    SWM_TRY(msm_twin_copy_launch(ctx, tc));
    if (!ctx->twin_copy_event[slot]) SWM_HIP(ctx, hipEventCreateWithFlags(&ctx->twin_copy_event[slot], hipEventDisableTiming));
    SWM_HIP(ctx, hipEventRecord(ctx->twin_copy_event[slot], ctx->stream));
    lead->twin_copied = ctx->twin_copy_event[slot];
    if (t.lane >= 0) ctx->lane_copy_event[t.lane] = ctx->twin_copy_event[slot];
    ctx->stat_msm_twins++;
    return SWM_OK;
}
// The job's zeroed block (MsmZeroLayout): counts, cursors, status words.
static int msm_zero_stage(swm_ctx* ctx, const MsmZeroLayout& z, const MsmBuffers& b) {
    SWM_HIP(ctx, zero_fill_async(b.hist, z.words * 4, ctx->stream));  // (a kernel with issue priority, not the runtime's fill: fill.cuh)
    return SWM_OK;
}
// Stage A: segments ordered by length, one partial sum per segment (msm_accumulate*), oversized buckets folded ahead of the
// bucket stage (msm_big_bucket_sum).
static int msm_accumulate_stage(swm_ctx* ctx, const MsmShape& s, const MsmBuffers& b, const MsmTable& tab, const G1Affine* d_bases,
                                const G1Affine* d_bases28) {
    SWM_TRY(msm_seg_order_stage(ctx, s, b));
    return msm_accumulate_launch(ctx, s, b, tab, d_bases, d_bases28);
}
int msm_enqueue(swm_ctx* ctx, int lane, const G1Affine* d_bases, const G1Affine* d_bases28, const void* d_scalars, size_t n,
                int mont, MsmJob* job, MsmInfMask inf, bool defer_tail, MsmTable tab, MsmTwin twin) {
    job->active = false;
    job->tail_pending = false;
    job->n = n;
    job->twin = MsmTwinSrc();
    job->twin_copied = nullptr;
    job->twin_kept_lane = false;
    if (n == 0) return SWM_OK;
    if (n >= (1ull << 31)) return set_err(ctx, SWM_ERR_INVALID_ARG, "msm: n must be < 2^31");
    ctx->stat_msm_calls++;
    ctx->stat_msm_points += n;
    ctx->log_call('m', n);
    struct SinceWait {  // (counted when this call returns: the choices below see the jobs BEFORE this one)
        swm_ctx* c;
        ~SinceWait() { c->msm_since_wait++; }
    } since_wait{ctx};
    // the job before this one waited to learn whether anything follows it: something does, so its bucket stage takes the
    // thin shape that runs BESIDE this job's sort and accumulation (msm_tail_shape)
    SWM_TRY(msm_launch_lazy_tail(ctx, false));
    MsmShape s;
    SWM_TRY(msm_shape(ctx, n, tab, lane, defer_tail, &s));
    static const bool trace_shape = sw(SW_TRACE) >= 1;
    if (trace_shape) msm_trace_shape(n, s);
    ctx->stat_msm_digits += s.total;
    const MsmZeroLayout z = msm_zero_layout(s);
    const MsmSortGeom geom{z.words, s.nseg_max, s.SEG, s.big_nseg, s.flat_bins};
    bool lead = false;
    MsmJob* const follow = msm_twin_match(job, s, geom, d_scalars, n, mont, inf, tab, twin, &lead);
    // An asynchronous MSM (lane >= 0) is a three-stage pipeline over three auxiliary streams:
    //   S  digits + counting sort          (HBM / LDS-atomic bound)
    //   A  segment planning + accumulation (saturates the integer pipes)      waits for the job's sort
    //   T  bucket stage + download         (a latency-bound chain at one wave per SIMD)   waits for the job's accumulation
    // so that consecutive jobs keep stage A busy back to back while the tail of the previous job and the sort of the
    // next one run beside it.  (r02 timeline: with two lanes that each ran sort -> accumulate -> tail in order, both
    // lanes reached their tails together and ~10 ms of bucket stage per 2^20 proof ran with nothing beside it.)
    // `lane` only selects the scratch set of the per-lane buffers (two sets: a job's sort may overwrite a set once
    // the accumulation that last read it has finished).  lane < 0: everything on the context's stream (K1 ABI).
    // S | A0, A1 by lane | T (two accumulations may overlap: one alone leaves bubbles at the end of its length-sorted grid).
    // Single-stream lanes 0, 1, 2 sit on three different hardware queues (accumulation 0, tail, sort); lane 3 shares the
    // second accumulation stream's queue.
    hipStream_t st_sort = ctx->stream, st_acc = ctx->stream, st_tail = ctx->stream;
    if (s.lane >= 0) {
        SWM_TRY(msm_setup_streams(ctx));
        static const int lane_stream[4] = {1, 3, 0, 2};
        st_sort = ctx->aux_stream[s.one_stream ? lane_stream[s.lane] : 0];
        st_acc = s.one_stream ? st_sort : ctx->aux_stream[1 + (s.lane & 1)];
        st_tail = s.one_stream ? st_sort : ctx->aux_stream[3];  // (a second bucket-stage stream: 51.4 -> 57.4 ms at 2^20, r05)
        SWM_HIP(ctx, hipEventRecord(ctx->fork_event, ctx->stream));
        SWM_HIP(ctx, hipStreamWaitEvent(st_sort, ctx->fork_event, 0));  // the scalars are ready
    }
    SWM_TRY(msm_take_slot(ctx, job));
    const int slot = job->slot;
    job->te = s.te;
    job->quad = s.quad;
    job->low = s.low;
    job->raw = s.raw;
    job->max_blocks = s.max_blocks;
    job->stream = st_tail;
    job->pl = s.rl;
    job->red_blocks = s.red_blocks;
    job->blk_lo = s.blk_lo;
    job->blk_hi = s.blk_hi;
    job->blk_low = s.blk_low;
    job->log_m = s.log_m;
    job->rb = s.rb;
    job->big_nseg = s.big_nseg;

    StreamSwap swap(ctx, st_sort);
    if (follow) {
        // A follower touches nothing of its lane's scratch set — its sorted array and its segment descriptors live in the pair's own
        // buffers, free once the previous pair's follower has accumulated (the lead waited for that before its bin sort) — so the
        // NEXT job may take this lane's set: the caller gets the lane back (pipelined form: job->twin_kept_lane), and that job's sort
        // runs beside the lead's accumulation instead of waiting for it (two sets: the sort of job k + 2 waits for accumulation k).
        job->twin_kept_lane = !s.one_stream;
    } else if (s.lane >= 0) {
        // the scratch set of this lane was last read by the accumulation of the job two back
        // (single-stream jobs too: their stream is not necessarily the one the set's previous reader ran on)
        if (ctx->set_acc_event[s.lane]) SWM_HIP(ctx, hipStreamWaitEvent(st_sort, ctx->set_acc_event[s.lane], 0));
        // ... and, when that job led a twin pair, copied by its follower
        if (ctx->lane_copy_event[s.lane]) SWM_HIP(ctx, hipStreamWaitEvent(st_sort, ctx->lane_copy_event[s.lane], 0));
    }
    MsmBuffers b;
    SWM_TRY(msm_buffers(ctx, s, z, slot, follow != nullptr, &b));
    job->d_acc = b.acc;
    SWM_TRY(msm_zero_stage(ctx, z, b));
    if (follow) {
        SWM_TRY(msm_twin_copy_stage(ctx, s, z, &b, follow, slot));
    } else {
        SWM_TRY(msm_digits_stage(ctx, s, b, d_scalars, n, mont, inf, tab));
        if (lead)  // what the follower takes: the arrays of this job's slot, ready once the bin sort has recorded `sorted`
            job->twin = {false, d_scalars, mont, s.lane, twin.tab2, b.hist, b.seg_start, b.seg_off, b.big_list, geom, ctx->sort_event[slot]};
        if (s.flat) SWM_TRY(msm_sort_flat(ctx, s, b, tab, n, lead ? &job->twin : nullptr));
        else SWM_TRY(msm_sort_windows(ctx, s, b, n));
    }
    if (st_acc != st_sort) {  // stage A
        SWM_HIP(ctx, hipEventRecord(ctx->sort_event[slot], st_sort));
        SWM_HIP(ctx, hipStreamWaitEvent(st_acc, ctx->sort_event[slot], 0));
        ctx->stream = st_acc;
    }
    SWM_TRY(msm_accumulate_stage(ctx, s, b, tab, d_bases, d_bases28));
    job->needs_acc_wait = st_tail != ctx->stream || defer_tail;  // the tail runs on another stream (or later, with others)
    job->d_partial = b.partial;
    job->d_seg_off = b.seg_off;
    job->d_hist = b.hist;
    job->seg = s.SEG;
    job->d_status = b.big_count + 1;
    job->d_entries = msm_entries_word(s, b);
    job->active = true;
    job->tail_pending = true;
    ctx->slot_busy[slot] = true;
    if (s.lane >= 0 || defer_tail) {
        SWM_HIP(ctx, hipEventRecord(job->acc_done, ctx->stream));
        if (s.lane >= 0 && !follow) ctx->set_acc_event[s.lane] = job->acc_done;
        if (follow) ctx->twin_sorted_event = job->acc_done;
    }
    job->joint_tail = defer_tail;
    if (defer_tail) {  // the bucket stage runs with the other jobs of the round (msm_flush_tails)
        ctx->pending_tails.push_back(job);
        return SWM_OK;
    }
    if (s.flat && !s.lat && s.lane >= 0 && s.rb == 256 && tab.shard_world <= 1) {
        ctx->lazy_tail = job;  // shaped and launched by the next msm_enqueue (thin) or by the flush of the round (wide)
        return SWM_OK;
    }
    MsmJob* one[1] = {job};
    return msm_launch_tails(ctx, one, 1);
}

// Shape of the bucket stage of a large flat job (r04).  The stage is a dependent chain of group operations — 2 m for the walk
// over the m buckets of a lane plus ~20 across the workgroup — on (2^(c-1) / m) / 256 workgroups of 144 KB of LDS each.  With
// m = 8 that is one workgroup on EVERY CU for ~0.5 ms: nothing that needs LDS (the partition and the bin sort of the next
// job) runs beside it, and the r04 timeline showed exactly that serialisation between consecutive accumulations.  With
// m = 32 the chain is ~84 steps (~1 ms) on a quarter of the CUs: as CU-time half the cost, and the rest of the chip goes
// on with the next job.  So: WIDE (m = 8, shortest chain) when the stage is exposed — the last job before a flush, i.e. of
// a prover round —, THIN (m = 32) when another job follows.  The job's result slot takes up to 256 workgroup results either way.
static void msm_tail_shape(MsmJob* j, bool wide) {
    // log2 buckets per lane: thin 32 (16 / 8 per lane: 51.5 / 52.5 vs 52.0 ms, r05); wide 4 before the workgroup cap applies
    // (the cap is the job's max_blocks: 256, which makes it 8 per lane for 2^19 buckets)
    static constexpr unsigned thin_log_m = 5u, wide_log_m = 2u;
    j->log_m = wide ? wide_log_m : thin_log_m;
    j->red_blocks = bucket_blocks(j->pl.maxB, j->rb, j->max_blocks, &j->log_m);
    j->blk_hi = j->red_blocks;  // (no bucket-range share on this path: blk_lo = 0, blk_low = 0)
}
// Measured in r06 and not kept (CHANGELOG.md): (i) the WIDE stage with four lanes per chain (msm_bucket_reduce<256, FormTEQuad>, 1024
// threads per workgroup, four waves per SIMD on the same 144 KB): 554 instead of 462 us per 2^19-bucket job — the quad form's 12
// products per addition and its lane exchanges cost more than the idle lanes of the tree steps; (ii) the second operand of every step
// in registers, the partial sum of a lane's NEXT walk step requested from HBM while the current addition runs (the three flat-load
// waits per "run += partial" step gone, 240 VGPRs): 524 instead of 467 us — the lone wave's cycles without an issue are not its
// operand loads (with typed loads of the whole operand up front, one wait instead of three and nothing else changed: 462.8 vs 463.3 us).
// What those cycles WERE: LDS bank conflicts and barriers — see RedSlot and the walk's wave-level vote (msm_bucket_reduce).
int msm_launch_lazy_tail(swm_ctx* ctx, bool wide) {
    MsmJob* j = ctx->lazy_tail;
    if (!j) return SWM_OK;
    ctx->lazy_tail = nullptr;
    msm_tail_shape(j, wide);
    MsmJob* one[1] = {j};
    return msm_launch_tails(ctx, one, 1);
}

// One bucket-stage launch + the downloads for k <= TAIL_MAX jobs, on the stream of the last one.
int msm_launch_tails(swm_ctx* ctx, MsmJob** jobs, int k) {
    if (k <= 0) return SWM_OK;
    const hipStream_t st = jobs[k - 1]->stream;
    StreamSwap swap(ctx, st);
    TailBatch batch;
    memset(&batch, 0, sizeof(batch));
    unsigned max_red = 1, max_win = 1;
    for (int i = 0; i < k; i++) {
        MsmJob* j = jobs[i];
        if (j->acc_done && j->stream != nullptr && j->needs_acc_wait) SWM_HIP(ctx, hipStreamWaitEvent(st, j->acc_done, 0));
        batch.j[i].partial = j->d_partial;
        batch.j[i].seg_off = j->d_seg_off;
        batch.j[i].hist = j->d_hist;
        batch.j[i].seg = j->seg;
        batch.j[i].out = j->host_dev;
        batch.j[i].acc = j->d_acc;
        batch.j[i].status = j->d_status;
        batch.j[i].entries = j->d_entries;
        batch.j[i].host_flags = j->host_flags_dev;
        batch.j[i].log_m = j->log_m;
        batch.j[i].red_blocks = j->red_blocks;
        batch.j[i].blk_lo = j->blk_lo;
        batch.j[i].blk_hi = j->blk_hi;
        batch.j[i].blk_low = j->blk_low;
        batch.j[i].big_nseg = j->big_nseg;
        batch.j[i].L = j->pl;
        max_red = std::max(max_red, j->red_blocks);
        max_win = std::max(max_win, j->pl.nwin);
    }
    const bool te = jobs[0]->te;  // every job of a launch has the same point form (msm_flush_tails groups them)
    // (jobs per stage kernel, for tests that hold a shape to the path it is meant to take: quad | low-LDS | wide / thin | XYZZ)
    const MsmTailKernel kernel = jobs[0]->quad ? TAIL_QUAD : (te && jobs[0]->low ? TAIL_LOW : (te ? TAIL_TE29 : TAIL_XYZZ));
    ctx->stat_msm_tails[kernel] += (uint64_t)k;
    SWM_TRY(msm_tail_launch(ctx, batch, k, kernel, jobs[0]->rb, max_red, max_win));
    for (int i = 0; i < k; i++) {
        SWM_HIP(ctx, hipEventRecord(jobs[i]->done, st));
        jobs[i]->tail_pending = false;
    }
    return SWM_OK;
}

// Shape of a JOINT stage (r05): the jobs of one launch share the chip, so they share its 256 CUs — the smallest common number
// of buckets per lane (a power of two from 4) with which the workgroups of all k jobs fit one per CU.  One job: 8 per lane on
// every CU (the wide shape); two 2^19-bucket jobs: 16 per lane, 128 workgroups each; four: 32 per lane; a round of three
// 2^17-bucket jobs and one of 2^19 (the Merkle circuit's round 1 with its prefix tables): 16 per lane, 32 + 32 + 32 + 128.
// (r02 - r04: 64 workgroups per job whatever the job.)
static void msm_joint_shape(MsmJob** jobs, size_t k) {
    for (size_t i = 0; i < k; i++)  // one-lane 256-chain stages over ONE bucket set, no bucket-range share
        if (jobs[i]->rb != 256 || jobs[i]->quad || jobs[i]->pl.nwin != 1 || jobs[i]->blk_lo != 0 || jobs[i]->blk_low != 0 ||
            jobs[i]->blk_hi != jobs[i]->red_blocks)
            return;
    for (unsigned log_m = 2; log_m <= 10; log_m++) {
        unsigned total = 0;
        bool ok = true;
        for (size_t i = 0; i < k; i++) {
            unsigned lm = log_m;
            total += bucket_blocks(jobs[i]->pl.maxB, jobs[i]->rb, jobs[i]->max_blocks, &lm);
            ok = ok && lm == log_m;  // (fits: bucket_blocks did not have to raise it)
        }
        if (!ok || total > 256) continue;
        for (size_t i = 0; i < k; i++) {
            jobs[i]->log_m = log_m;
            jobs[i]->red_blocks = bucket_blocks(jobs[i]->pl.maxB, jobs[i]->rb, jobs[i]->max_blocks, &jobs[i]->log_m);
            jobs[i]->blk_hi = jobs[i]->red_blocks;
        }
        return;
    }
}

// Launches the deferred bucket stages (all jobs enqueued with defer_tail since the last flush), TAIL_MAX per launch.
int msm_flush_tails(swm_ctx* ctx) {
    SWM_TRY(msm_launch_lazy_tail(ctx, true));  // nothing follows it before the round's results are awaited
    std::vector<MsmJob*> jobs;
    jobs.swap(ctx->pending_tails);
    for (size_t i = 0; i < jobs.size();) {  // one launch per run of up to TAIL_MAX jobs of the same workgroup width
        size_t k = 1;
        while (i + k < jobs.size() && k < TAIL_MAX && jobs[i + k]->rb == jobs[i]->rb && jobs[i + k]->te == jobs[i]->te &&
               jobs[i + k]->quad == jobs[i]->quad && jobs[i + k]->low == jobs[i]->low)
            k++;
        msm_joint_shape(jobs.data() + i, k);
        SWM_TRY(msm_launch_tails(ctx, jobs.data() + i, (int)k));
        i += k;
    }
    return SWM_OK;
}

// Waits for a job's download, releases its slot and checks the status words.
static int msm_finish_wait(swm_ctx* ctx, MsmJob* job) {
    if (job->tail_pending) SWM_TRY(msm_flush_tails(ctx));  // awaited before its round was flushed
    // a twin's follower copies this job's descriptors out of the slot's arrays: the slot is not handed on before that
    if (job->twin_copied) (void)hipEventSynchronize(job->twin_copied);
    job->twin_copied = nullptr;
    job->twin.ready = false;
    const hipError_t werr = hipEventSynchronize(job->done);
    job->active = false;
    ctx->slot_busy[job->slot] = false;  // released whatever the wait returned: the slot must not stay blocked for good
    SWM_HIP(ctx, werr);
    ctx->stat_msm_adds += job->host_flags[1];  // entries the sort placed = non-zero digits
    ctx->stat_msm_zero_points += job->host_flags[2];
    if (job->host_flags[0])
        return set_err(ctx, SWM_ERR_INVALID_ARG, "msm: a scalar is not a canonical field element (>= r)");
    return SWM_OK;
}

// point form of a job's workgroup results on the host: XYZZ, or extended twisted Edwards (job->te; g1.cuh)
struct HostXYZZ {
    static G1XYZZ identity() { return g1_xyzz_identity(); }
    static void add(G1XYZZ& a, const G1XYZZ& q) { g1_add(a, q); }
    static G1XYZZ dbl(const G1XYZZ& p) { return g1_dbl(p); }
    static bool is_inf(const G1XYZZ& p) { return g1_is_inf(p); }
    static G1XYZZ to_xyzz(const G1XYZZ& p) { return p; }
};
struct HostTE {
    static G1XYZZ identity() { return g1te_identity(); }
    static void add(G1XYZZ& a, const G1XYZZ& q) { g1te_add(a, q); }
    static G1XYZZ dbl(const G1XYZZ& p) { return g1te_dbl(p); }
    static bool is_inf(const G1XYZZ& p) { return fp_is_zero(p.x) && fp_eq(p.y, p.zzz); }  // (0 : z : 0 : z)
    static G1XYZZ to_xyzz(const G1XYZZ& p) { return g1te_to_xyzz(p); }
};
// over the workgroups blk in [lo, hi): sum of A, sum of R, and sum of (blk - lo) R_blk by suffix sums
template <class HF>
static void fold_range(const G1XYZZ* h, unsigned lo, unsigned hi, G1XYZZ* sa_out, G1XYZZ* sr_out, G1XYZZ* wt_out) {
    G1XYZZ sa = HF::identity(), suffix = HF::identity(), wt = HF::identity();
    for (unsigned blk = hi; blk-- > lo;) {
        HF::add(sa, h[2 * blk]);
        HF::add(suffix, h[2 * blk + 1]);                // Suffix_blk = sum_{u >= blk} R_u
        if (blk > lo) HF::add(wt, suffix);              // sum_{blk > lo} Suffix_blk = sum (blk - lo) R_blk
    }
    *sa_out = sa;
    *sr_out = suffix;
    *wt_out = wt;
}
// flat schedule: one window, up to 256 workgroups, folded in groups of 16 consecutive workgroups (independent: host
// workers); with g0 = 16 g the first workgroup of group g:  sum blk R_blk = sum_g [W_g + 16 g SR_g], and sum_g g SR_g
// comes from suffix sums over the groups, times 16 by four doublings.
static constexpr unsigned FOLD_GROUP = 16;
template <class HF>
static void fold_groups_combine(const G1XYZZ* ga, const G1XYZZ* gr, const G1XYZZ* gw, unsigned G, G1XYZZ* sum_a, G1XYZZ* weighted) {
    G1XYZZ sa = HF::identity(), wsum = HF::identity(), suffix = HF::identity(), gsum = HF::identity();
    for (unsigned g = G; g-- > 0;) {
        HF::add(sa, ga[g]);
        HF::add(wsum, gw[g]);
        HF::add(suffix, gr[g]);
        if (g > 0) HF::add(gsum, suffix);  // sum_g g SR_g
    }
    for (int k = 0; k < 4; k++) gsum = HF::dbl(gsum);
    static_assert(FOLD_GROUP == 16, "four doublings");
    HF::add(wsum, gsum);
    *sum_a = sa;
    *weighted = wsum;
}

// Host fold of a job's downloaded workgroup results.  `pool`: the context's host workers for the independent parts of
// ONE job (null: serial — the caller is already folding several jobs side by side).  Returns false on an inconsistent
// window layout (internal error).
// `groups` (flat schedule, more than one group): the group sums (ga | gr | gw, G each) were already computed by the caller.
template <class HF>
static bool msm_fold_form(const MsmJob* job, HostPool* pool, G1XYZZ* result, const G1XYZZ* groups) {
    // host: per window  X_w = sum_blk A_blk + 2^shift * W_w,  W_w = sum_blk blk R_blk  (2^shift = RED_BLOCK * m buckets per
    // workgroup; W_w by suffix sums over the <= 16 workgroups).  The windows are independent: they are folded on the
    // context's host workers.  Then Horner over the windows (high -> low, c_w doublings each), with the 2^shift of W_w
    // riding on the window's own doublings:  T <- 2^shift (2^(c_w - shift) T + W_w) + sum_blk A_blk.
    const WinLayout& pl = job->pl;
    const unsigned nb = job->red_blocks;
    unsigned shift = job->log_m;
    for (unsigned v = job->rb; v > 1; v >>= 1) shift++;
    G1XYZZ sum_a[MAX_WIN], weighted[MAX_WIN];
    auto fold_window = [&](int w) {
        G1XYZZ sr;
        fold_range<HF>(job->host + (size_t)w * nb * 2, 0, nb, &sum_a[w], &sr, &weighted[w]);
    };
    auto run = [&](int n, const std::function<void(int)>& fn) {
        if (pool) pool->parallel_for(n, fn);
        else
            for (int i = 0; i < n; i++) fn(i);
    };
    if (pl.nwin == 1 && nb > FOLD_GROUP && (pool || groups)) {
        const unsigned G = (nb + FOLD_GROUP - 1) / FOLD_GROUP;
        std::vector<G1XYZZ> own;
        if (!groups) {
            own.resize(3 * (size_t)G);
            G1XYZZ* o = own.data();
            run((int)G, [&](int g) {
                fold_range<HF>(job->host, FOLD_GROUP * g, std::min(nb, FOLD_GROUP * (g + 1)), &o[g], &o[G + g], &o[2 * G + g]);
            });
            groups = o;
        }
        fold_groups_combine<HF>(groups, groups + G, groups + 2 * G, G, &sum_a[0], &weighted[0]);
    } else if (nb > 1 && pl.nwin > 1) {
        run((int)pl.nwin, fold_window);
    } else {
        for (unsigned w = 0; w < pl.nwin; w++) fold_window((int)w);
    }
    G1XYZZ total_pt = HF::identity();
    for (unsigned w = pl.nwin; w-- > 0;) {
        unsigned cw = pl.c[w];
        if (!HF::is_inf(weighted[w])) {
            if (cw >= shift) {
                for (unsigned k = shift; k < cw; k++) total_pt = HF::dbl(total_pt);
                HF::add(total_pt, weighted[w]);
                cw = shift;
            } else {  // a window narrower than one workgroup's span cannot have content beyond workgroup 0
                return false;
            }
        }
        for (unsigned k = 0; k < cw; k++) total_pt = HF::dbl(total_pt);
        HF::add(total_pt, sum_a[w]);
    }
    *result = HF::to_xyzz(total_pt);
    return true;
}
static bool msm_fold(const MsmJob* job, HostPool* pool, G1XYZZ* result, const G1XYZZ* groups = nullptr) {
    return job->te ? msm_fold_form<HostTE>(job, pool, result, groups) : msm_fold_form<HostXYZZ>(job, pool, result, groups);
}

// Host workers of a context: 15 (7 on hosts with fewer than 32 hardware threads), but never more than this process's share of
// the machine: hardware threads / ranks on the node (LOCAL_WORLD_SIZE of the launcher, or the context's shard world for ranks
// that are threads of one process) minus the proving thread — eight ranks with 15 polling workers each would be 120 spinning
// threads beside the provers, torch and the RCCL proxies.  SWM_POOL_WORKERS overrides.
HostPool* host_pool_of(swm_ctx* ctx) {
    if (!ctx->host_pool) {
        unsigned hw = std::thread::hardware_concurrency();
        unsigned want = hw > 1 ? std::min(hw - 1, hw >= 32 ? 15u : 7u) : 0u;
        unsigned ranks = std::max(1u, ctx->shard_world);
        ranks = std::max(ranks, (unsigned)sw(SW_LOCAL_WORLD_SIZE));  // (torchrun's: ranks that share this host's cores)
        if (ranks > 1 && hw) want = std::min(want, std::max(1u, hw / ranks) - 1);
        if (const long forced = sw(SW_POOL_WORKERS); forced >= 0) want = (unsigned)forced;  // (diagnostic: the host fold's worker threads)
        ctx->host_pool = new HostPool(want);
    }
    return ctx->host_pool;
}
// how long the workers poll for the fold that follows a wait (microseconds, 0 = they sleep)
static unsigned pool_spin_us() { return (unsigned)sw(SW_POOL_SPIN_US); }

int msm_finish(swm_ctx* ctx, MsmJob* job, G1XYZZ* result) {
    *result = g1_xyzz_identity();
    ctx->msm_since_wait = 0;
    if (!job->active) return SWM_OK;
    static const bool trace = sw(SW_TRACE) >= 1;
    auto tw0 = std::chrono::steady_clock::now();
    if (pool_spin_us()) host_pool_of(ctx)->arm(pool_spin_us());  // the fold follows the wait at once: the workers poll for it meanwhile
    SWM_TRY(msm_finish_wait(ctx, job));
    auto tw1 = std::chrono::steady_clock::now();
    if (!msm_fold(job, host_pool_of(ctx), result)) return set_err(ctx, SWM_ERR_INTERNAL, "msm: inconsistent window fold");
    if (trace)
        fprintf(stderr, "[swm trace]   msm_finish n=%zu: waited %.3f ms, host fold %.3f ms\n", job->n,
                std::chrono::duration<double, std::milli>(tw1 - tw0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw1).count());
    return SWM_OK;
}

// Several jobs at once (the commitments of a prover round): wait for all of them, then fold them side by side, one job
// per host worker (a fold is a serial chain of ~3 additions per workgroup result: four of them back to back were
// ~0.25 ms between the last kernel of a round and its Fiat-Shamir challenge).
int msm_finish_many(swm_ctx* ctx, MsmJob** jobs, int k, G1XYZZ* results) {
    static const bool trace = sw(SW_TRACE) >= 1;
    ctx->msm_since_wait = 0;
    auto tw0 = std::chrono::steady_clock::now();
    std::vector<int> live;
    for (int i = 0; i < k; i++) {
        results[i] = g1_xyzz_identity();
        if (jobs[i] && jobs[i]->active) live.push_back(i);
    }
    int rc = SWM_OK;
    if (!live.empty() && pool_spin_us()) host_pool_of(ctx)->arm(pool_spin_us());  // the folds follow the wait at once: the workers poll for them meanwhile
    // Jobs with their own tail finish one after the other (the tail stream runs them in order): each is folded as soon as
    // its results are there, while the GPU is still busy with the tails of the later ones — only the last fold is exposed.
    // Jobs of one joint tail launch finish together: those are folded side by side below.
    bool pipelined = false;
    for (int i : live) pipelined = pipelined || !jobs[i]->joint_tail;
    if (pipelined && live.size() > 1) {
        bool ok_all = true;
        for (int i : live) {
            int r = msm_finish_wait(ctx, jobs[i]);
            if (rc == SWM_OK) rc = r;
            if (r == SWM_OK && !msm_fold(jobs[i], host_pool_of(ctx), &results[i])) ok_all = false;
        }
        if (rc != SWM_OK) return rc;
        if (!ok_all) return set_err(ctx, SWM_ERR_INTERNAL, "msm: inconsistent window fold");
        if (trace)
            fprintf(stderr, "[swm trace]   msm_finish_many k=%zu: waits and folds interleaved, %.3f ms\n", live.size(),
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count());
        return SWM_OK;
    }
    for (int i : live) {  // every job is waited for and released even if one reports an error
        int r = msm_finish_wait(ctx, jobs[i]);
        if (rc == SWM_OK) rc = r;
    }
    if (rc != SWM_OK) return rc;
    auto tw1 = std::chrono::steady_clock::now();
    // tasks: one per group of 16 workgroup results of a flat job, one per job otherwise
    struct Task {
        int job;
        int group;  // -1: the whole job
    };
    std::vector<Task> tasks;
    std::vector<std::vector<G1XYZZ>> groups(live.size());
    for (size_t t = 0; t < live.size(); t++) {
        const MsmJob* j = jobs[live[t]];
        if (j->pl.nwin == 1 && j->red_blocks > FOLD_GROUP) {
            const unsigned G = (j->red_blocks + FOLD_GROUP - 1) / FOLD_GROUP;
            groups[t].resize(3 * (size_t)G);
            for (unsigned g = 0; g < G; g++) tasks.push_back({(int)t, (int)g});
        } else {
            tasks.push_back({(int)t, -1});
        }
    }
    std::vector<char> ok(live.size(), 1);
    host_pool_of(ctx)->parallel_for((int)tasks.size(), [&](int i) {
        const Task& tk = tasks[i];
        const MsmJob* j = jobs[live[tk.job]];
        if (tk.group < 0) {
            ok[tk.job] = msm_fold(j, nullptr, &results[live[tk.job]]);
        } else {
            const unsigned G = (j->red_blocks + FOLD_GROUP - 1) / FOLD_GROUP, g = (unsigned)tk.group;
            G1XYZZ* o = groups[tk.job].data();
            if (j->te) fold_range<HostTE>(j->host, FOLD_GROUP * g, std::min(j->red_blocks, FOLD_GROUP * (g + 1)), &o[g], &o[G + g], &o[2 * G + g]);
            else fold_range<HostXYZZ>(j->host, FOLD_GROUP * g, std::min(j->red_blocks, FOLD_GROUP * (g + 1)), &o[g], &o[G + g], &o[2 * G + g]);
        }
    });
    host_pool_of(ctx)->parallel_for((int)live.size(), [&](int t) {  // per job: the combine of its group sums
        if (!groups[t].empty()) ok[t] = msm_fold(jobs[live[t]], nullptr, &results[live[t]], groups[t].data());
    });
    for (char c : ok)
        if (!c) return set_err(ctx, SWM_ERR_INTERNAL, "msm: inconsistent window fold");
    if (trace)
        fprintf(stderr, "[swm trace]   msm_finish_many k=%zu: waited %.3f ms, host folds %.3f ms\n", live.size(),
                std::chrono::duration<double, std::milli>(tw1 - tw0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw1).count());
    return SWM_OK;
}

// Synchronous form on the context's stream (K1 ABI).
int msm_run(swm_ctx* ctx, const G1Affine* d_bases, const G1Affine* d_bases28, const void* d_scalars, size_t n, int mont,
            G1XYZZ* result, MsmInfMask inf, MsmTable tab) {
    MsmJob job;
    SWM_TRY(msm_enqueue(ctx, -1, d_bases, d_bases28, d_scalars, n, mont, &job, inf, false, tab));
    return msm_finish(ctx, &job, result);
}

// ---------------------------------------------------------------------------------------------- sort self-test
// One job up to and including msm_seg_order, through the functions msm_enqueue runs and in its order, on the context's stream;
// then everything the stage left for the accumulation and the bucket stage is downloaded (include/swmarlin.h:
// swm_selftest_msm_sort).  lane -1 as msm_run, lane 0 with a follower's table (a LEAD needs a lane: msm_twin_match).  The job takes
// no result slot: it uses the scratch of the slot the next job will get, which must be free, and has synchronised when it returns.
int msm_selftest_sort(swm_ctx* ctx, const void* d_scalars, size_t n, int mont, MsmInfMask inf, bool defer_tail, MsmTable tab,
                      const MsmTable* tab2, MsmSortDump* out, bool run) {
    if (n == 0 || n >= (1ull << 31)) return set_err(ctx, SWM_ERR_INVALID_ARG, "selftest_msm_sort: n must be in [1, 2^31)");
    MsmShape s;
    SWM_TRY(msm_shape(ctx, n, tab, tab2 ? 0 : -1, defer_tail, &s));
    const MsmZeroLayout z = msm_zero_layout(s);
    const MsmSortGeom geom{z.words, s.nseg_max, s.SEG, s.big_nseg, s.flat_bins};
    MsmTwin twin;
    if (tab2) {
        twin.role = MsmTwin::LEAD;
        twin.tab2 = *tab2;
    }
    bool lead = false;
    (void)msm_twin_match(nullptr, s, geom, d_scalars, n, mont, inf, tab, twin, &lead);
    out->flat = s.flat, out->te = s.te, out->lat = s.lat, out->quad = s.quad, out->raw = s.raw, out->interleave = msm_interleaves(s);
    out->lead = lead;
    out->pl = s.pl;
    out->total = s.total, out->nseg_max = s.nseg_max;
    out->SEG = s.SEG, out->big_nseg = s.big_nseg, out->log_g = s.log_g, out->flat_fb = s.flat_fb, out->flat_bins = s.flat_bins;
    out->tstride = (uint32_t)tab.stride;
    if (!run) return SWM_OK;
    const int slot = ctx->next_slot;
    if (ctx->slot_busy[slot] || ctx->msm_since_wait) return set_err(ctx, SWM_ERR_INTERNAL, "selftest_msm_sort: MSM jobs in flight");
    MsmBuffers b;
    SWM_TRY(msm_buffers(ctx, s, z, slot, false, &b));
    // words the stage never writes read back as 0xFFFFFFFF
    uint32_t* sorted2 = nullptr;
    SWM_HIP(ctx, hipMemsetAsync(b.sorted, 0xFF, s.total * 4, ctx->stream));
    SWM_HIP(ctx, hipMemsetAsync(b.seg_start, 0xFF, s.nseg_max * 12, ctx->stream));  // seg_start | seg_len | order
    SWM_HIP(ctx, hipMemsetAsync(b.big_list, 0xFF, (size_t)s.pl.NB * 4, ctx->stream));
    MsmTwinSrc src;
    if (lead) {
        SWM_TRY(scratch(ctx, "msmT.sorted", s.total * 4, (void**)&sorted2));  // (the buffer msm_sort_flat asks for)
        SWM_HIP(ctx, hipMemsetAsync(sorted2, 0xFF, s.total * 4, ctx->stream));
        if (!ctx->sort_event[slot]) SWM_HIP(ctx, hipEventCreateWithFlags(&ctx->sort_event[slot], hipEventDisableTiming));
        src = {false, d_scalars, mont, s.lane, twin.tab2, b.hist, b.seg_start, b.seg_off, b.big_list, geom, ctx->sort_event[slot]};
    }
    SWM_TRY(msm_zero_stage(ctx, z, b));
    SWM_TRY(msm_digits_stage(ctx, s, b, d_scalars, n, mont, inf, tab));
    if (s.flat) SWM_TRY(msm_sort_flat(ctx, s, b, tab, n, lead ? &src : nullptr));
    else SWM_TRY(msm_sort_windows(ctx, s, b, n));
    SWM_TRY(msm_seg_order_stage(ctx, s, b));
    const size_t NB = s.pl.NB;
    auto down = [&](void* to, const void* from, size_t words) {
        return to && words ? hipMemcpyAsync(to, from, words * 4, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
    };
    std::vector<uint32_t> lens((size_t)(s.SEG + 1) * LEN_STRIDE);
    SWM_HIP(ctx, down(out->hist, b.hist, NB));
    SWM_HIP(ctx, down(out->bucket_off, b.bucket_off, NB));
    SWM_HIP(ctx, down(out->seg_off, b.seg_off, NB));
    SWM_HIP(ctx, down(out->sorted, b.sorted, s.total));
    SWM_HIP(ctx, down(out->seg_start, b.seg_start, s.nseg_max));
    SWM_HIP(ctx, down(out->seg_len, b.seg_len, s.nseg_max));
    SWM_HIP(ctx, down(out->order, b.order, s.nseg_max));
    SWM_HIP(ctx, down(out->big_list, b.big_list, NB));
    if (lead) SWM_HIP(ctx, down(out->sorted2, sorted2, s.total));
    SWM_HIP(ctx, down(lens.data(), b.len_hist, lens.size()));
    SWM_HIP(ctx, down(out->status, b.big_count, 4));  // big_count | bad scalar | points that contribute nothing | live segments
    SWM_HIP(ctx, down(&out->seg_bound, msm_seg_space(s, b), 1));
    SWM_HIP(ctx, down(&out->entries, msm_entries_word(s, b), 1));
    SWM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (out->len_hist)
        for (uint32_t i = 0; i <= s.SEG; i++) out->len_hist[i] = lens[(size_t)i * LEN_STRIDE];
    return SWM_OK;
}

}  // namespace swm

// msm_stages.h — what the units of the G1 MSM share among themselves: msm.hip (driver), msm_sort.hip, msm_table.hip, msm_stages.hip,
// msm_selftest.hip.  The rest of the library sees msm.h only.  A kernel is launched, and its attributes are set, in the unit that
// defines it: the units export the host functions declared at the end of this file, never kernels.
#pragma once
#include "msm.h"

namespace swm {

// ---------------------------------------------------------------------------------------------- parameters
static constexpr int SEG_MAX = 128;     // points per accumulation segment: upper bound, chosen per MSM (msm_seg_bound)
static constexpr int BIG_NSEG = 16;     // buckets with more segments than this are folded by a whole workgroup
static constexpr int RED_BLOCK = 256;
static constexpr uint32_t PART_MAX_BINS = 1024;
static constexpr uint32_t FLAT_MAX_BINS = 4096;
static constexpr uint32_t FLAT_MAX_FINE = 2048;  // buckets per bin at most (2^fb): fine counts + offsets (16 KB) next to the 128-KB stage
// The per-bin cursors of msm_flat_partition sit one per 128-byte line: every workgroup of the launch reserves its runs with
// one returning atomic per bin, and packed (32 cursors to a line) those atomics queued up behind one another at the
// memory side — 135 of the kernel's 191 us at 2^20 points (measured by replacing the atomic with arithmetic).
static constexpr uint32_t FLAT_CUR_STRIDE = 32;   // = the most windows a table can have (msm_flat_applies): one cursor per (bin, window)
static constexpr uint32_t LEN_STRIDE = 32;  // the SEG + 1 length counters sit one per 128-byte line (see FLAT_CUR_STRIDE)
// segments of a bucket with cnt entries (the sort writes them, the point stages walk them)
__device__ __forceinline__ uint32_t nseg_of(uint32_t cnt, uint32_t seg) { return (cnt + seg - 1) / seg; }
static constexpr int SCAN_BLOCK = 256;
static constexpr int SCAN_ITEMS = 8;  // consecutive buckets per lane
static constexpr int SCAN_TILE = SCAN_BLOCK * SCAN_ITEMS;
static constexpr int TAIL_MAX = 4;  // jobs per bucket-stage launch (msm_stages.hip, "Batch form")

// ---------------------------------------------------------------------------------------------- structs
// Bucket-range split of one proof over several ranks (MsmTable::shard_world): a digit of a full-width window is kept when
// its bucket lies in [blo, bhi), a digit of a narrower window when its point lies in [plo, phi).
struct DigitShard {
    uint32_t on, cfull, blo, bhi;
    uint64_t plo, phi;
};
struct BinPlan {
    uint8_t fb[MAX_WIN];      // fine bits of window w: bin = bucket >> fb[w], at most 128 buckets per bin
    uint16_t nbins[MAX_WIN];  // bins that can be non-empty in window w
    uint32_t max_nbins;
};
// The follower of a twin pair takes the lead's bucket and segment descriptors: up to eight word ranges, one launch.
struct TwinCopy {
    const uint32_t* src[8];
    uint32_t* dst[8];
    uint32_t words[8];
    int k;
};
// One launch of the bucket stage (msm_stages.hip: msm_bucket_reduce[_low]): filled by the driver's msm_launch_tails.
struct TailJob {
    const void* partial;  // points of the launch's form (Form::Pt): 28-bit slots, or raw 29-bit points when the job is MsmJob::raw
    const uint32_t *seg_off, *hist;  // first segment and entry count of every bucket: its segments are seg_off[b] .. + ceil(hist[b] / seg)
    uint32_t seg;
    G1XYZZ* out;
    void* acc;  // msm_bucket_reduce_low: the weighted sums of the lanes, one slot per lane in HBM / L2 (red_blocks x RB per window)
    unsigned log_m, red_blocks, big_nseg;
    unsigned blk_lo, blk_hi, blk_low;   // workgroups of this rank's bucket share (MsmJob); the others only emit the identity
    const uint32_t *status, *entries;  // device status words of the job, forwarded to ...
    uint32_t* host_flags;              // ... the tail of its pinned result slot
    WinLayout L;
};
struct TailBatch {
    TailJob j[TAIL_MAX];
};
// ---- shape: every decision about one MSM, made by msm_shape (which says what each field is); the bucket-stage fields are MsmJob's.
struct MsmShape {
    bool flat, te, lat, quad, low, quad_acc, one_stream, two_level, raw;
    int lane;
    WinLayout pl, rl;
    size_t total, wpart_n, nseg_max;
    unsigned rb, max_blocks, log_m, red_blocks, blk_lo, blk_hi, blk_low, log_g, scan_tiles, flat_fb;
    uint32_t SEG, big_nseg, flat_bins;
    DigitShard dshard;
    BinPlan bp;
};
// The block a job zeroes before its sort (one fill, per result slot), as word offsets: hist [NB + 1] entries per bucket | cursor
// [NB + 1] (msm_scatter) | big_count [4]: oversized buckets, the two status words (msm_digits), segments that hold entries (the
// count of msm_seg_order) | len_hist, len_cursor: the segments per length and the run cursors of msm_seg_order, one per length
// class | two_level_bad: one flag per window, then bin_cursor: the per-(window, bin) cursors | flat schedule: [windows x bins]
// counts (room for 32 windows) | [bins x 32] offsets | [bins x 32] cursors (one 128-byte line per bin each) | [bins + 1] offsets |
// [bins + 1] first segment index (the [bins x 32] blocks start on 128-byte lines: vector loads / stores of a bin's windows)
struct MsmZeroLayout {
    size_t hist, cursor, big_count, len_hist, len_cursor, two_level_bad, bin_cursor;
    size_t flat_cnt, flat_win_off, flat_cur, flat_off, flat_seg_off;
    size_t words;  // whole 256-byte lines: the runtime then clears them with one kernel, not two
};
// The device arrays of a job (the driver's msm_buffers).
struct MsmBuffers {
    uint32_t *hist, *cursor, *big_count, *len_hist, *len_cursor, *two_level_bad, *bin_cursor;  // the zeroed block (MsmZeroLayout)
    uint32_t *flat_cnt, *flat_win_off, *flat_cur, *flat_off, *flat_seg_off;
    uint32_t *seg_start, *seg_len, *order, *bucket_off, *seg_off, *digits, *sorted, *tot_cnt, *tot_seg, *big_list;
    uint2* pairs;
    // partial[nseg_max] (then room for wpart_n points); the low-LDS bucket stage's sums, one point per lane — G1XYZZ, or TE29Pt (MsmShape::raw)
    void *partial, *acc;
};
// do the segments of a bucket with more than SEG entries take its entries round-robin (FlatSegOut::interleave)?
static bool msm_interleaves(const MsmShape& s) { return s.flat && s.te; }
static uint32_t* msm_nseg_live(const MsmBuffers& b) { return b.big_count + 3; }  // segments that hold entries = lanes of work for the accumulation
// segment indices in use (a device word): the flat schedule's bins hand them out by capacity, the per-window schedule densely
static const uint32_t* msm_seg_space(const MsmShape& s, const MsmBuffers& b) { return s.flat ? b.flat_seg_off + s.flat_bins : b.seg_off + s.pl.NB; }
// entries the sort placed (a device word)
static const uint32_t* msm_entries_word(const MsmShape& s, const MsmBuffers& b) { return s.flat ? b.flat_off + s.flat_bins : b.bucket_off + s.pl.NB; }

// ---------------------------------------------------------------------------------------------- msm.hip
// The kernels that may ask for more than 64 KB of dynamic LDS, by their entry in allow_big_lds' process-wide cache.
enum MsmLdsSlot {
    LDS_HIST = 0,
    LDS_SCATTER = 1,
    LDS_REDUCE_XYZZ = 2,
    LDS_PARTITION = 3,
    LDS_BIN_SORT = 4,
    LDS_FLAT_PARTITION_8 = 5,
    LDS_FLAT_BIN_SORT = 6,
    LDS_REDUCE_TE29 = 7,
    LDS_REDUCE_QUAD_256 = 8,
    LDS_REDUCE_QUAD_128 = 9,
    LDS_FLAT_PARTITION_16 = 10,
    LDS_SLOTS = 12
};
int allow_big_lds(swm_ctx* ctx, MsmLdsSlot slot, const void* fn, size_t bytes);

// ---------------------------------------------------------------------------------------------- msm_sort.hip
WinLayout msm_plan(size_t n);
// The stages from scalars to ordered segments; each enqueues on the context's stream.
int msm_digits_stage(swm_ctx* ctx, const MsmShape& s, const MsmBuffers& b, const void* d_scalars, size_t n, int mont,
                     const MsmInfMask& inf, const MsmTable& tab);
int msm_sort_flat(swm_ctx* ctx, const MsmShape& s, const MsmBuffers& b, const MsmTable& tab, size_t n, MsmTwinSrc* lead);
int msm_sort_windows(swm_ctx* ctx, const MsmShape& s, const MsmBuffers& b, size_t n);
int msm_seg_order_stage(swm_ctx* ctx, const MsmShape& s, const MsmBuffers& b);
int msm_twin_copy_launch(swm_ctx* ctx, const TwinCopy& tc);  // the launch of the driver's msm_twin_copy_stage

// ---------------------------------------------------------------------------------------------- msm_table.hip
// msm_te_convert on caller-chosen points, for the point-layer self-test (its ops P28T_ROWS, and P28T_ROWS29 with limb29)
int msm_te_convert_run(swm_ctx* ctx, bool limb29, const G1Affine* in, size_t n, Fq* pref, G1TE* out, uint32_t* bad);

// ---------------------------------------------------------------------------------------------- msm_stages.hip
// The launches of the driver's msm_accumulate_stage: msm_accumulate[_te, _te_quad], then msm_big_bucket_sum.
int msm_accumulate_launch(swm_ctx* ctx, const MsmShape& s, const MsmBuffers& b, const MsmTable& tab, const G1Affine* d_bases,
                          const G1Affine* d_bases28);
// The bucket-stage kernel of a launch; the values index swm_ctx::stat_msm_tails (quad | low-LDS | wide / thin | XYZZ).
enum MsmTailKernel { TAIL_QUAD = 0, TAIL_LOW = 1, TAIL_TE29 = 2, TAIL_XYZZ = 3 };
// One bucket-stage launch for the k jobs of `batch` on the context's stream.  rb: chains per workgroup of a TAIL_QUAD launch (256 or
// 128); max_red, max_win: the most workgroups per window and windows of any job.
int msm_tail_launch(swm_ctx* ctx, const TailBatch& batch, int k, MsmTailKernel kernel, unsigned rb, unsigned max_red, unsigned max_win);

}  // namespace swm

// msm_sort.hip — the G1 MSM from scalars to ordered segments (stages 1 - 3 of msm.hip's list): the window layouts, the signed-digit
// recoding, the counting sorts of the two schedules (per-window: one level, two for large MSMs; flat: coarse bins, then one
// workgroup per bin), the copy a twin pair's follower takes instead, the scans, and the segment descriptors and their order by
// length.  The driver (msm.hip) decides the geometry (MsmShape) and owns the buffers, streams and events; the stage functions at
// the end of this file launch on the context's stream.
#include <string.h>
#include <algorithm>
#include "context.h"
#include "g1.cuh"
#include "msm_stages.h"

namespace swm {

// ---------------------------------------------------------------------------------------------- parameters
static constexpr uint32_t SORT_TILE_MIN = 65536;  // digits per workgroup in the LDS-privatised counting sort (at least)
static constexpr int SORT_THREADS = 1024;

unsigned msm_table_windows(unsigned c) { return (254 + c - 1) / c; }
// The 254 recoding bits in ceil(254 / c) windows whose widths differ by at most one, the widest c bits (c[0] is always the
// widest): a short top window would put a quarter of all points into two buckets.  Bucket counts and offsets are the caller's.
static WinLayout msm_windows(unsigned c) {
    WinLayout L;
    memset(&L, 0, sizeof(L));
    L.nwin = msm_table_windows(c);
    const unsigned base = 254 / L.nwin, extra = 254 % L.nwin;
    for (unsigned w = 0, bit = 0; w < L.nwin; bit += L.c[w++]) {
        L.c[w] = (uint8_t)(base + (w < extra ? 1 : 0));
        L.bit[w] = (uint16_t)bit;
    }
    L.maxB = 1u << (L.c[0] - 1);
    return L;
}
WinLayout msm_plan(size_t n) {
    // Target window size for the GPU schedule (NOT arkworks' ln-based rule): large enough that the n*W accumulate
    // adds dominate the fixed-latency bucket reduction, small enough that buckets stay populated.
    // measured on MI355X (sweep over c = 8..16, r01): 2^10 -> 10, 2^12..2^16 -> 12, 2^18 -> 14, >= 2^19 -> 16.
    // c is capped at 16 by the LDS histogram of the counting sort (2^(c-1) words).
    unsigned c;
    if (n <= (1u << 11)) c = 10;
    else if (n <= 98304) c = 12;
    else if (n <= 393216) c = 14;
    else c = 16;
    WinLayout L = msm_windows(c);
    for (unsigned w = 0; w < L.nwin; w++) {  // window w: 2^(c[w]-1) buckets of its own
        L.boff[w] = L.NB;
        L.NB += 1u << (L.c[w] - 1);
    }
    L.boff[L.nwin] = L.NB;
    return L;
}
// Windows of the flat schedule for a table of width c: all of them index ONE set of 2^(c-1) buckets.
WinLayout msm_table_layout(unsigned c) {
    WinLayout L = msm_windows(c);
    L.NB = L.maxB;
    L.boff[L.nwin] = L.NB;
    return L;
}
unsigned msm_table_width(size_t n_bases) {
    if (const unsigned forced = (unsigned)sw(SW_MSM_TABLE_C)) return forced;  // one width for every base set of the process
    if (n_bases < 512) return 0;  // tiny base sets keep the per-window schedule
    // measured r02 (prove() at 2^10 .. 2^20 constraints, base sets of 3 x that): two bits above the size of the base
    // set up to 2^15 points — 4 .. 10 points per bucket for the MSMs of a proof, which keeps the accumulation chains
    // short — one bit above it from there, up to 20 (21 and 22 lose at 2^20 and above: the bucket stage grows faster
    // than the accumulation shrinks)
    unsigned lg = 0;
    while (((size_t)2 << lg) <= n_bases) lg++;
    return lg <= 14 ? lg + 2 : std::min(20u, lg + 1);  // (lg = 15, the key of a 2^14-constraint circuit: 17 until r04; 16: 4.73 instead of 4.98 ms per proof)
}

// ---------------------------------------------------------------------------------------------- digits
// Signed-digit recoding of a 253-bit standard-form scalar; calls f(window, bucket_index, negative) for every
// non-zero digit.  Digit d in [-2^(c-1), 2^(c-1)]; bucket index |d| - 1.
// (r06: the scalar is consumed as a shift register — the window's bits are the low bits of word 0, then the eight words move down by
// the window's width with funnel shifts — instead of being indexed by the window's bit position: the dynamic index made the compiler
// keep the scalar in LDS (promoted alloca), and msm_digits spent 76 % of its wave-cycles waiting, 81 % of its LDS cycles in bank
// conflicts.  The windows are consecutive from bit 0 (msm_plan, msm_table_layout), 2 <= c <= 22.)
template <class Fn>
__device__ __forceinline__ void for_each_digit(const Fr& s, const WinLayout& L, Fn f) {
    uint32_t carry = 0;
    uint32_t r[8];
#pragma unroll
    for (int i = 0; i < 8; i++) r[i] = s.v[i];
    for (unsigned w = 0; w < L.nwin; w++) {
        const unsigned c = L.c[w];
        const uint32_t mask = (1u << c) - 1, half = 1u << (c - 1);
        const uint32_t v = r[0];
#pragma unroll
        for (int i = 0; i < 7; i++) r[i] = __funnelshift_r(r[i], r[i + 1], c);
        r[7] >>= c;
        uint32_t d = (v & mask) + carry;
        uint32_t code = 0;  // 0 = zero digit, else ((bucket << 1) | negative) + 1
        if (d > half) {
            carry = 1;
            if (d != (1u << c)) code = ((((1u << c) - d - 1) << 1) | 1u) + 1;  // digit d - 2^c < 0
        } else {
            carry = 0;
            if (d != 0) code = ((d - 1) << 1) + 1;
        }
        f(w, code);
    }
}

// digits[w * n + i] = code of window w of scalar i (coalesced over i).            HBM: 32 B read + 4 W B written / point
// A scalar that is not a canonical field element (>= r; arkworks' BigInteger256 scalars always are) raises *bad: the
// recoding only covers 254 bits, so such an input cannot be given a meaning.  Points flagged in the infinity mask get
// zero digits (they contribute nothing, as in VariableBaseMSM).  bad[1] counts the points that contribute nothing.
__global__ void __launch_bounds__(256) msm_digits(const Fr* __restrict__ scalars, size_t n, int mont, WinLayout L,
                                                  uint32_t* __restrict__ digits, const uint32_t* __restrict__ inf_mask,
                                                  size_t inf_first, uint32_t* __restrict__ bad, DigitShard sh, unsigned sblk_log,
                                                  size_t sbstride) {
    SWM_LIGHT_KERNEL();
    // scalar i sits at scalars[(i >> sblk_log) * sbstride + (i & (2^sblk_log - 1))]: contiguous by default (sblk_log = 31), the
    // blocks a rank of a sharded proof takes of a polynomial every rank holds otherwise (MsmTable::scalar_stride, blk_log, bstride)
    const size_t smask = ((size_t)1 << sblk_log) - 1;
    // (r06: two scalars per lane and trip, both loads issued before the first is recoded — 64.5 instead of 60.3 us per 2^20 points on
    // the box that measured it: not kept)
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        Fr s = scalars[(i >> sblk_log) * sbstride + (i & smask)];
        bool ge = true;  // s >= r ?
#pragma unroll
        for (int k = 7; k >= 0; k--) {
            if (s.v[k] != FrParams::P[k]) {
                ge = s.v[k] > FrParams::P[k];
                break;
            }
        }
        if (ge) atomicOr(bad, 1u);
        if (mont) s = fp_to_std(s);
        bool skip = false;
        if (inf_mask) {
            size_t b = inf_first + i;
            skip = (inf_mask[b >> 5] >> (b & 31)) & 1u;
        }
        {   // points that contribute nothing (zero scalar, or an identity base): counted per wave, one atomic per wave —
            // the measurement prices them at their 32-B scalar only (bench.py: roofline numerator)
            uint32_t z = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) z |= s.v[k];
            const unsigned long long m = __ballot(z == 0 || skip);
            if (m && (threadIdx.x & 63) == (unsigned)__ffsll((long long)m) - 1) atomicAdd(bad + 1, (uint32_t)__popcll(m));
        }
        for_each_digit(s, L, [&](unsigned w, uint32_t code) {
            if (sh.on && code) {
                const uint32_t bucket = (code - 1) >> 1;
                const bool keep = L.c[w] == sh.cfull ? (bucket >= sh.blo && bucket < sh.bhi) : (i >= sh.plo && i < sh.phi);
                if (!keep) code = 0;
            }
            digits[(size_t)w * n + i] = skip ? 0u : code;
        });
    }
}

// Counting sort, pass 1: per-(tile, window) histogram in LDS, one global atomic per non-empty LDS bin.
__global__ void __launch_bounds__(SORT_THREADS) msm_hist(const uint32_t* __restrict__ digits, size_t n, WinLayout L,
                                                         uint32_t SORT_TILE, uint32_t* __restrict__ hist) {
    extern __shared__ uint32_t lh[];
    const uint32_t w = blockIdx.y;
    const uint32_t B = 1u << (L.c[w] - 1), boff = L.boff[w];
    const size_t lo = (size_t)blockIdx.x * SORT_TILE, hi = min(lo + (size_t)SORT_TILE, n);
    for (uint32_t b = threadIdx.x; b < B; b += SORT_THREADS) lh[b] = 0;
    __syncthreads();
    const uint32_t* d = digits + (size_t)w * n;
    // four independent loads in flight per lane: the loop is bound by load latency, not by bandwidth
    for (size_t i = lo + threadIdx.x; i < hi; i += 4 * SORT_THREADS) {
        uint32_t c[4];
#pragma unroll
        for (int u = 0; u < 4; u++) c[u] = i + u * SORT_THREADS < hi ? d[i + u * SORT_THREADS] : 0u;
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (c[u]) atomicAdd(&lh[(c[u] - 1) >> 1], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < B; b += SORT_THREADS) {
        uint32_t v = lh[b];
        if (v) atomicAdd(&hist[boff + b], v);
    }
}

// Counting sort, pass 2: the tile reserves a contiguous run in every bucket it touches (one returning global
// atomic per non-empty bin), then ranks its digits with LDS atomics and writes (point index | sign).
__global__ void __launch_bounds__(SORT_THREADS) msm_scatter(const uint32_t* __restrict__ digits, size_t n, WinLayout L,
                                                            uint32_t SORT_TILE, const uint32_t* __restrict__ bucket_off,
                                                            uint32_t* __restrict__ cursor,
                                                            uint32_t* __restrict__ sorted,
                                                            const uint32_t* __restrict__ two_level_bad /* null: always run */) {
    extern __shared__ uint32_t lh[];
    const uint32_t w = blockIdx.y;
    if (two_level_bad && two_level_bad[w] == 0) return;  // the two-level scatter below handles this window
    const uint32_t B = 1u << (L.c[w] - 1), boff = L.boff[w];
    const size_t lo = (size_t)blockIdx.x * SORT_TILE, hi = min(lo + (size_t)SORT_TILE, n);
    for (uint32_t b = threadIdx.x; b < B; b += SORT_THREADS) lh[b] = 0;
    __syncthreads();
    const uint32_t* d = digits + (size_t)w * n;
    for (size_t i = lo + threadIdx.x; i < hi; i += 4 * SORT_THREADS) {
        uint32_t c[4];
#pragma unroll
        for (int u = 0; u < 4; u++) c[u] = i + u * SORT_THREADS < hi ? d[i + u * SORT_THREADS] : 0u;
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (c[u]) atomicAdd(&lh[(c[u] - 1) >> 1], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < B; b += 4 * SORT_THREADS) {  // four returning global atomics in flight per lane
        uint32_t v[4], r[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = b + u * SORT_THREADS < B ? lh[b + u * SORT_THREADS] : 0u;
#pragma unroll
        for (int u = 0; u < 4; u++) r[u] = v[u] ? atomicAdd(&cursor[boff + b + u * SORT_THREADS], v[u]) : 0u;
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (v[u]) lh[b + u * SORT_THREADS] = bucket_off[boff + b + u * SORT_THREADS] + r[u];
    }
    __syncthreads();
    for (size_t i = lo + threadIdx.x; i < hi; i += 4 * SORT_THREADS) {
        uint32_t c[4];
#pragma unroll
        for (int u = 0; u < 4; u++) c[u] = i + u * SORT_THREADS < hi ? d[i + u * SORT_THREADS] : 0u;
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (c[u]) {
                uint32_t pos = atomicAdd(&lh[(c[u] - 1) >> 1], 1u);
                sorted[pos] = (uint32_t)(i + u * SORT_THREADS) | (((c[u] - 1) & 1u) << 31);
            }
    }
}

// ---- two-level scatter for large MSMs
// The one-level scatter above writes every entry to its final position with a 4-byte store; at ~2 entries per
// (tile, bucket) those stores are scattered over the whole array and the kernel is bound by write sectors (73 G
// digits/s whatever the tile size).  Two levels keep every store in a run:
//   msm_partition : a workgroup groups the (entry, bucket) pairs of an 8192-digit tile by COARSE bin (bucket >> fb[w])
//                   in LDS, reserves one run per (tile, bin) with a global atomic and copies the tile out run by run
//                   (~32 pairs = 256 B each);
//   msm_bin_sort  : one workgroup per bin (<= BIN_CAP entries: the region of `sorted` between the offsets of its
//                   first and last bucket) places the entries by fine bucket in LDS — the per-bucket offsets are
//                   already known from the prefix sums — and copies the region out in order.
// Bins are sized per window (BinPlan): the top window only sees digits up to r >> bit, i.e. much denser buckets.
// A bin larger than BIN_CAP (skewed digits: many equal scalars) marks its WINDOW bad and that window takes the
// one-level path: both sets of kernels are launched and the unused one returns at once — no host read-back.
static constexpr uint32_t BIN_CAP = 24576;   // entries per bin (96 KB of LDS in msm_bin_sort)
static constexpr int BIN_THREADS = 1024;
static constexpr uint32_t PART_TILE = 8192;  // digits per workgroup in msm_partition (64 KB of LDS for the pairs)
__global__ void __launch_bounds__(256) msm_bin_check(const uint32_t* __restrict__ bucket_off, WinLayout L, BinPlan P,
                                                     uint32_t* __restrict__ bad) {
    const uint32_t w = blockIdx.y, bin = blockIdx.x * blockDim.x + threadIdx.x;
    if (bin >= P.nbins[w]) return;
    const uint32_t B = 1u << (L.c[w] - 1), fb = P.fb[w], first = bin << fb, last = min(first + (1u << fb), B);
    uint32_t size = bucket_off[L.boff[w] + last] - bucket_off[L.boff[w] + first];
    if (bin + 1 == P.nbins[w]) size = bucket_off[L.boff[w] + B] - bucket_off[L.boff[w] + first];  // nothing may lie beyond
    if (size > BIN_CAP || (bin + 1 == P.nbins[w] && last < B && bucket_off[L.boff[w] + B] != bucket_off[L.boff[w] + last]))
        bad[w] = 1u;
}
__global__ void __launch_bounds__(1024) msm_partition(const uint32_t* __restrict__ digits, size_t n, WinLayout L, BinPlan P,
                                                      const uint32_t* __restrict__ bucket_off,
                                                      uint32_t* __restrict__ bin_cursor, const uint32_t* __restrict__ bad,
                                                      uint2* __restrict__ tmp) {
    __shared__ uint32_t cnt[PART_MAX_BINS], start[PART_MAX_BINS], gpos[PART_MAX_BINS];
    extern __shared__ uint2 stage[];  // PART_TILE pairs
    const uint32_t w = blockIdx.y;
    if (bad[w]) return;
    const uint32_t nb = P.nbins[w], fb = P.fb[w], boff = L.boff[w], t = threadIdx.x;
    const size_t lo = (size_t)blockIdx.x * PART_TILE;
    for (uint32_t b = t; b < nb; b += 1024) cnt[b] = 0;
    __syncthreads();
    const uint32_t* d = digits + (size_t)w * n;
    uint32_t c[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
        size_t i = lo + t + (size_t)u * 1024;
        c[u] = i < n ? d[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < 8; u++)
        if (c[u]) atomicAdd(&cnt[((c[u] - 1) >> 1) >> fb], 1u);
    __syncthreads();
    // exclusive scan of cnt over the (<= 1024) bins: one bin per lane, Hillis-Steele in `start`
    uint32_t mine = t < nb ? cnt[t] : 0u;
    start[t] = mine;
    __syncthreads();
    for (uint32_t dd = 1; dd < 1024; dd <<= 1) {
        uint32_t v = t >= dd ? start[t - dd] : 0u;
        __syncthreads();
        start[t] += v;
        __syncthreads();
    }
    const uint32_t excl = start[t] - mine;
    __syncthreads();
    start[t] = excl;
    if (t < nb) {
        cnt[t] = excl;  // running cursor of the bin inside the staged tile
        gpos[t] = mine ? bucket_off[boff + (t << fb)] + atomicAdd(&bin_cursor[w * PART_MAX_BINS + t], mine) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; u++)
        if (c[u]) {
            const uint32_t bucket = (c[u] - 1) >> 1;
            const uint32_t p = atomicAdd(&cnt[bucket >> fb], 1u);
            stage[p] = make_uint2((uint32_t)(lo + t + (size_t)u * 1024) | (((c[u] - 1) & 1u) << 31), bucket);
        }
    __syncthreads();
    const uint32_t total = start[nb - 1] + (cnt[nb - 1] - start[nb - 1]);  // pairs staged by this tile
    for (uint32_t i = t; i < total; i += 1024) {
        uint2 e = stage[i];
        uint32_t b = e.y >> fb;
        tmp[gpos[b] + (i - start[b])] = e;
    }
}
__global__ void __launch_bounds__(BIN_THREADS) msm_bin_sort(const uint2* __restrict__ tmp, WinLayout L, BinPlan P,
                                                            const uint32_t* __restrict__ bucket_off,
                                                            const uint32_t* __restrict__ bad, uint32_t* __restrict__ sorted) {
    extern __shared__ uint32_t stage32[];  // BIN_CAP entries
    __shared__ uint32_t fc[128];
    const uint32_t w = blockIdx.y, bin = blockIdx.x;
    if (bad[w] || bin >= P.nbins[w]) return;
    const uint32_t B = 1u << (L.c[w] - 1), fb = P.fb[w], first = bin << fb, nf = min(1u << fb, B - first);
    const uint32_t* off = bucket_off + L.boff[w] + first;
    const uint32_t lo = off[0], cnt = off[nf] - lo;
    for (uint32_t f = threadIdx.x; f < nf; f += BIN_THREADS) fc[f] = off[f] - lo;
    __syncthreads();
    const uint32_t fmask = (1u << fb) - 1;
    for (uint32_t i = threadIdx.x; i < cnt; i += 4 * BIN_THREADS) {
        uint2 e[4];
#pragma unroll
        for (int u = 0; u < 4; u++) e[u] = i + u * BIN_THREADS < cnt ? tmp[lo + i + u * BIN_THREADS] : make_uint2(0u, 0u);
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (i + u * BIN_THREADS < cnt) stage32[atomicAdd(&fc[e[u].y & fmask], 1u)] = e[u].x;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cnt; i += BIN_THREADS) sorted[lo + i] = stage32[i];
}


// ---------------------------------------------------------------------------------------------- precomputed-window ("flat") schedule
// For a RESIDENT base set the multiples 2^(bit_w) P_i of every point are precomputed once (msm_table_build: W copies
// of the set, 96 B x n x W in HBM — what 288 GB are for).  A digit of window w then selects table row w instead of a
// bucket set of its own: ALL windows share ONE set of 2^(c-1) buckets, so
//   * the window width is no longer capped by "buckets per window x windows" (the bucket stage runs once): c = 20 gives
//     13 windows instead of 16, i.e. 19 % fewer mixed additions in msm_accumulate for the same result;
//   * there is no Horner chain over the windows at the end (the shifts are in the table).
// The counting sort over 2^19 buckets cannot histogram in LDS in one go; it is two-level from the start:
//   msm_flat_coarse_hist / msm_flat_scan_bins  entries per COARSE bin (bucket >> fb, <= 4096 bins) — LDS histogram per tile,
//   msm_flat_partition                         entries grouped by bin in LDS and written out in runs (as msm_partition),
//   msm_flat_bin_sort                          one workgroup per bin: fine counts (they ARE the bucket histogram the
//                                              scans below consume), placement in LDS, coalesced copy-out; a bin that
//                                              does not fit LDS (structured scalars) is placed directly in HBM.
static constexpr uint32_t FLAT_BIN_CAP = 32768;  // entries a bin may hold to be placed in LDS (128 KB)
// grid (tiles over the points, windows): counts per (window, coarse bin), bin_count[w * nbins + b] (window-major: a workgroup's
// atomics land on consecutive words; bin-major lines made this kernel 23 instead of 11 us) — the partition places a
// bin's entries WINDOW BY WINDOW (see msm_flat_scan_bins), for which it needs the bin's count of every window
__global__ void __launch_bounds__(SORT_THREADS) msm_flat_coarse_hist(const uint32_t* __restrict__ digits, size_t n, unsigned fb,
                                                                     uint32_t nbins, uint32_t tile, uint32_t* __restrict__ bin_count) {
    SWM_LIGHT_KERNEL();
    __shared__ uint32_t lh[FLAT_MAX_BINS];
    for (uint32_t b = threadIdx.x; b < nbins; b += SORT_THREADS) lh[b] = 0;
    __syncthreads();
    const uint32_t w = blockIdx.y;
    const uint32_t* d = digits + (size_t)w * n;
    const size_t lo = (size_t)blockIdx.x * tile, hi = min(lo + (size_t)tile, n);
    for (size_t i = lo + threadIdx.x; i < hi; i += 4 * SORT_THREADS) {
        uint32_t c[4];
#pragma unroll
        for (int u = 0; u < 4; u++) c[u] = i + u * SORT_THREADS < hi ? d[i + u * SORT_THREADS] : 0u;
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (c[u]) atomicAdd(&lh[((c[u] - 1) >> 1) >> fb], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nbins; b += SORT_THREADS) {
        uint32_t v = lh[b];
        if (v) atomicAdd(&bin_count[(size_t)w * nbins + b], v);
    }
}
// Exclusive scan of <= 4096 bin totals (summed over the windows) by one workgroup: bin_off[0 .. nbins]; the offsets of every
// (bin, window) inside that, win_off[b * FLAT_CUR_STRIDE + w] — a bin's entries are laid out WINDOW BY WINDOW, so that a bucket's entries
// reach the accumulation window by window too: all lanes of the chip then gather from the table rows of the same one or two
// windows at a time (1 / 13 of a multi-GB table: TLB reach and Infinity Cache, r04 — DESIGN.md §3.1) instead of from all of it;
// and the bins' SEGMENT capacities 2^fb + count / SEG (an upper bound of sum over the bin's buckets of ceil(count_b / SEG)):
// bin_seg_off[0 .. nbins] — the segment indices a bin's workgroup of msm_flat_bin_sort hands out without knowing what the
// other bins need.
// BPT bins per lane: 1 up to 1024 bins (one lane per bin: its 2 x 32 loads are all the latency there is), 4 above
template <int BPT>
__global__ void __launch_bounds__(1024) msm_flat_scan_bins(const uint32_t* __restrict__ bin_count, uint32_t nbins, uint32_t nwin,
                                                           uint32_t* __restrict__ bin_off, uint32_t* __restrict__ win_off, unsigned fb,
                                                           uint32_t SEG, uint32_t* __restrict__ bin_seg_off) {
    SWM_LIGHT_KERNEL();
    __shared__ uint32_t sm[1024], sg[1024];
    const uint32_t t = threadIdx.x;
    uint32_t v[BPT], g[BPT], s = 0, q = 0;
    // a bin's counts of all windows.  No branches: every load is unconditional, from a clamped (window, bin), and masked afterwards;
    // the offsets leave as whole 128-byte lines.  (r04's first form looped over the windows with a load per trip, each waiting for
    // the one before; its second predicated every load and store: 392 branches and 35 us in a kernel every MSM waits for.)
#pragma unroll
    for (int u = 0; u < BPT; u++) {
        const bool in = BPT * t + u < nbins;
        const uint32_t bc = min(BPT * t + u, nbins - 1);
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < FLAT_CUR_STRIDE; w++) {
            const uint32_t x = bin_count[(size_t)min(w, nwin - 1) * nbins + bc];
            sum += w < nwin ? x : 0u;
        }
        v[u] = in ? sum : 0u;
        g[u] = in ? (1u << fb) + v[u] / SEG : 0u;
        s += v[u];
        q += g[u];
    }
    sm[t] = s;
    sg[t] = q;
    __syncthreads();
    const uint32_t T = blockDim.x;  // a power of two >= nbins / BPT (a single wave for the few bins of a small MSM)
    for (uint32_t d = 1; d < T; d <<= 1) {
        uint32_t x = t >= d ? sm[t - d] : 0u, y = t >= d ? sg[t - d] : 0u;
        __syncthreads();
        sm[t] += x;
        sg[t] += y;
        __syncthreads();
    }
    uint32_t run = sm[t] - s, rung = sg[t] - q;
#pragma unroll
    for (int u = 0; u < BPT; u++) {
        const uint32_t b = BPT * t + u;
        if (b < nbins) {
            bin_off[b] = run;
            bin_seg_off[b] = rung;
            uint4* o = reinterpret_cast<uint4*>(win_off + (size_t)b * FLAT_CUR_STRIDE);
            uint32_t at = run;
#pragma unroll
            for (uint32_t k = 0; k < FLAT_CUR_STRIDE / 4; k++) {  // exclusive prefix over the windows (the words beyond nwin: unused)
                uint4 c;
                c.x = bin_count[(size_t)min(4 * k + 0, nwin - 1) * nbins + b];
                c.y = bin_count[(size_t)min(4 * k + 1, nwin - 1) * nbins + b];
                c.z = bin_count[(size_t)min(4 * k + 2, nwin - 1) * nbins + b];
                c.w = bin_count[(size_t)min(4 * k + 3, nwin - 1) * nbins + b];
                uint4 w4;
                w4.x = at;
                w4.y = w4.x + c.x;
                w4.z = w4.y + c.y;
                w4.w = w4.z + c.z;
                at = w4.w + c.w;
                o[k] = w4;
            }
        }
        run += v[u];
        rung += g[u];
    }
    if (t == T - 1) {
        bin_off[nbins] = sm[T - 1];
        bin_seg_off[nbins] = sg[T - 1];
    }
}
// (entry, bucket) pairs grouped by coarse bin; grid (tiles over the points, windows).  entry = table row of the point:
// w * tstride + toff + i, with the sign of the digit in bit 31.
template <int FLAT_PART_U>
__global__ void __launch_bounds__(1024) msm_flat_partition(const uint32_t* __restrict__ digits, size_t n, uint32_t tstride,
                                                           uint32_t toff, unsigned blk_log, uint32_t bstride, unsigned fb, uint32_t nbins,
                                                           const uint32_t* __restrict__ win_off, uint32_t nwin,
                                                           uint32_t* __restrict__ bin_cursor, uint2* __restrict__ tmp) {
    SWM_LIGHT_KERNEL();
    // LDS: PART_TILE pairs | cnt, start, gpos (nbins words each, rounded up to a multiple of 4) | 1024 scan words: sized by
    // the bin count of the call (74 KB at 512 bins: two workgroups per CU; the fixed 4096-bin arrays allowed one)
    constexpr uint32_t FLAT_PART_TILE = FLAT_PART_U * 1024u;
    extern __shared__ uint2 stage[];  // FLAT_PART_TILE pairs
    const uint32_t nb4 = (nbins + 3) & ~3u;
    uint32_t* cnt = reinterpret_cast<uint32_t*>(stage + FLAT_PART_TILE);
    uint32_t* start = cnt + nb4;
    uint32_t* gpos = start + nb4;
    uint32_t* scan = gpos + nb4;
    const uint32_t w = blockIdx.y, t = threadIdx.x;
    const size_t lo = (size_t)blockIdx.x * FLAT_PART_TILE;
    for (uint32_t b = t; b < nbins; b += 1024) cnt[b] = 0;
    __syncthreads();
    const uint32_t* d = digits + (size_t)w * n;
    uint32_t c[FLAT_PART_U];
#pragma unroll
    for (int u = 0; u < FLAT_PART_U; u++) {
        size_t i = lo + t + (size_t)u * 1024;
        c[u] = i < n ? d[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < FLAT_PART_U; u++)
        if (c[u]) atomicAdd(&cnt[((c[u] - 1) >> 1) >> fb], 1u);
    __syncthreads();
    // exclusive scan of cnt over <= 4096 bins: four bins per lane
    uint32_t v[4], sum = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        v[u] = 4 * t + u < nbins ? cnt[4 * t + u] : 0u;
        sum += v[u];
    }
    // inclusive scan over the 1024 lanes: shuffles inside a wave, the 16 wave totals through LDS (two barriers instead of
    // the twenty of a Hillis-Steele scan in LDS)
    uint32_t inc = sum;
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) {
        uint32_t x = __shfl_up(inc, dd, 64);
        if ((t & 63) >= (uint32_t)dd) inc += x;
    }
    if ((t & 63) == 63) scan[t >> 6] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t wv = 0; wv < 16; wv++) {
        const uint32_t x = scan[wv];
        if (wv < (t >> 6)) before += x;
        total += x;
    }
    uint32_t run = before + inc - sum;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint32_t b = 4 * t + u;
        if (b < nbins) {
            start[b] = run;
            cnt[b] = run;  // running cursor of the bin inside the staged tile
            // the run of this (tile, bin) inside the bin's range of window w; the cursors of a bin's windows share one line
            gpos[b] = v[u] ? win_off[(size_t)b * FLAT_CUR_STRIDE + w] + atomicAdd(&bin_cursor[(size_t)b * FLAT_CUR_STRIDE + w], v[u]) : 0u;
        }
        run += v[u];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < FLAT_PART_U; u++)
        if (c[u]) {
            const uint32_t bucket = (c[u] - 1) >> 1;
            const uint32_t p = atomicAdd(&cnt[bucket >> fb], 1u);
            const uint32_t i = (uint32_t)(lo + t + (size_t)u * 1024);  // scalar i -> its base (MsmTable: blocks of a sharded layout)
            const uint32_t row = w * tstride + toff + (i >> blk_log) * bstride + (i & ((1u << blk_log) - 1u));
            stage[p] = make_uint2(row | (((c[u] - 1) & 1u) << 31), bucket);
        }
    __syncthreads();
    for (uint32_t i = t; i < total; i += 1024) {
        uint2 e = stage[i];
        uint32_t b = e.y >> fb;
        tmp[gpos[b] + (i - start[b])] = e;
    }
}
// One workgroup per bin: bucket histogram of the bin, placement by bucket — and everything the accumulation and the bucket
// stage need to know about the bin's buckets (r04; four launches — three scans over the histogram and a binary search per
// segment — did this before): a bin is a contiguous bucket range whose first entry (bin_off) and first segment index
// (bin_seg_off, a capacity: see msm_flat_scan_bins) are known, so with the bin's fine counts in LDS the workgroup writes
//   hist[b], bucket_off[b], seg_off[b]           count, first entry and first segment of bucket b
//   seg_start[s], seg_len[s]                     the balanced segments (<= SEG entries) of its buckets; the unused tail of the
//                                                bin's segment indices gets length 0 (msm_seg_order skips those)
//   len_hist                                     segments per length (for the ordering by length that follows)
//   big_list                                     buckets with more than big_nseg segments (folded ahead of the bucket stage)
struct FlatSegOut {
    uint32_t *hist, *bucket_off, *seg_off, *seg_start, *seg_len, *len_hist, *big_count, *big_list;
    uint32_t SEG, big_nseg;
    // the ns segments of a bucket with more than SEG entries take its entries ROUND-ROBIN (segment k: entries k, k + ns, ...;
    // seg_len = length | ns << 8) instead of as consecutive ranges: a bucket's entries lie window by window, and every lane
    // should walk the windows in the same order (the locality of the accumulation's gathers).  TE jobs only.
    uint32_t interleave;
};
#ifndef SWM_PLACE_U
#define SWM_PLACE_U 4
#endif
static constexpr int PLACE_U = SWM_PLACE_U;
// segment k of the ns balanced segments of a bucket with c entries starting at `ent` (segment indices from s0); lh: the
// workgroup's length histogram in LDS.  Interleaved segments pack their stride into seg_len (length | ns << 8): ns < 2^24,
// otherwise (only reachable with a one-entry segment bound on a degenerate input) the bucket keeps consecutive ranges.
static constexpr uint32_t FLAT_WIDE_NS = 16, FLAT_WIDE_Q = 32;  // segments above which a bucket is written by the workgroup; queue length
__device__ __forceinline__ void flat_seg_write(const FlatSegOut& o, uint32_t c, uint32_t ns, uint32_t ent, uint32_t s0, uint32_t k,
                                               uint32_t* lh) {
    if (o.interleave && ns > 1 && ns < (1u << 24)) {
        const uint32_t len = (c - k + ns - 1) / ns;
        o.seg_start[s0 + k] = ent + k;
        o.seg_len[s0 + k] = len | (ns << 8);
        atomicAdd(&lh[o.SEG - len], 1u);
    } else {
        const uint32_t ks = (uint32_t)(((uint64_t)c * k) / ns), ke = (uint32_t)(((uint64_t)c * (k + 1)) / ns);
        o.seg_start[s0 + k] = ent + ks;
        o.seg_len[s0 + k] = ke - ks;
        atomicAdd(&lh[o.SEG - (ke - ks)], 1u);
    }
}
// A twin's second sorted array (MsmTwin): the same entries with the rows of the follower's table — an entry's window is
// row / tstride (the rows of a window are tstride apart and offset + i < tstride), its row there row + w * dstride + doff
// (mod 2^31: the sign of the digit stays in bit 31).
struct TwinOut {
    uint32_t* sorted2;  // null: no follower
    uint32_t tstride, dstride, doff;
    __device__ __forceinline__ uint32_t map(uint32_t e) const {
        const uint32_t row = e & 0x7fffffffu, w = row / tstride;
        return (e & 0x80000000u) | ((row + w * dstride + doff) & 0x7fffffffu);
    }
};
template <int BT>
__global__ void __launch_bounds__(BT) msm_flat_bin_sort(const uint2* __restrict__ tmp, unsigned fb, uint32_t NB,
                                                                 const uint32_t* __restrict__ bin_off,
                                                                 const uint32_t* __restrict__ bin_seg_off, FlatSegOut o,
                                                                 uint32_t* __restrict__ sorted, TwinOut tw) {
    SWM_LIGHT_KERNEL();
    extern __shared__ uint32_t stage32[];  // fc[nf] | fo[nf] | FLAT_BIN_CAP entries
    __shared__ uint32_t wsum[2][BT / 64];
    __shared__ uint32_t lh[SEG_MAX + 1];
    __shared__ uint32_t wide[FLAT_WIDE_Q][3], nwide;  // buckets whose descriptors the whole workgroup writes: (count, first entry, first segment)
    uint32_t* fc = stage32;
    uint32_t* fo = fc + (1u << fb);
    uint32_t* stage = fo + (1u << fb);
    const uint32_t bin = blockIdx.x, nf = 1u << fb, first = bin << fb, fmask = nf - 1, t = threadIdx.x;
    const uint32_t lo = bin_off[bin], cnt = bin_off[bin + 1] - lo;
    const uint32_t seg_lo = bin_seg_off[bin], seg_hi = bin_seg_off[bin + 1];
    for (uint32_t f = t; f < nf; f += BT) fc[f] = 0;
    for (uint32_t i = t; i <= o.SEG; i += BT) lh[i] = 0;
    if (t == 0) nwide = 0;
    __syncthreads();
    for (uint32_t i = t; i < cnt; i += BT) atomicAdd(&fc[tmp[lo + i].y & fmask], 1u);
    __syncthreads();
    // exclusive prefixes of the fine counts and of the segments per bucket (nf <= 2048): a chunk per lane, shuffles inside
    // a wave, the 16 wave totals through LDS
    const uint32_t per = (nf + BT - 1) / BT, f0 = t * per, f1 = min(f0 + per, nf);
    uint32_t sum = 0, sums = 0;
    for (uint32_t f = f0; f < f1; f++) {
        sum += fc[f];
        sums += nseg_of(fc[f], o.SEG);
    }
    uint32_t inc = sum, incs = sums;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t x = __shfl_up(inc, d, 64), y = __shfl_up(incs, d, 64);
        if ((t & 63) >= (uint32_t)d) {
            inc += x;
            incs += y;
        }
    }
    if ((t & 63) == 63) {
        wsum[0][t >> 6] = inc;
        wsum[1][t >> 6] = incs;
    }
    __syncthreads();
    uint32_t run = inc - sum, runs = incs - sums, used = 0;
#pragma unroll
    for (uint32_t wv = 0; wv < BT / 64; wv++) {
        if (wv < (t >> 6)) {
            run += wsum[0][wv];
            runs += wsum[1][wv];
        }
        used += wsum[1][wv];
    }
    for (uint32_t f = f0; f < f1; f++) {
        const uint32_t c = fc[f], ns = nseg_of(c, o.SEG);
        fo[f] = run;
        if (first + f < NB) {
            const uint32_t b = first + f, ent = lo + run, s0 = seg_lo + runs;
            o.hist[b] = c;
            o.bucket_off[b] = ent;
            o.seg_off[b] = s0;
            // balanced split, as msm_seg_desc: one segment per bucket unless c > SEG.  A bucket with many segments (skewed
            // scalars: 2^20 equal ones are 8192 segments of one bucket) is queued for the WHOLE workgroup (below) instead of
            // being written by this lane alone — the kernel every flat MSM waits for must not serialise on one lane
            uint32_t slot = FLAT_WIDE_Q;
            if (ns > FLAT_WIDE_NS) slot = atomicAdd(&nwide, 1u);
            if (slot < FLAT_WIDE_Q) {
                wide[slot][0] = c;
                wide[slot][1] = ent;
                wide[slot][2] = s0;
            } else {
                for (uint32_t k = 0; k < ns; k++) flat_seg_write(o, c, ns, ent, s0, k, lh);
            }
            if (ns > o.big_nseg) o.big_list[atomicAdd(o.big_count, 1u)] = b;
        }
        run += c;
        runs += ns;
    }
    for (uint32_t k = seg_lo + used + t; k < seg_hi; k += BT) o.seg_len[k] = 0;  // indices the bin did not need
    __syncthreads();
    for (uint32_t q = 0, nq = min(nwide, FLAT_WIDE_Q); q < nq; q++) {  // the queued many-segment buckets: one segment per lane and trip
        const uint32_t c = wide[q][0], ns = nseg_of(c, o.SEG);
        for (uint32_t k = t; k < ns; k += BT) flat_seg_write(o, c, ns, wide[q][1], wide[q][2], k, lh);
    }
    __syncthreads();
    for (uint32_t i = t; i <= o.SEG; i += BT)
        if (lh[i]) atomicAdd(&o.len_hist[i * LEN_STRIDE], lh[i]);
    if (cnt <= FLAT_BIN_CAP) {
        // the bin's entries lie window by window (msm_flat_scan_bins); they are placed in chunks of PLACE_U x 1024 consecutive
        // entries, so a bucket's entries keep that order up to the chunk size — what the accumulation's locality rests on
        for (uint32_t i = t; i < cnt; i += PLACE_U * BT) {
            uint2 e[PLACE_U];
#pragma unroll
            for (int u = 0; u < PLACE_U; u++) e[u] = i + u * BT < cnt ? tmp[lo + i + u * BT] : make_uint2(0u, 0u);
#pragma unroll
            for (int u = 0; u < PLACE_U; u++)
                if (i + u * BT < cnt) stage[atomicAdd(&fo[e[u].y & fmask], 1u)] = e[u].x;
        }
        __syncthreads();
        for (uint32_t i = t; i < cnt; i += BT) sorted[lo + i] = stage[i];
        if (tw.sorted2)
            for (uint32_t i = t; i < cnt; i += BT) tw.sorted2[lo + i] = tw.map(stage[i]);
    } else {  // oversized bin (many equal digits): scattered 4-byte stores, correct for any size
        for (uint32_t i = t; i < cnt; i += BT) {
            uint2 e = tmp[lo + i];
            const uint32_t at = lo + atomicAdd(&fo[e.y & fmask], 1u);
            sorted[at] = e.x;
            if (tw.sorted2) tw.sorted2[at] = tw.map(e.x);
        }
    }
}
// The follower of a twin pair takes the lead's bucket and segment descriptors (TwinCopy, msm_stages.h): one launch.
__global__ void __launch_bounds__(256) msm_twin_copy(TwinCopy c) {
    SWM_LIGHT_KERNEL();
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
    for (int r = 0; r < c.k; r++)
        for (uint32_t i = gid; i < c.words[r]; i += step) c.dst[r][i] = c.src[r][i];
}

// Exclusive scans of the bucket counts and of the per-bucket segment counts, in three launches:
// per-workgroup totals, a single-workgroup scan of those totals, per-workgroup scan + offset.
// (SCAN_BLOCK lanes with SCAN_ITEMS consecutive buckets each: msm_stages.h — the driver sizes the totals by SCAN_TILE)

__device__ __forceinline__ void block_inclusive_scan2(uint32_t& a, uint32_t& b, uint32_t* sa, uint32_t* sb) {
    // Hillis-Steele over SCAN_BLOCK lanes (values returned in place: inclusive prefix)
    uint32_t tid = threadIdx.x;
    sa[tid] = a;
    sb[tid] = b;
    __syncthreads();
    for (uint32_t d = 1; d < SCAN_BLOCK; d <<= 1) {
        uint32_t va = tid >= d ? sa[tid - d] : 0, vb = tid >= d ? sb[tid - d] : 0;
        __syncthreads();
        sa[tid] += va;
        sb[tid] += vb;
        __syncthreads();
    }
    a = sa[tid];
    b = sb[tid];
}

__global__ void __launch_bounds__(SCAN_BLOCK) msm_scan_totals(const uint32_t* __restrict__ hist, uint32_t NB, uint32_t SEG,
                                                             uint32_t* __restrict__ tot_cnt,
                                                             uint32_t* __restrict__ tot_seg) {
    __shared__ uint32_t sa[SCAN_BLOCK], sb[SCAN_BLOCK];
    uint32_t lo = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    uint32_t a = 0, b = 0;
    for (uint32_t i = lo; i < min(lo + SCAN_ITEMS, NB); i++) {
        a += hist[i];
        b += nseg_of(hist[i], SEG);
    }
    block_inclusive_scan2(a, b, sa, sb);
    if (threadIdx.x == SCAN_BLOCK - 1) {
        tot_cnt[blockIdx.x] = a;
        tot_seg[blockIdx.x] = b;
    }
}

// one workgroup: exclusive scan of the tile totals, in place; grand totals to tot[ntiles]
__global__ void __launch_bounds__(SCAN_BLOCK) msm_scan_mid(uint32_t* __restrict__ tot_cnt, uint32_t* __restrict__ tot_seg,
                                                          uint32_t ntiles) {
    __shared__ uint32_t sa[SCAN_BLOCK], sb[SCAN_BLOCK];
    uint32_t per = (ntiles + SCAN_BLOCK - 1) / SCAN_BLOCK;
    uint32_t lo = threadIdx.x * per, hi = min(lo + per, ntiles);
    uint32_t a = 0, b = 0;
    for (uint32_t i = lo; i < hi; i++) {
        a += tot_cnt[i];
        b += tot_seg[i];
    }
    uint32_t la = a, lb = b;
    block_inclusive_scan2(a, b, sa, sb);
    uint32_t ra = a - la, rb = b - lb;
    for (uint32_t i = lo; i < hi; i++) {
        uint32_t ca = tot_cnt[i], cb = tot_seg[i];
        tot_cnt[i] = ra;
        tot_seg[i] = rb;
        ra += ca;
        rb += cb;
    }
    if (threadIdx.x == SCAN_BLOCK - 1) {
        tot_cnt[ntiles] = a;
        tot_seg[ntiles] = b;
    }
}

// Also appends buckets with > big_nseg segments to the big list.
__global__ void __launch_bounds__(SCAN_BLOCK) msm_scan_final(const uint32_t* __restrict__ hist, uint32_t NB, uint32_t SEG,
                                                            const uint32_t* __restrict__ tot_cnt,
                                                            const uint32_t* __restrict__ tot_seg, uint32_t ntiles,
                                                            uint32_t* __restrict__ bucket_off,
                                                            uint32_t* __restrict__ seg_off,
                                                            uint32_t* __restrict__ big_count,
                                                            uint32_t* __restrict__ big_list, uint32_t big_nseg) {
    __shared__ uint32_t sa[SCAN_BLOCK], sb[SCAN_BLOCK];
    uint32_t lo = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    uint32_t hi = min(lo + SCAN_ITEMS, NB);
    uint32_t a = 0, b = 0;
    for (uint32_t i = lo; i < hi; i++) {
        a += hist[i];
        b += nseg_of(hist[i], SEG);
    }
    uint32_t la = a, lb = b;
    block_inclusive_scan2(a, b, sa, sb);
    uint32_t ra = tot_cnt[blockIdx.x] + a - la, rb = tot_seg[blockIdx.x] + b - lb;
    for (uint32_t i = lo; i < hi; i++) {
        uint32_t h = hist[i], ns = nseg_of(h, SEG);
        bucket_off[i] = ra;
        seg_off[i] = rb;
        ra += h;
        rb += ns;
        if (ns > big_nseg) big_list[atomicAdd(big_count, 1u)] = i;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        bucket_off[NB] = tot_cnt[ntiles];
        seg_off[NB] = tot_seg[ntiles];
    }
}

// bucket that owns segment `seg`: largest b with seg_off[b] <= seg (empty buckets share offsets; skip them)
__device__ __forceinline__ uint32_t bucket_of_segment(const uint32_t* __restrict__ seg_off, uint32_t NB, uint32_t seg) {
    uint32_t lo = 0, hi = NB;  // invariant: seg_off[lo] <= seg < seg_off[hi]
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (seg_off[mid] <= seg) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Segment descriptors + ordering by length.  Lanes of a wave run in lock step, so a wave costs as much as its
// longest segment; bucket sizes are Poisson-spread (a wave of 64 unsorted segments idles ~25 % of its lane-cycles).
// Segments are therefore counting-sorted by length (longest first) and handed to lanes in that order.
static constexpr int ORD_THREADS = 256;
// (the SEG + 1 length counters / cursors sit one per 128-byte line, LEN_STRIDE: every workgroup of msm_seg_desc and
// msm_seg_order updates most of them; packed, those atomics queue up behind one another — see FLAT_CUR_STRIDE)
__global__ void __launch_bounds__(ORD_THREADS) msm_seg_desc(const uint32_t* __restrict__ bucket_off,
                                                            const uint32_t* __restrict__ seg_off, uint32_t NB,
                                                            uint32_t SEG, uint32_t* __restrict__ seg_start,
                                                            uint32_t* __restrict__ seg_len,
                                                            uint32_t* __restrict__ len_hist) {
    __shared__ uint32_t lh[SEG_MAX + 1];
    for (uint32_t i = threadIdx.x; i <= SEG; i += ORD_THREADS) lh[i] = 0;
    __syncthreads();
    uint32_t seg = blockIdx.x * ORD_THREADS + threadIdx.x;
    if (seg < seg_off[NB]) {
        uint32_t b = bucket_of_segment(seg_off, NB, seg);
        uint32_t s = seg - seg_off[b], ns = seg_off[b + 1] - seg_off[b];
        uint32_t o = bucket_off[b], cnt = bucket_off[b + 1] - o;
        uint32_t k = o + (uint32_t)(((uint64_t)cnt * s) / ns), e = o + (uint32_t)(((uint64_t)cnt * (s + 1)) / ns);
        seg_start[seg] = k;
        seg_len[seg] = e - k;
        atomicAdd(&lh[SEG - (e - k)], 1u);  // bin 0 = longest
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i <= SEG; i += ORD_THREADS)
        if (lh[i]) atomicAdd(&len_hist[i * LEN_STRIDE], lh[i]);
}
// (4096 segments per workgroup — r04; 256 before: every workgroup reserves a run per length class with a returning global atomic,
// and ~230 k of those on 129 addresses were the kernel's 24 us at 2^20 points)
static constexpr int ORD2_THREADS = 1024, ORD2_U = 4;
// r06: the exclusive scan of the SEG + 1 length counts — until r05 a single-wave kernel of its own between the sort and the
// accumulation of every MSM (5 us + a launch gap on the path of every job whose accumulation waits for its sort) — is done by
// every workgroup here for itself: three counters per lane of its first wave, a shuffle scan, the offsets in LDS.  The counts stay
// as the sort wrote them; the runs a workgroup reserves come from a second, zeroed array of cursors.  Workgroup 0 writes
// *nseg_live (the segments that hold entries: the lanes of work of the accumulation).
__global__ void __launch_bounds__(ORD2_THREADS) msm_seg_order(const uint32_t* __restrict__ seg_len,
                                                              const uint32_t* __restrict__ nseg_ptr, uint32_t SEG,
                                                              const uint32_t* __restrict__ len_hist /* SEG + 1 counts */,
                                                              uint32_t* __restrict__ len_cursor /* zeroed, advanced */,
                                                              uint32_t* __restrict__ nseg_live, uint32_t* __restrict__ order) {
    SWM_LIGHT_KERNEL();
    __shared__ uint32_t lh[SEG_MAX + 1], loff[SEG_MAX + 1];
    static_assert(SEG_MAX + 1 <= 3 * 64, "three counters per lane");
    for (uint32_t i = threadIdx.x; i <= SEG; i += ORD2_THREADS) lh[i] = 0;
    if (threadIdx.x < 64) {
        const uint32_t l = threadIdx.x;
        uint32_t c[3], sum = 0;
#pragma unroll
        for (int u = 0; u < 3; u++) {
            const uint32_t i = 3 * l + u;
            c[u] = i <= SEG ? len_hist[i * LEN_STRIDE] : 0u;
            sum += c[u];
        }
        uint32_t inc = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            uint32_t x = __shfl_up(inc, d, 64);
            if (l >= (uint32_t)d) inc += x;
        }
        uint32_t run = inc - sum;
#pragma unroll
        for (int u = 0; u < 3; u++) {
            const uint32_t i = 3 * l + u;
            if (i <= SEG) loff[i] = run;
            if (i == SEG && blockIdx.x == 0) *nseg_live = run;  // class SEG holds the empty segments: everything before it has entries
            run += c[u];
        }
    }
    __syncthreads();
    // *nseg_ptr bounds the segment INDICES in use; the flat schedule leaves indices without entries between the bins
    // (msm_flat_bin_sort): those are not handed to a lane
    const uint32_t nseg = *nseg_ptr;
    uint32_t bin[ORD2_U];
    bool live[ORD2_U];
#pragma unroll
    for (int u = 0; u < ORD2_U; u++) {
        const uint32_t seg = (blockIdx.x * ORD2_U + u) * ORD2_THREADS + threadIdx.x;
        const uint32_t len = seg < nseg ? seg_len[seg] & 0xffu : 0u;  // (bits 8 ..: the stride of an interleaved segment)
        live[u] = len != 0;
        bin[u] = SEG - len;
        if (live[u]) atomicAdd(&lh[bin[u]], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i <= SEG; i += ORD2_THREADS) {
        uint32_t v = lh[i];
        if (v) lh[i] = loff[i] + atomicAdd(&len_cursor[i * LEN_STRIDE], v);  // reserve a run; lh[i] = its start
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < ORD2_U; u++)
        if (live[u]) order[atomicAdd(&lh[bin[u]], 1u)] = (blockIdx.x * ORD2_U + u) * ORD2_THREADS + threadIdx.x;
}

// ---------------------------------------------------------------------------------------------- stages (each enqueues on the context's stream)
// Signed-digit recoding of the scalars into b.digits; the status words (big_count + 1, + 2) were zeroed with the histogram.
int msm_digits_stage(swm_ctx* ctx, const MsmShape& s, const MsmBuffers& b, const void* d_scalars, size_t n, int mont,
                     const MsmInfMask& inf, const MsmTable& tab) {
    const unsigned grid_n = (unsigned)std::min<size_t>((n + 255) / 256, 256 * 16);
    SWM_LAUNCH(ctx, "msm_digits", msm_digits, dim3(grid_n), dim3(256), 0, reinterpret_cast<const Fr*>(d_scalars), n, mont, s.pl,
               b.digits, inf.mask, inf.first, b.big_count + 1, s.dshard, tab.scalar_stride != 1 ? tab.blk_log : 31u,
               tab.scalar_stride != 1 ? tab.bstride : (size_t)0);
    return SWM_OK;
}
// Flat schedule: two-level counting sort over the shared bucket set; the fine counts written by msm_flat_bin_sort are the
// histogram the scans consume, and the bins are contiguous bucket ranges, so `sorted` is in bucket order.
// lead (a twin pair's LEAD, filled in but for `ready`): the bin sort also writes the sorted array of lead->tab2, and lead->sorted
// is recorded after it.
int msm_sort_flat(swm_ctx* ctx, const MsmShape& s, const MsmBuffers& b, const MsmTable& tab, size_t n, MsmTwinSrc* lead) {
    const WinLayout& pl = s.pl;
    uint32_t ctile = 65536;  // digits per workgroup of the coarse histogram: at least ~256 workgroups
    while (ctile > 4096 && (size_t)ctile * 256 > s.total) ctile >>= 1;
    // digits per workgroup of the partition: 16 K (r04: half the (tile, bin) runs and reserving atomics of 8 K tiles, one
    // workgroup per CU instead of two — prove 2^20 51.6 -> 51.0 ms, and the transforms beside it run a quarter faster) as long
    // as the pairs and the three per-bin arrays fit the 160 KB of LDS (up to 2 048 bins); 8 K above
    const size_t lds_bins = (3 * (size_t)((s.flat_bins + 3) & ~3u) + 1024) * 4;
    const bool tile16 = 16384 * sizeof(uint2) + lds_bins <= 160 * 1024;
    const uint32_t part_tile = tile16 ? 16384u : 8192u;
    const size_t lds_part = (size_t)part_tile * sizeof(uint2) + lds_bins;
    SWM_TRY(allow_big_lds(ctx, tile16 ? LDS_FLAT_PARTITION_16 : LDS_FLAT_PARTITION_8,
                          tile16 ? (const void*)msm_flat_partition<16> : (const void*)msm_flat_partition<8>, lds_part));
    const size_t lds_bin = ((size_t)FLAT_BIN_CAP + 2 * ((size_t)1 << s.flat_fb)) * 4;
    SWM_TRY(allow_big_lds(ctx, LDS_FLAT_BIN_SORT, (const void*)msm_flat_bin_sort<BIN_THREADS>, lds_bin));
    // (256-lane forms of the partition and the bin sort for sorts that run beside an accumulation: built and measured in r05 —
    // 51.15 vs 50.8 ms at 2^20 with the issue priorities in place — and removed in r06)
    SWM_LAUNCH(ctx, "msm_flat_hist", msm_flat_coarse_hist, dim3((unsigned)((n + ctile - 1) / ctile), pl.nwin), dim3(SORT_THREADS), 0,
               b.digits, n, s.flat_fb, s.flat_bins, ctile, b.flat_cnt);
    unsigned scan_threads = 64;
    const bool one_bin_per_lane = s.flat_bins <= 1024;
    while (scan_threads * (one_bin_per_lane ? 1 : 4) < s.flat_bins) scan_threads <<= 1;
    SWM_LAUNCH(ctx, "msm_flat_hist", one_bin_per_lane ? msm_flat_scan_bins<1> : msm_flat_scan_bins<4>, dim3(1), dim3(scan_threads), 0,
               b.flat_cnt, s.flat_bins, pl.nwin, b.flat_off, b.flat_win_off, s.flat_fb, s.SEG, b.flat_seg_off);
    SWM_LAUNCH(ctx, "msm_flat_partition", tile16 ? msm_flat_partition<16> : msm_flat_partition<8>,
               dim3((unsigned)((n + part_tile - 1) / part_tile), pl.nwin), dim3(1024), lds_part, b.digits, n, (uint32_t)tab.stride,
               (uint32_t)tab.offset, tab.blk_log, (uint32_t)tab.bstride, s.flat_fb, s.flat_bins, b.flat_win_off, pl.nwin, b.flat_cur, b.pairs);
    // (bucket / segment offsets, segment descriptors, the length histogram and the list of oversized buckets come out of
    // the bin sort: no scans over the bucket histogram, no msm_seg_desc)
    const FlatSegOut fso{b.hist,    b.bucket_off, b.seg_off, b.seg_start, b.seg_len, b.len_hist,
                         b.big_count, b.big_list, s.SEG,     s.big_nseg,  msm_interleaves(s) ? 1u : 0u};
    TwinOut two{nullptr, 1u, 0u, 0u};
    if (lead) {
        // (the array is read by the accumulation of the previous pair's follower)
        SWM_TRY(scratch(ctx, "msmT.sorted", s.total * 4, (void**)&two.sorted2));
        if (ctx->twin_sorted_event) SWM_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->twin_sorted_event, 0));
        two.tstride = (uint32_t)tab.stride;
        two.dstride = (uint32_t)lead->tab2.stride - (uint32_t)tab.stride;
        two.doff = (uint32_t)lead->tab2.offset - (uint32_t)tab.offset;
    }
    SWM_LAUNCH(ctx, "msm_flat_bin_sort", msm_flat_bin_sort<BIN_THREADS>, dim3(s.flat_bins), dim3(BIN_THREADS), lds_bin,
               (const uint2*)b.pairs, s.flat_fb, pl.NB, b.flat_off, b.flat_seg_off, fso, b.sorted, two);
    if (lead) {
        SWM_HIP(ctx, hipEventRecord(lead->sorted, ctx->stream));
        lead->ready = true;
    }
    return SWM_OK;
}
// Per-window schedule: counting sort by (window, bucket), with the two-level scatter for large MSMs.
int msm_sort_windows(swm_ctx* ctx, const MsmShape& s, const MsmBuffers& b, size_t n) {
    const WinLayout& pl = s.pl;
    // tile size: flat between 2^15 and 2^18 on MI355X (the scatter is bound by its 4-byte scattered writes: 73 G digits/s)
    const uint32_t SORT_TILE = SORT_TILE_MIN;
    unsigned tiles = (unsigned)((n + SORT_TILE - 1) / SORT_TILE);
    size_t lds_sort = (size_t)pl.maxB * 4;
    SWM_TRY(allow_big_lds(ctx, LDS_HIST, (const void*)msm_hist, lds_sort));
    SWM_TRY(allow_big_lds(ctx, LDS_SCATTER, (const void*)msm_scatter, lds_sort));
    SWM_LAUNCH(ctx, "msm_hist", msm_hist, dim3(tiles, pl.nwin), dim3(SORT_THREADS), lds_sort, b.digits, n, pl, SORT_TILE, b.hist);
    SWM_LAUNCH(ctx, "msm_scan", msm_scan_totals, dim3(s.scan_tiles), dim3(SCAN_BLOCK), 0, b.hist, pl.NB, s.SEG, b.tot_cnt, b.tot_seg);
    SWM_LAUNCH(ctx, "msm_scan", msm_scan_mid, dim3(1), dim3(SCAN_BLOCK), 0, b.tot_cnt, b.tot_seg, s.scan_tiles);
    SWM_LAUNCH(ctx, "msm_scan", msm_scan_final, dim3(s.scan_tiles), dim3(SCAN_BLOCK), 0, b.hist, pl.NB, s.SEG, b.tot_cnt, b.tot_seg,
               s.scan_tiles, b.bucket_off, b.seg_off, b.big_count, b.big_list, s.big_nseg);
    if (s.two_level) {
        SWM_TRY(allow_big_lds(ctx, LDS_PARTITION, (const void*)msm_partition, (size_t)PART_TILE * sizeof(uint2)));
        SWM_TRY(allow_big_lds(ctx, LDS_BIN_SORT, (const void*)msm_bin_sort, (size_t)BIN_CAP * 4));
        SWM_LAUNCH(ctx, "msm_bin_check", msm_bin_check, dim3((s.bp.max_nbins + 255) / 256, pl.nwin), dim3(256), 0, b.bucket_off, pl,
                   s.bp, b.two_level_bad);
        SWM_LAUNCH(ctx, "msm_partition", msm_partition, dim3((unsigned)((n + PART_TILE - 1) / PART_TILE), pl.nwin), dim3(1024),
                   (size_t)PART_TILE * sizeof(uint2), b.digits, n, pl, s.bp, b.bucket_off, b.bin_cursor, b.two_level_bad, b.pairs);
        SWM_LAUNCH(ctx, "msm_bin_sort", msm_bin_sort, dim3(s.bp.max_nbins, pl.nwin), dim3(BIN_THREADS), (size_t)BIN_CAP * 4,
                   (const uint2*)b.pairs, pl, s.bp, b.bucket_off, b.two_level_bad, b.sorted);
    }
    SWM_LAUNCH(ctx, "msm_scatter", msm_scatter, dim3(tiles, pl.nwin), dim3(SORT_THREADS), lds_sort, b.digits, n, pl, SORT_TILE,
               b.bucket_off, b.cursor, b.sorted, s.two_level ? (const uint32_t*)b.two_level_bad : (const uint32_t*)nullptr);
    return SWM_OK;
}
// Segment planning: the descriptors (per-window schedule: msm_seg_desc; the flat schedule's bin sort has written them) and the
// segments ordered by length, longest first, with the count of those that hold entries (msm_seg_order).
int msm_seg_order_stage(swm_ctx* ctx, const MsmShape& s, const MsmBuffers& b) {
    unsigned grid_s = (unsigned)((s.nseg_max + ORD_THREADS - 1) / ORD_THREADS);
    if (!s.flat)
        SWM_LAUNCH(ctx, "msm_seg_order", msm_seg_desc, dim3(grid_s), dim3(ORD_THREADS), 0, b.bucket_off, b.seg_off, s.pl.NB, s.SEG,
                   b.seg_start, b.seg_len, b.len_hist);
    SWM_LAUNCH(ctx, "msm_seg_order", msm_seg_order, dim3((unsigned)((s.nseg_max + ORD2_THREADS * ORD2_U - 1) / (ORD2_THREADS * ORD2_U))),
               dim3(ORD2_THREADS), 0, b.seg_len, msm_seg_space(s, b), s.SEG, (const uint32_t*)b.len_hist, b.len_cursor, msm_nseg_live(b),
               b.order);
    return SWM_OK;
}
// The follower of a twin pair: the ranges the driver's msm_twin_copy_stage chose, in one launch.
int msm_twin_copy_launch(swm_ctx* ctx, const TwinCopy& tc) {
    SWM_LAUNCH(ctx, "msm_twin_copy", msm_twin_copy, dim3(1024), dim3(256), 0, tc);
    return SWM_OK;
}

}  // namespace swm

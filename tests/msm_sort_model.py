"""A digit model of the MSM's sort stage (csrc/msm_sort.hip: msm_digits, msm_flat_partition / msm_flat_bin_sort or msm_hist / msm_scan_* /
msm_seg_desc / msm_scatter, msm_seg_order) in plain numpy and Python integers, a checker that holds the arrays the stage leaves on
the device (swm_selftest_msm_sort) to it, and scalar vectors whose buckets sit exactly on the entry counts the stage branches on.
No device, no library.

Model.  From the scalars, the window layout, the table's rows per window and the job's offset: the entry word of every non-zero
digit (table row w * stride + offset + i, or the point index i without a table, sign of the digit in bit 31), its bucket (the flat
schedule's windows share ONE set of 2^(c-1) buckets; the per-window schedule gives window w its own 2^(c[w]-1)), the counts, the
segments per bucket ns = ceil(count / SEG) and their lengths (round-robin — segment k holds ceil((count - k) / ns) entries at
stride ns — for twisted Edwards jobs with ns > 1, consecutive floor cuts otherwise), the big set {b : ns > big_nseg}, the length
histogram, the live-segment count.

check() asserts what the code promises and is free where the code is free: the order of the entries inside a bucket, the order of
big_list, the order of the segments inside one length class, where a bucket's entries and segment indices lie."""
import numpy as np

R = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001   # the scalar field of BLS12-377
FLAT_WIDE_NS = 16     # msm_sort.hip: a bucket with more segments is written by the whole workgroup of msm_flat_bin_sort
UNWRITTEN = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ digits
def window_widths(nwin):
    """msm_windows: 254 recoding bits over nwin windows whose widths differ by at most one, the wider ones first"""
    base, extra = divmod(254, nwin)
    return [base + (1 if w < extra else 0) for w in range(nwin)]


def signed_digits(sc, nwin):
    """The signed-digit recoding of msm_sort.hip (for_each_digit) on the layout of msm_windows: int64 [nwin, n], digit w of scalar i.
    sc: (n, 4) uint64, standard form."""
    sc = np.ascontiguousarray(sc, dtype=np.uint64)
    out = np.empty((nwin, sc.shape[0]), dtype=np.int64)
    carry = np.zeros(sc.shape[0], dtype=np.int64)
    bit = 0
    for w, c in enumerate(window_widths(nwin)):
        limb, sh = divmod(bit, 64)
        v = sc[:, limb] >> np.uint64(sh)
        if sh + c > 64 and limb + 1 < 4:
            v = v | (sc[:, limb + 1] << np.uint64(64 - sh))
        d = (v & np.uint64((1 << c) - 1)).astype(np.int64) + carry
        carry = (d > (1 << (c - 1))).astype(np.int64)
        out[w] = d - (carry << c)
        bit += c
    return out


def buckets(sc, nwin):
    """signed_digits() without the signs: int64 [nwin, n] with the bucket index |digit| - 1 of every digit, -1 for a zero digit."""
    return np.abs(signed_digits(sc, nwin)) - 1


def limbs(values):
    """Python integers -> (n, 4) uint64, little-endian limbs"""
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        for k in range(4):
            out[i, k] = (v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


def per_window_c(n):
    """msm_plan: the window width of the per-window schedule for n points"""
    return 10 if n <= 2048 else 12 if n <= 98304 else 14 if n <= 393216 else 16


def twin_map(e, tstride, dstride, doff):
    """TwinOut::map of msm_sort.hip on uint32 arrays, with the kernel's wrapped 32-bit arithmetic: dstride and doff are the wrapped
    differences msm_sort_flat computes."""
    e = np.asarray(e, dtype=np.uint32)
    row = e & np.uint32(0x7FFFFFFF)
    w = row // np.uint32(tstride)
    with np.errstate(over="ignore"):
        moved = row + w * np.uint32(dstride) + np.uint32(doff)
    return (e & np.uint32(0x80000000)) | (moved & np.uint32(0x7FFFFFFF))


# ------------------------------------------------------------------------------------------------ model
def segment_lengths(count, seg, interleave):
    """lengths of the ns = ceil(count / seg) segments of a bucket of `count` entries, in segment order"""
    ns = -(-count // seg)
    if interleave and ns > 1:
        return [-(-(count - k) // ns) for k in range(ns)]
    return [count * (k + 1) // ns - count * k // ns for k in range(ns)]


class Model:
    """What the sort stage must leave for one job.  shape: the dict swm_selftest_msm_sort reports (flat, nwin, c, NB, SEG, big_nseg,
    interleave, tstride are read); skip: boolean [n], the scalars whose base is the identity (their digits are dropped); follow:
    None or (rows per window, offset) of the follower's table."""

    def __init__(self, sc, shape, offset=0, skip=None, follow=None):
        sc = np.ascontiguousarray(sc, dtype=np.uint64).reshape(-1, 4)
        self.n = n = sc.shape[0]
        self.shape = dict(shape)
        self.flat, self.nwin, self.seg, self.big_nseg = bool(shape["flat"]), shape["nwin"], shape["SEG"], shape["big_nseg"]
        self.interleave = bool(shape["interleave"])
        self.widths = window_widths(self.nwin)
        assert list(shape["c"]) == self.widths, "shape: window widths %r, msm_windows gives %r" % (shape["c"], self.widths)
        if self.flat:
            boff = [0] * self.nwin
            self.NB = 1 << (self.widths[0] - 1)
        else:
            boff = [int(v) for v in np.cumsum([0] + [1 << (c - 1) for c in self.widths[:-1]])]
            self.NB = sum(1 << (c - 1) for c in self.widths)
        assert shape["NB"] == self.NB and shape["total"] == n * self.nwin
        self.boff = boff
        d = signed_digits(sc, self.nwin)
        if skip is not None:
            d[:, np.asarray(skip, dtype=bool)] = 0
        w, i = np.nonzero(d)
        dv = d[w, i]
        row = (w * shape["tstride"] + offset + i) if self.flat else i
        assert row.size == 0 or row.max() < 1 << 31
        self.word = (row | ((dv < 0).astype(np.int64) << 31)).astype(np.uint32)
        self.bucket = np.asarray(boff, dtype=np.int64)[w] + np.abs(dv) - 1
        self.window = w
        self.count = np.bincount(self.bucket, minlength=self.NB).astype(np.int64)
        self.entries = int(self.word.size)
        self.ns = -(-self.count // self.seg)
        self.big = set(int(b) for b in np.nonzero(self.ns > self.big_nseg)[0])
        self.nseg_live = int(self.ns.sum())
        # segments per length: buckets of one segment directly, the others bucket by bucket
        lh = np.bincount(self.count[self.ns == 1], minlength=self.seg + 1).astype(np.int64)
        for b in np.nonzero(self.ns > 1)[0]:
            for ln in segment_lengths(int(self.count[b]), self.seg, self.interleave):
                lh[ln] += 1
        self.len_count = lh                      # [length] -> segments
        self.len_hist = lh[::-1].copy()          # the device's classes: class i = segments of SEG - i entries
        self._keys = None
        self.follow = follow
        if follow is not None:
            self.dstride = (follow[0] - shape["tstride"]) % (1 << 32)
            self.doff = (follow[1] - offset) % (1 << 32)

    def sorted_keys(self):
        """bucket << 32 | word of every entry, ascending (computed once)"""
        if self._keys is None:
            self._keys = np.sort((self.bucket.astype(np.uint64) << np.uint64(32)) | self.word.astype(np.uint64))
        return self._keys

    def arrays(self, gap=3):
        """Arrays that meet every promise, as a device run could have left them: buckets in index order, `gap` unused segment indices
        (length 0) after every 64th bucket the way the flat schedule's bins leave some, segments ordered by length."""
        sorted_ = (self.sorted_keys() & np.uint64(UNWRITTEN)).astype(np.uint32)
        bucket_off = np.concatenate([[0], np.cumsum(self.count)[:-1]]).astype(np.uint32)
        pad = np.zeros(self.NB, dtype=np.int64)
        if self.flat:
            pad[63::64] = gap
        seg_off = np.concatenate([[0], np.cumsum(self.ns + pad)[:-1]]).astype(np.uint32)
        bound = int((self.ns + pad).sum())
        nseg_max = self.shape["nseg_max"]
        assert bound <= nseg_max
        seg_start = np.full(nseg_max, UNWRITTEN, dtype=np.uint32)
        seg_len = np.full(nseg_max, UNWRITTEN, dtype=np.uint32)
        seg_len[:bound] = 0
        one = np.nonzero(self.ns == 1)[0]
        seg_start[seg_off[one]] = bucket_off[one]
        seg_len[seg_off[one]] = self.count[one]
        for b in np.nonzero(self.ns > 1)[0]:
            c, ns, s0, ent = int(self.count[b]), int(self.ns[b]), int(seg_off[b]), int(bucket_off[b])
            lens = segment_lengths(c, self.seg, self.interleave)
            for k, ln in enumerate(lens):
                if self.interleave:
                    seg_start[s0 + k], seg_len[s0 + k] = ent + k, ln | (ns << 8)
                else:
                    seg_start[s0 + k], seg_len[s0 + k] = ent + c * k // ns, ln
        live = np.nonzero((seg_len[:bound] & 0xFF) != 0)[0]
        order = np.full(nseg_max, UNWRITTEN, dtype=np.uint32)
        order[:live.size] = live[np.argsort(-(seg_len[live] & 0xFF).astype(np.int64), kind="stable")]
        big_list = np.full(self.NB, UNWRITTEN, dtype=np.uint32)
        big = sorted(self.big)
        big_list[:len(big)] = big
        out = {"hist": self.count.astype(np.uint32), "bucket_off": bucket_off, "seg_off": seg_off, "sorted": sorted_,
               "seg_start": seg_start, "seg_len": seg_len, "order": order, "len_hist": self.len_hist.astype(np.uint32),
               "big_list": big_list, "seg_bound": bound, "nseg_live": self.nseg_live, "big_count": len(big), "bad_scalar": 0,
               "zero_points": 0, "entries": self.entries}
        if self.follow is not None:
            out["sorted2"] = twin_map(sorted_, self.shape["tstride"], self.dstride, self.doff)
        return out


# ------------------------------------------------------------------------------------------------ checker
class SortMismatch(AssertionError):
    pass


def fail(tag, fmt, *args):
    raise SortMismatch("%s: %s" % (tag, fmt % args))


def check(shape, arrays, model):
    """Holds the downloaded arrays of one job to the model; raises SortMismatch whose message starts with the name of the promise
    that is broken (hist, entries, ranges, unwritten, multiset, segments, lengths, cover, tail, nseg_live, len_hist, order,
    big_list, sorted2)."""
    m, a = model, arrays
    NB, total, seg = m.NB, shape["total"], m.seg
    hist = a["hist"].astype(np.int64)
    # 1, 2
    if not np.array_equal(hist, m.count):
        b = int(np.nonzero(hist != m.count)[0][0])
        fail("hist", "bucket %d holds %d entries, the model %d (%d buckets differ)", b, hist[b], m.count[b], int((hist != m.count).sum()))
    if a["entries"] != m.entries:
        fail("entries", "the status word says %d, the scalars have %d non-zero digits", a["entries"], m.entries)
    # 3: the ranges
    live = np.nonzero(hist)[0]
    off = a["bucket_off"].astype(np.int64)[live]
    cnt = hist[live]
    by = np.argsort(off, kind="stable")
    lo, hi = off[by], off[by] + cnt[by]
    if live.size and (hi.max() > total or (lo[1:] < hi[:-1]).any()):
        k = int(np.nonzero(np.concatenate([lo[1:] < hi[:-1], [hi[-1] > total]]))[0][0])
        fail("ranges", "bucket %d's entries [%d, %d) overlap the next range or exceed total = %d", live[by][k], lo[k], hi[k], total)
    owner = np.repeat(live, cnt)                                       # bucket of every position, range by range
    inside = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    pos = np.repeat(off, cnt) + inside
    got = a["sorted"][pos]
    # 4
    if (got == UNWRITTEN).any():
        k = int(np.nonzero(got == UNWRITTEN)[0][0])
        fail("unwritten", "sorted[%d] (bucket %d) was never written; %d such words", pos[k], owner[k], int((got == UNWRITTEN).sum()))
    # (one 64-bit key per entry, bucket above word: a plain sort instead of a lexsort)
    got_key = np.sort((owner.astype(np.uint64) << np.uint64(32)) | got.astype(np.uint64))
    want_key = m.sorted_keys()
    if not np.array_equal(got_key, want_key):
        k = int(np.nonzero(got_key != want_key)[0][0])
        fail("multiset", "bucket %d: entry 0x%08x where the model has 0x%08x in bucket %d (entries sorted per bucket; %d words differ)",
             int(got_key[k]) >> 32, int(got_key[k]) & UNWRITTEN, int(want_key[k]) & UNWRITTEN, int(want_key[k]) >> 32,
             int((got_key != want_key).sum()))
    # 5, 6: the segments of every bucket
    ns = m.ns[live]
    s0 = a["seg_off"].astype(np.int64)[live]
    bound = a["seg_bound"]
    sby = np.argsort(s0, kind="stable")
    if live.size and ((s0 + ns).max() > bound or (s0[sby][1:] < (s0 + ns)[sby][:-1]).any() or bound > shape["nseg_max"]):
        fail("segments", "the segment indices of two buckets overlap, or exceed the bound %d (nseg_max %d)", bound, shape["nseg_max"])
    if not m.flat and not (np.array_equal(a["seg_off"].astype(np.int64), np.cumsum(m.ns) - m.ns) and bound == m.nseg_live):
        fail("segments", "per-window schedule: seg_off is not the running sum of ceil(count / SEG), or the bound %d != %d", bound, m.nseg_live)
    sidx = np.repeat(s0, ns) + np.arange(ns.sum()) - np.repeat(np.cumsum(ns) - ns, ns)       # every segment of every bucket
    sown = np.repeat(np.arange(live.size), ns)                                                 # its bucket (index into live)
    raw = a["seg_len"][sidx].astype(np.int64)
    start = a["seg_start"][sidx].astype(np.int64)
    ln, stride_bits = raw & 0xFF, raw >> 8
    inter = (np.repeat(ns, ns) > 1) & m.interleave
    if (ln > seg).any() or (ln == 0).any():
        k = int(np.nonzero((ln > seg) | (ln == 0))[0][0])
        fail("lengths", "segment %d of bucket %d has %d entries (SEG = %d)", sidx[k], live[sown[k]], ln[k], seg)
    if (stride_bits[inter] != np.repeat(ns, ns)[inter]).any() or (stride_bits[~inter] != 0).any():
        k = int(np.nonzero(np.where(inter, stride_bits != np.repeat(ns, ns), stride_bits != 0))[0][0])
        fail("lengths", "segment %d of bucket %d (count %d): stride field %d, ceil(count / SEG) = %d, round-robin %d", sidx[k],
             live[sown[k]], cnt[sown[k]], stride_bits[k], ns[sown[k]], inter[k])
    first = np.cumsum(ns) - ns
    mx, mn = np.maximum.reduceat(ln, first) if live.size else ln, np.minimum.reduceat(ln, first) if live.size else ln
    if (mx - mn > 1).any():
        k = int(np.nonzero(mx - mn > 1)[0][0])
        fail("lengths", "bucket %d (count %d, %d segments): lengths from %d to %d", live[k], cnt[k], ns[k], mn[k], mx[k])
    step = np.where(inter, stride_bits, 1)
    covered = np.repeat(start, ln) + (np.arange(ln.sum()) - np.repeat(np.cumsum(ln) - ln, ln)) * np.repeat(step, ln)
    cown = np.repeat(sown, ln)
    cover_key = np.sort((cown.astype(np.uint64) << np.uint64(32)) | covered.astype(np.uint64))
    range_key = (np.repeat(np.arange(live.size), cnt).astype(np.uint64) << np.uint64(32)) | pos.astype(np.uint64)
    if not np.array_equal(cover_key, range_key):
        per = np.bincount(cown, minlength=live.size)
        bad = np.nonzero(per != cnt)[0]
        if bad.size == 0:
            bad = (cover_key[cover_key != range_key] >> np.uint64(32)).astype(np.int64)
        k = int(bad[0])
        fail("cover", "bucket %d: its %d segments cover %d positions, not its %d entries [%d, %d) exactly once", live[k], ns[k], per[k],
             cnt[k], off[k], off[k] + cnt[k])
    # 7: indices below the bound that belong to no bucket
    used = np.zeros(bound, dtype=bool)
    used[sidx] = True
    tail = np.nonzero(~used & ((a["seg_len"][:bound] & 0xFF) != 0))[0]
    if tail.size:
        fail("tail", "segment index %d belongs to no bucket and reads length 0x%x (%d such indices below the bound %d)", tail[0],
             a["seg_len"][tail[0]], tail.size, bound)
    # 8
    if a["nseg_live"] != m.nseg_live:
        fail("nseg_live", "%d segments with entries, the model has %d", a["nseg_live"], m.nseg_live)
    if not np.array_equal(a["len_hist"].astype(np.int64), m.len_hist):
        k = int(np.nonzero(a["len_hist"].astype(np.int64) != m.len_hist)[0][0])
        fail("len_hist", "%d segments of %d entries, the model has %d", a["len_hist"][k], seg - k, m.len_hist[k])
    order = a["order"][:m.nseg_live].astype(np.int64)
    if not np.array_equal(np.sort(order), np.sort(sidx)):
        missing = np.setdiff1d(sidx, order)
        fail("order", "not a permutation of the %d segments with entries: %d missing (first %s), %d repeated or foreign", sidx.size,
             missing.size, missing[:1], order.size - np.intersect1d(order, sidx).size)
    olen = a["seg_len"][order].astype(np.int64) & 0xFF
    if (olen[1:] > olen[:-1]).any():
        k = int(np.nonzero(olen[1:] > olen[:-1])[0][0])
        fail("order", "lengths increase along order: %d entries at %d, %d at %d", olen[k], k, olen[k + 1], k + 1)
    # 9
    bl = [int(b) for b in a["big_list"][:a["big_count"]]]
    if len(set(bl)) != len(bl) or set(bl) != m.big:
        fail("big_list", "lists %d buckets (%d distinct), the model's %d with more than %d segments: wrongly listed %r, missing %r",
             len(bl), len(set(bl)), len(m.big), m.big_nseg, sorted(set(bl) - m.big)[:4], sorted(m.big - set(bl))[:4])
    # 10
    if m.follow is not None:
        if not shape["lead"] or "sorted2" not in a:
            fail("sorted2", "the job did not sort as a lead")
        want2 = twin_map(a["sorted"][pos], shape["tstride"], m.dstride, m.doff)
        if not np.array_equal(a["sorted2"][pos], want2):
            k = int(np.nonzero(a["sorted2"][pos] != want2)[0][0])
            fail("sorted2", "sorted2[%d] = 0x%08x, the follower's row of 0x%08x is 0x%08x (%d words differ)", pos[k], a["sorted2"][pos[k]],
                 a["sorted"][pos[k]], want2[k], int((a["sorted2"][pos] != want2).sum()))


# ------------------------------------------------------------------------------------------------ ladders
def rung_targets(shape):
    """name -> entry count of every rung for a job of this shape.  G: the lanes msm_big_bucket_sum folds a bucket with."""
    seg, big, G, wide = shape["SEG"], shape["big_nseg"], 1 << shape["log_g"], FLAT_WIDE_NS
    t = {"1": 1, "2": 2, "SEG-1": seg - 1, "SEG": seg, "SEG+1": seg + 1, "2SEG-1": 2 * seg - 1, "2SEG": 2 * seg, "2SEG+1": 2 * seg + 1,
         "ns=big": big * seg, "ns=big,first+1": (big - 1) * seg + 1, "ns=big+1": (big + 1) * seg, "ns=big+1,first+1": big * seg + 1,
         "ns=wide": wide * seg, "ns=wide+1": wide * seg + 1,
         "ns=G-1": (G - 1) * seg, "ns=G": G * seg, "ns=G+1": G * seg + 1, "ns=2G+1": 2 * G * seg + 1, "negative": 3}
    return t


RUNGS = tuple(rung_targets({"SEG": 16, "big_nseg": 4, "log_g": 2}))


def predicates(shape):
    """name -> predicate on a bucket's entry count: every line the stage branches on"""
    seg, big, G = shape["SEG"], shape["big_nseg"], 1 << shape["log_g"]
    ns = lambda c: -(-c // seg)
    return {"c > SEG": lambda c: c > seg, "c % ns != 0": lambda c: c % ns(c) != 0, "ns > FLAT_WIDE_NS": lambda c: ns(c) > FLAT_WIDE_NS,
            "ns > big_nseg": lambda c: ns(c) > big, "ns > G": lambda c: ns(c) > G, "ns >= G": lambda c: ns(c) >= G,
            "ns > 2G": lambda c: ns(c) > 2 * G}


def ladder(shape, n, seed, rungs=RUNGS, skip=None):
    """A scalar vector of n elements (standard form) whose rung buckets hold EXACTLY their target counts under the model, and
    {rung name: bucket}.  A scalar v <= 2^(c0 - 2) has one non-zero digit (window 0, bucket v - 1), so every repeat adds one entry
    to one bucket; r - v has the digit -(v - 1) there (r = 1 mod 2^c0) and r's own digits above.  The rest is uniform; a uniform
    scalar with a digit in a rung bucket that would overfill it (or in the negative rung's bucket at all) is drawn again, then
    the repeats are topped up to the target.  skip: rows whose base is the identity (no rung scalar is placed there).
    Raises ValueError naming the rungs when they do not fit into n."""
    from pyref.prng import fr_array
    rng = np.random.default_rng(seed)
    targets = rung_targets(shape)
    nwin, c0, flat = shape["nwin"], shape["c"][0], bool(shape["flat"])
    assert R % (1 << c0) == 1
    free = np.ones(n, dtype=bool) if skip is None else ~np.asarray(skip, dtype=bool)
    need = sum(targets[k] for k in rungs)
    if need > int(free.sum()):
        raise ValueError("ladder: rungs %r need %d rows, the job has %d" % (list(rungs), need, int(free.sum())))
    # rung values: distinct, 2 <= v <= 2^(c0 - 2), away from the buckets r's own digits fall into
    r_digits = signed_digits(limbs([R - 2]), nwin)[:, 0]
    taken = set(int(abs(d)) - 1 for d in r_digits[1:]) if flat else set()
    value = {}
    for k in rungs:
        while True:
            v = int(rng.integers(3, (1 << (c0 - 2)) + 1))
            b = v - 2 if k == "negative" else v - 1
            if b not in taken:
                taken.add(b)
                value[k] = v
                break
    bucket = {k: (value[k] - 2 if k == "negative" else value[k] - 1) for k in rungs}
    rung_of = {b: k for k, b in bucket.items()}
    # which rows carry rung scalars: a seeded choice among the rows with a base; the background is everything else
    rows = rng.permutation(np.nonzero(free)[0])
    sc = fr_array(n, seed)
    for attempt in range(64):
        bk = buckets(sc, nwin)
        if not flat:
            bk = bk[:1]              # the rung buckets lie in window 0's own bucket set
        bk[:, rows[:need]] = -1      # rows that will be overwritten by rung scalars
        if skip is not None:
            bk[:, np.asarray(skip, dtype=bool)] = -1
        redraw = np.zeros(n, dtype=bool)
        for b, k in rung_of.items():
            hit = np.nonzero((bk == b).any(axis=0))[0]
            background = int((bk == b).sum())
            if k == "negative" or background > targets[k]:
                redraw[hit] = True
        if not redraw.any():
            break
        sc[redraw] = fr_array(int(redraw.sum()), seed * 1000 + attempt + 1)
    else:
        raise ValueError("ladder: the background keeps overfilling the rungs %r" % list(rungs))
    at = 0
    for k in rungs:
        b = bucket[k]
        repeats = targets[k] - int((bk == b).sum())
        s = R - value[k] if k == "negative" else value[k]
        sc[rows[at:at + repeats]] = limbs([s])
        at += repeats
    # rows reserved for repeats that the background made unnecessary keep small scalars of a bucket outside the ladder
    spare = next(v for v in range(3, 1 << (c0 - 2)) if v - 1 not in taken)
    sc[rows[at:need]] = limbs([spare])
    return sc, bucket


# ------------------------------------------------------------------------------------------------ shapes and the case table
def table_width(set_n):
    """msm_table_width: the window width of the table a resident set of set_n points gets (0: none)"""
    if set_n < 512:
        return 0
    lg = set_n.bit_length() - 1
    return lg + 2 if lg <= 14 else min(20, lg + 1)


def predicted_shape(n, set_n, lead=False):
    """msm_shape (default switches, a twisted Edwards table wherever the set has one) for a job of n points on a resident set of
    set_n points, in the fields swm_selftest_msm_sort reports."""
    c = table_width(set_n)
    flat = c != 0 and n >= 1 << max(c - 8, 0)
    if flat:
        nwin = -(-254 // c)
        nb = 1 << (c - 1)
    else:
        nwin = -(-254 // per_window_c(n))
        nb = sum(1 << (w - 1) for w in window_widths(nwin))
    total = n * nwin
    lat = flat and n < 262144
    seg, big, log_g = (128 if nb >= 262144 else 32), 16, 8
    if lat:
        seg = 32 if total // nb >= 10 else 16
        big = 4 if n < 65536 else 6
        log_g = 2
        while log_g < 6 and (1 << log_g) < 2 * (total // (nb * seg) + 1):
            log_g += 1
    fb = bins = 0
    if flat:
        target = min(28000, max(1024, total // 1024))
        want = 64
        while want < 4096 and want * target < total:
            want <<= 1
        while (nb >> fb) > want:
            fb += 1
        while (1 << fb) > 2048:
            fb -= 1
        bins = (nb + (1 << fb) - 1) >> fb
    quad = lat and nb <= 32768
    return {"flat": int(flat), "te": int(flat), "lat": int(lat), "quad": int(quad), "raw": int(flat and not quad), "interleave": int(flat),
            "lead": int(lead), "nwin": nwin, "NB": nb, "total": total, "SEG": seg, "big_nseg": big, "log_g": log_g, "flat_fb": fb,
            "flat_bins": bins, "nseg_max": total // seg + nb + 1 + (2048 + 4096 if flat else 0), "tstride": set_n if flat else 0,
            "c": window_widths(nwin)}


N_BIG = (1 << 18) + 1     # [tau^i]G, c = 19
N_QUAD = 513              # c = 11
N_SMALL = 300             # no table
N_MID = (1 << 15) + 3
TWIN_LO = 512             # the twin set: the 2 * N_MID points of the big set from here on, none of them the identity (c = 17)
ALL_PREDICATES = tuple(predicates({"SEG": 16, "big_nseg": 4, "log_g": 2}))
SMALL_RUNGS = ("1", "2", "SEG-1", "SEG", "SEG+1", "2SEG-1", "2SEG", "2SEG+1")
# job -> the set it runs on, its size and offset, the rungs its ladder holds — every rung of RUNGS that is NOT listed is dropped
# because the job has too few points for it — and the predicates its rungs therefore leave on one side
JOBS = {
    # (offsets 1: row 0 of the sets is an identity base in the GPU tests, and a job of one or two points has none to spare)
    "per_window_n1": {"set": "small", "n": 1, "offset": 1, "rungs": ("1",),
                      "one_sided": ALL_PREDICATES},
    "per_window_n2": {"set": "small", "n": 2, "offset": 1, "rungs": ("2",),
                      "one_sided": ALL_PREDICATES},
    # 300 points: the eight small rungs (291 rows) and the negative one; no room for any bucket of 16 segments (481 entries or more)
    "per_window_n300": {"set": "small", "n": 300, "offset": 0, "rungs": SMALL_RUNGS + ("negative",),
                        "one_sided": ("ns > FLAT_WIDE_NS", "ns > big_nseg", "ns > G", "ns >= G", "ns > 2G")},
    # 513 points, SEG = 32: the big_nseg line (128 and 129 entries) and the small rungs but 2 SEG
    "quad_513": {"set": "quad", "n": N_QUAD, "offset": 0,
                 "rungs": ("1", "2", "SEG-1", "SEG", "SEG+1", "2SEG-1", "2SEG+1", "ns=big", "ns=big+1,first+1", "negative"),
                 "one_sided": ("ns > FLAT_WIDE_NS", "ns > 2G")},
    "lat_2p15": {"set": "big", "n": N_MID, "offset": 0, "rungs": RUNGS, "one_sided": ()},
    "lat_2p15_offset": {"set": "big", "n": N_MID, "offset": 70001, "rungs": RUNGS, "one_sided": ()},
    "lat_65537": {"set": "big", "n": 65537, "offset": 0, "rungs": RUNGS, "one_sided": ()},
    "lat_190000": {"set": "big", "n": 190000, "offset": 0, "rungs": RUNGS, "one_sided": ()},
    "throughput": {"set": "big", "n": N_BIG, "offset": 0, "rungs": RUNGS, "one_sided": ()},
    "twin_lead": {"set": "twin", "n": N_MID, "offset": 0, "follow_offset": N_MID, "rungs": RUNGS, "one_sided": ()},
}
SET_SIZE = {"small": N_SMALL, "quad": N_QUAD, "big": N_BIG, "twin": 2 * N_MID}
# what the shape line of each job must read (SEG, big_nseg, G = 2^log_g, the regime): a tuning change fails here by name
REGIME = {
    "per_window_n1": {"flat": 0, "nwin": 26, "SEG": 32, "big_nseg": 16, "log_g": 8},
    "per_window_n2": {"flat": 0, "nwin": 26, "SEG": 32, "big_nseg": 16, "log_g": 8},
    "per_window_n300": {"flat": 0, "nwin": 26, "SEG": 32, "big_nseg": 16, "log_g": 8},
    "quad_513": {"flat": 1, "lat": 1, "quad": 1, "raw": 0, "nwin": 24, "SEG": 32, "big_nseg": 4, "log_g": 2},
    "lat_2p15": {"flat": 1, "lat": 1, "quad": 0, "raw": 1, "nwin": 14, "SEG": 16, "big_nseg": 4, "log_g": 2},
    "lat_2p15_offset": {"flat": 1, "lat": 1, "quad": 0, "raw": 1, "nwin": 14, "SEG": 16, "big_nseg": 4, "log_g": 2},
    "lat_65537": {"flat": 1, "lat": 1, "quad": 0, "raw": 1, "nwin": 14, "SEG": 16, "big_nseg": 6, "log_g": 2},
    "lat_190000": {"flat": 1, "lat": 1, "quad": 0, "raw": 1, "nwin": 14, "SEG": 32, "big_nseg": 6, "log_g": 2},
    "throughput": {"flat": 1, "lat": 0, "quad": 0, "raw": 1, "nwin": 14, "SEG": 128, "big_nseg": 16, "log_g": 8},
    "twin_lead": {"flat": 1, "lat": 1, "quad": 0, "raw": 1, "lead": 1, "nwin": 15, "SEG": 16, "big_nseg": 4, "log_g": 2},
}


def job_shape(name):
    j = JOBS[name]
    return predicted_shape(j["n"], SET_SIZE[j["set"]], lead="follow_offset" in j)

"""The ASYNCHRONOUS entry of the MSM (msm_enqueue with lane >= 0: what every commitment of a proof runs) against the CPU oracle,
through swm_selftest_msm_jobs, which enqueues one round of jobs the way commit_enqueue does.  test_gpu_msm_schedules.py covers
the synchronous entry; what only this entry reaches, and what each family of cases here pins:

  * twin pairs (msm.h: MsmTwin) — the lead's second sorted array through TwinOut::map, from bins that fit LDS and from OVERSIZED
    bins (the scattered branch of msm_flat_bin_sort), with every sign of (dstride, doff); the follower's copied descriptors
    (msm_twin_copy) when they describe many-segment buckets and big-list buckets; every fallback of msm_twin_match;
  * the joint bucket stage of deferred jobs (msm_flush_tails with k > 1), also with the quad form (16-bit tables);
  * the lanes: four single-stream lanes, the three-stream pipeline on two scratch sets (pipe_min = 1), the pair-owned
    msmT.sorted / msmT.segs buffers that consecutive pairs reuse.

Base sets: slices of ONE run of powers [tau^i]G, sized so that the default msm_table_width gives 17-bit tables (A17: 98304 points,
B17: 65536 from another start) and 16-bit ones (A16: 65535, B16: 49152: maxB = 32768, the quad bucket stage), plus a copy of B17
with one point replaced by the identity (it carries an infinity mask).  Sizes: 32767 .. 65538 points, the smallest at which the
twin path exists (twin_min = 32768).

Discipline, as in test_gpu_msm_schedules.py: every group of rounds runs in ONE child process under its own timeout; the child
holds the `msm shape:` line of every job against the geometry the case was built for (geometry() below models msm_shape) and
exits with "PRECONDITION ..." otherwise; the parent checks the bin occupancies the case is named after with the digit model
BEFORE it launches anything, and the (dstride, doff) signs its name claims.  References: the CPU oracle over the same slice of
the powers, or the closed form for equal scalars.  All comparisons are bit-exact on the affine point.

After a child that ended by a signal, with status 134 / 139 or at its timeout, no later test of this module starts another GPU
process (DEAD below): whatever faulted must not be run again before its cause is known."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from msm_sort_model import signed_digits, twin_map  # noqa: F401  (moved to the sort model; used and re-exported here)
from oracle_lib import Oracle, golden, h2i, ints_to_limbs, limbs_to_ints, R
from test_gpu_msm_schedules import FLAT_BIN_CAP, ROOT, Refs, buckets, equal, witness_mix

TWIN_MIN = 32768                     # msm_twin_match: jobs below keep their own sort
B_START = 4099                       # B17 / B16 start at this power of tau
SETS = {"A17": (0, 98304), "B17": (B_START, 65536), "A16": (0, 65535), "B16": (B_START, 49152), "B17h": (B_START, 65536)}
WIDTH = {"A17": 17, "B17": 17, "A16": 16, "B16": 16, "B17h": 17}
HOLE = 60000                         # the row of B17h that is the identity
N_POWERS = 98304
N_UNIFORM = 50021                    # one table, two offsets
N_SHORT = 40961                      # two tables: fits B16 at two offsets (32769 equal + 8192 uniform for the mixed vector)
N_EQUAL = TWIN_MIN + 1
N_CAP = {17: 65536, 16: 65000}       # the cap_edge vectors: ~31 000 small scalars in one bin, the rest uniform
CAP_BIN = 5
SWM_ERR_INVALID_ARG = -1
DEAD = []                            # why no further GPU process of this module is started


# ------------------------------------------------------------------------------------------------ models
def geometry(c, n):
    """msm_shape for a low-latency job of n points on a twisted Edwards table of width c (n < 262144): what the child holds every
    shape line against, and what the clustered vectors are placed with."""
    nwin = -(-254 // c)
    nb = 1 << (c - 1)
    total = n * nwin
    target = min(28000, max(1024, total // 1024))
    want = 64
    while want < 4096 and want * target < total:
        want <<= 1
    fb = 0
    while (nb >> fb) > want:
        fb += 1
    while (1 << fb) > 2048:
        fb -= 1
    return {"n": n, "flat": 1, "te": 1, "lat": 1, "c": c, "nwin": nwin, "flat_fb": fb, "flat_bins": (nb + (1 << fb) - 1) >> fb,
            "SEG": 32 if total // nb >= 10 else 16, "big_nseg": 4 if n < 65536 else 6}


def bin_counts(sc, g):
    """entries per coarse bin of the ONE bucket set all windows of a flat job share"""
    bk = buckets(sc, g["nwin"])
    return np.bincount(bk[bk >= 0] >> g["flat_fb"], minlength=g["flat_bins"])


def twin_deltas(lead, follow):
    """(dstride, doff) of a pair as plain integers; lead, follow: jobs (set, offset, vector, n, role)"""
    return SETS[follow[0]][1] - SETS[lead[0]][1], follow[1] - lead[1]


def sign(v):
    return "+" if v > 0 else "-" if v < 0 else "0"


def test_twin_map_model_against_plain_integers():
    """Entry (point i, window w, sign) of the lead is row w * stride_a + off_a + i; the follower's is w * stride_b + off_b + i with
    the same sign bit.  All four sign combinations of (dstride, doff) plus the zeros, the first and the last window, both values
    of bit 31, the first and the last point of the job."""
    seen = set()
    for (sa, oa), (sb, ob) in (((98304, 0), (98304, 65535)), ((98304, 65535), (98304, 0)),        # one table: dstride 0, doff + / -
                               ((98304, 0), (65536, 24575)), ((98304, 24575), (65536, 0)),        # dstride -, doff + / -
                               ((65536, 0), (98304, 57343)), ((65536, 24575), (98304, 0)),        # dstride +, doff + / -
                               ((98304, 1234), (65536, 1234)), ((65536, 1234), (98304, 1234)),
                               ((65535, 16382), (49152, 5)), ((49152, 8191), (65535, 24574))):
        for nwin, n in ((15, 40961), (16, 32769)):
            if oa + n > sa or ob + n > sb:
                n = min(sa - oa, sb - ob)
            ds, do = sb - sa, ob - oa
            seen.add((sign(ds), sign(do)))
            i = np.array([0, 1, n // 2, n - 1], dtype=np.int64)
            for w in (0, 1, nwin - 1):
                for neg in (0, 1):
                    row_a = w * sa + oa + i
                    row_b = w * sb + ob + i
                    assert row_a.max() < 1 << 31 and row_b.max() < 1 << 31
                    e = (row_a | (neg << 31)).astype(np.uint32)
                    got = twin_map(e, sa, ds % (1 << 32), do % (1 << 32))
                    assert got.dtype == np.uint32 and [int(v) for v in got] == [int(r) | (neg << 31) for r in row_b], (sa, oa, sb, ob, w, neg)
    assert seen >= {(a, b) for a in "+-" for b in "+-"} | {("0", "+"), ("0", "-"), ("+", "0"), ("-", "0")}


# ------------------------------------------------------------------------------------------------ scalar vectors
def one_bucket_scalar(c):
    """the scalar whose every digit is +1 on the layout of a width-c table"""
    nwin = -(-254 // c)
    base, extra = divmod(254, nwin)
    s, bit = 0, 0
    for w in range(nwin):
        s |= 1 << bit
        bit += base + (1 if w < extra else 0)
    return s


def interleave(a, b):
    """a and b merged with the rows of b spread evenly"""
    n = len(a) + len(b)
    at_b = (np.arange(len(b), dtype=np.int64) * n) // len(b) + (n // len(b)) // 2
    mask = np.zeros(n, dtype=bool)
    mask[at_b] = True
    out = np.empty((n, 4), dtype=np.uint64)
    out[mask] = b
    out[~mask] = a
    return out


def cap_edge(c, uniform):
    """(at, over): N_CAP[c] scalars with exactly FLAT_BIN_CAP and FLAT_BIN_CAP + 1 entries in coarse bin CAP_BIN — uniform scalars
    without an entry in that bin are replaced by small ones (window 0 only) whose bucket lies in it, one entry each — as
    test_per_window_bin_at_and_above_bin_cap builds its inputs."""
    n = N_CAP[c]
    g = geometry(c, n)
    fb = g["flat_fb"]
    sc = uniform[:n].copy()
    hits = ((buckets(sc, g["nwin"]) >> fb) == CAP_BIN).sum(axis=0)
    need = FLAT_BIN_CAP + 1 - int(hits.sum())
    move = np.flatnonzero(hits == 0)[:need]
    assert need > 0 and len(move) == need
    sc[move] = 0
    sc[move, 0] = ((CAP_BIN << fb) + 1 + (np.arange(need, dtype=np.uint64) * np.uint64(37)) % np.uint64(1 << fb)).astype(np.uint64)
    at = sc.copy()
    at[move[-1]] = uniform[move[-1]]     # one entry fewer
    return at, sc


def all_but_top_negative(c):
    """the scalar whose digits are -1 in every window but the top one (+1) on the layout of a width-c table"""
    nwin = -(-254 // c)
    base, extra = divmod(254, nwin)
    bits, bit = [], 0
    for w in range(nwin):
        bits.append(bit)
        bit += base + (1 if w < extra else 0)
    return (1 << bits[-1]) - sum(1 << b for b in bits[:-1])


def signs_small(c, i):
    return 1 + (i * 7919) % ((1 << (c - 1)) - 1)


def signs_vector(c, n=36001):
    """rows i = 0 mod 5: a small scalar v (one positive digit in window 0); 1: r - 1; 2: r - 2; 3: r - (v + 1), whose window-0 digit
    is -v (r = 1 mod 2^47): the bucket of v, reached by a negative digit; 4: the scalar with the digit -1 in every window but the
    top one — 14 or 15 negative entries of bucket 0 per row."""
    vals = [(signs_small(c, i), R - 1, R - 2, R - (signs_small(c, i) + 1), all_but_top_negative(c))[i % 5] for i in range(n)]
    return ints_to_limbs(vals, 4)


class Vectors:
    """The scalar vectors by name, standard form, built once; `check` asserts the precondition a vector is named after from the
    digit model — bin occupancies for the table width it is used on."""

    def __init__(self):
        from pyref.prng import fr_array
        self.uniform = fr_array(66000, 2901)
        self.eq_s = limbs_to_ints(self.uniform[7:8])[0]     # a uniform scalar: no window's digit is zero (checked)
        u = self.uniform
        self.v = {
            "uniform": u[:N_UNIFORM], "uniform_short": u[:N_SHORT], "other_short": fr_array(N_SHORT, 2902), "below_min": u[:TWIN_MIN - 1],
            "small_job": u[:20011], "mid_job": u[:45007],
            "equal": equal(self.eq_s, N_EQUAL),
            "mixed": interleave(equal(self.eq_s, N_EQUAL), u[:N_EQUAL]),
            "mixed_short": interleave(equal(self.eq_s, N_EQUAL), u[:N_SHORT - N_EQUAL]),
            "witness": witness_mix(40001),
        }
        for c in (17, 16):
            self.v["one_bucket%d" % c] = equal(one_bucket_scalar(c), TWIN_MIN)
            self.v["cap_at%d" % c], self.v["cap_over%d" % c] = cap_edge(c, u)
            self.v["signs%d" % c] = signs_vector(c)
        self.closed = {"equal": self.eq_s, "one_bucket17": one_bucket_scalar(17), "one_bucket16": one_bucket_scalar(16)}
        self.checked = {}

    def kinds(self, c):
        """the vectors of case 1 for a table of width c"""
        return ["uniform", "equal", "one_bucket%d" % c, self.mixed(c), "cap_at%d" % c, "cap_over%d" % c, "witness", "signs%d" % c]

    def mixed(self, c):
        """32769 equal and 32769 uniform scalars; on the 16-bit sets (65535 points) 32769 equal and 8192 uniform ones"""
        return "mixed" if c == 17 else "mixed_short"

    def check(self, name, c):
        if (name, c) not in self.checked:
            self.checked[name, c] = self.check_now(name, c)
        return self.checked[name, c]

    def check_now(self, name, c):
        sc = self.v[name]
        g = geometry(c, sc.shape[0])
        cnt = bin_counts(sc, g)
        used = cnt[cnt > 0]
        kind = name.rstrip("0123456789")
        msg = "PRECONDITION %s on c = %d: bin occupancies (max %d, bins used %d) in %r" % (name, c, cnt.max(), len(used), g)
        if kind in ("uniform", "uniform_short", "other_short", "below_min", "small_job", "mid_job"):
            assert cnt.max() <= FLAT_BIN_CAP // 4, msg
        elif kind == "equal":        # every window one bucket of n entries: every bin that holds entries is oversized
            d = signed_digits(sc[:1], g["nwin"])[:, 0]
            assert (d != 0).all() and used.min() > FLAT_BIN_CAP and sc.shape[0] == FLAT_BIN_CAP + 1, msg
        elif kind == "one_bucket":   # all n * nwin entries in bucket 0, which also goes on the big list
            bk = buckets(sc, g["nwin"])
            assert (bk == 0).all() and cnt[0] == sc.shape[0] * g["nwin"] > FLAT_BIN_CAP, msg
            assert -(-int(cnt[0]) // g["SEG"]) > g["big_nseg"], msg
        elif kind in ("mixed", "mixed_short"):   # oversized and ordinary bins in one job
            assert (used > FLAT_BIN_CAP).sum() >= 2 and ((used <= FLAT_BIN_CAP) & (used > 32)).sum() >= g["flat_bins"] // 2, msg
        elif kind in ("cap_at", "cap_over"):
            assert cnt[CAP_BIN] == FLAT_BIN_CAP + (kind == "cap_over") and np.delete(cnt, CAP_BIN).max() < FLAT_BIN_CAP // 4, msg
        elif kind == "witness":      # a quarter of the scalars is 1: bucket 0 alone holds 10 000 entries, in a bin that fits LDS
            assert FLAT_BIN_CAP >= cnt[0] >= sc.shape[0] // 4 and cnt.max() == cnt[0], msg
        elif kind == "signs":        # the sign bit has to survive map: over a third of the entries are negative, also in an oversized bin
            d = signed_digits(sc, g["nwin"])
            rows = np.arange(sc.shape[0])
            small = np.array([signs_small(c, int(i)) for i in rows])
            assert (d[:, rows % 5 == 0] >= 0).all() and (d[0, rows % 5 == 0] == small[rows % 5 == 0]).all(), msg
            assert ((d[:, rows % 5 == 1] < 0).sum(axis=0) >= 1).all() and ((d[:, rows % 5 == 2] < 0).sum(axis=0) >= 1).all(), msg
            assert (d[0, rows % 5 == 3] == -small[rows % 5 == 3]).all(), msg
            assert (d[:-1, rows % 5 == 4] == -1).all() and (d[-1, rows % 5 == 4] == 1).all(), msg
            assert 3 * (d < 0).sum() > (d != 0).sum() and cnt[0] > FLAT_BIN_CAP, msg
        else:
            raise AssertionError("no precondition for " + name)
        return g


@pytest.fixture(scope="module")
def vecs():
    return Vectors()


def test_scalar_vectors_meet_their_preconditions(vecs):
    """No device: every clustered vector puts its entries where its name says, by the digit model, on the width it is used with;
    the model of the digits with signs agrees with buckets() of the sibling module."""
    for c in (17, 16):
        for name in set(vecs.kinds(c) + ["uniform_short", "other_short", "mixed_short", "below_min", "small_job", "mid_job"]):
            assert vecs.check(name, c)["c"] == c
        sc = vecs.v["signs%d" % c][:2000]
        nwin = geometry(c, 2000)["nwin"]
        assert (np.abs(signed_digits(sc, nwin)) - 1 == buckets(sc, nwin)).all()
    # the two cap_edge variants differ in ONE scalar, and sit on the two sides of the LDS / scattered branch
    for c in (17, 16):
        at, over = vecs.v["cap_at%d" % c], vecs.v["cap_over%d" % c]
        assert (at != over).any(axis=1).sum() == 1


# ------------------------------------------------------------------------------------------------ references
class AsyncRefs(Refs):
    """Refs of the sibling module over the N_POWERS powers this module needs (none of its 393 217-point references); every
    reference is computed once per (vector, n, range of the powers)."""

    def __init__(self, tmp):
        self.orc = orc = Oracle()
        self.threads = orc.lib.oracle_max_threads()
        self.tmp = tmp
        self.tau = h2i(golden("msm.json")["tau"])
        self.G = orc.points_to_mont([tuple(h2i(v) for v in golden("g1.json")["generator"])])
        self.bases = orc.srs_bases(N_POWERS, self.tau, self.G)
        self.bases_path = os.path.join(tmp, "bases.npy")
        np.save(self.bases_path, self.bases)
        self.cache = {}
        self.saved = {}

    def geometric_at(self, s, n, off):
        """[s tau^off (tau^n - 1) / (tau - 1)]G: n equal scalars over the powers off .. off + n"""
        geo = pow(self.tau, off, R) * (pow(self.tau, n, R) - 1) * pow(self.tau - 1, -1, R)
        pt = self.orc.fixed_base_mul(self.G, ints_to_limbs([s * geo % R], 4), threads=1)
        return self.orc.points_from_mont(np.ascontiguousarray(pt.reshape(1, 12)))[0]

    def want(self, vecs, job):
        """the affine reference of job (set, offset, vector, n, role)"""
        set_name, off, name, n = job[:4]
        start, size = SETS[set_name]
        assert off + n <= size and start + off + n <= N_POWERS
        hole = set_name == "B17h" and off <= HOLE < off + n
        key = (name, n, start + off, hole)
        if key not in self.cache:
            sc = vecs.v[name][:n]
            if name in vecs.closed and not hole:
                self.cache[key] = self.geometric_at(vecs.closed[name], n, start + off)
            else:
                jac = self.msm(sc, start + off)
                if hole:   # the identity row contributes nothing
                    jac = self.add(jac, self.sparse([start + HOLE], [-limbs_to_ints(sc[HOLE - off:HOLE - off + 1])[0]]))
                self.cache[key] = self.affine(jac)
        return self.cache[key]

    def vector_path(self, vecs, name, mont):
        key = (name, mont)
        if key not in self.saved:
            sc = np.ascontiguousarray(vecs.v[name], dtype=np.uint64)
            self.saved[key] = os.path.join(self.tmp, "%s%s.npy" % (name, "_mont" if mont else ""))
            np.save(self.saved[key], self.orc.fr_to_mont(sc) if mont else sc)
        return self.saved[key]


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return AsyncRefs(str(tmp_path_factory.mktemp("msm_async")))


def test_closed_form_with_an_offset(vecs):
    """No device: the closed form for equal scalars over a sub-range of the powers against the oracle MSM (small range)."""
    import types
    orc = Oracle()
    r = types.SimpleNamespace(orc=orc, tau=h2i(golden("msm.json")["tau"]), threads=1)
    r.G = orc.points_to_mont([tuple(h2i(v) for v in golden("g1.json")["generator"])])
    r.bases = orc.srs_bases(64, r.tau, r.G)
    for off, n in ((0, 64), (5, 59), (63, 1)):
        want = orc.jac_to_affine_int(Refs.msm(r, equal(vecs.eq_s, n), off))
        assert AsyncRefs.geometric_at(r, vecs.eq_s, n, off) == want


# ------------------------------------------------------------------------------------------------ child process
CHILD = r"""
import json, os, sys, tempfile
spec = json.load(open(sys.argv[1]))
sys.path.insert(0, spec["root"])
import numpy as np
real_err = os.dup(2)
log = tempfile.TemporaryFile()
os.dup2(log.fileno(), 2)       # the library's trace lines: read back round by round
def trace_lines(pos):
    log.seek(pos)
    return log.read().decode(errors="replace").splitlines()
try:
    import simpleworks_amd as swm
    ctx = swm.Context(0)
    powers = np.load(spec["bases"], mmap_mode="r")
    handles = []
    for s in spec["sets"]:
        b = powers[s["start"]:s["start"] + s["n"]].copy()
        if s["hole"] is not None:
            b[s["hole"]] = 0
        handles.append(ctx.srs_upload(b))
    vectors = {}
    for rnd in spec["rounds"]:
        for p in rnd["vectors"]:
            if p not in vectors:
                vectors[p] = np.load(p)
        pos = log.seek(0, 2)
        rec = {"name": rnd["name"], "error": None, "twins": None, "points": [], "shapes": []}
        try:
            jacs, twins = ctx.selftest_msm_jobs(handles, [vectors[p] for p in rnd["vectors"]], [tuple(j) for j in rnd["jobs"]],
                                                montgomery=rnd["mont"], defer_tail=rnd["defer"], pipe_min=rnd["pipe_min"])
        except swm.SwmError as e:
            if not rnd["expect_error"]:
                raise
            rec["error"] = e.code
            print("ROUND " + json.dumps(rec), flush=True)
            continue
        lines = [l for l in trace_lines(pos) if "msm shape:" in l]
        assert len(lines) == len(rnd["jobs"]), "PRECONDITION %s: expected one shape line per job, got %r" % (rnd["name"], lines)
        for line, want in zip(lines, rnd["expect"]):
            shape = {k: int(v) for k, v in (f.split("=") for f in line.split("msm shape:")[1].split())}
            wrong = {k: (v, shape.get(k)) for k, v in want.items() if shape.get(k) != v}
            if wrong:
                raise SystemExit("PRECONDITION %s: a job ran another schedule than the case was built for: (wanted, got) %r in %r"
                                 % (rnd["name"], wrong, shape))
            rec["shapes"].append(line.split("msm shape:")[1].strip())
        for jac in jacs:
            xy, inf = ctx.g1_normalize(jac)
            rec["points"].append(None if inf else [int(v) for v in xy])
        rec["twins"] = twins
        print("ROUND " + json.dumps(rec), flush=True)
    for h in handles:
        h.free()
    ctx.close()
finally:
    os.dup2(real_err, 2)
    sys.stderr.write("\n".join(trace_lines(0)[-40:]) + "\n")
"""


def prepare(refs, vecs, set_names, rounds):
    """What is checked BEFORE a launch: every job's range lies inside its set, every pair's (dstride, doff) has the signs the round
    claims (`claim`), the preconditions of the vectors hold on the width they are used with.  Returns the rounds as the child
    reads them, each job with the shape line it has to print."""
    assert len(set_names) <= 2, "a child uploads at most two tables"
    listed = []
    for r in rounds:
        names = sorted({j[2] for j in r["jobs"]})
        mont = bool(r.get("mont", False))
        expect = []
        for j in r["jobs"]:
            c = WIDTH[j[0]]
            if not r.get("expect_error"):
                assert j[1] + j[3] <= SETS[j[0]][1], (r["name"], j)
            vecs.check(j[2], c)
            expect.append(geometry(c, j[3]))
        pairs = [twin_deltas(a, b) for a, b in zip(r["jobs"], r["jobs"][1:]) if a[4] == "lead" and b[4] == "follow"]
        assert [(sign(ds), sign(do)) for ds, do in pairs] == list(r.get("claim", [])), "PRECONDITION %s: (dstride, doff) %r" % (r["name"], pairs)
        listed.append({"name": r["name"], "vectors": [refs.vector_path(vecs, v, mont) for v in names], "mont": mont,
                       "jobs": [[set_names.index(j[0]), j[1], names.index(j[2]), j[3], j[4]] for j in r["jobs"]],
                       "defer": r.get("defer", "prover"), "pipe_min": int(r.get("pipe_min", 0)), "expect": expect,
                       "expect_error": bool(r.get("expect_error", False))})
    return listed


def run_rounds(refs, vecs, set_names, rounds, env_extra=None, timeout=180):
    """One child process: uploads the sets, runs the rounds (dicts: name, jobs [(set, offset, vector, n, role)], claim, twins,
    optional mont, defer, pipe_min, expect_error), returns {name: record}."""
    if DEAD:
        pytest.fail("no GPU process started: %s — its cause has to be found first" % DEAD[0])
    listed = prepare(refs, vecs, set_names, rounds)
    tag = "%s_%d" % (rounds[0]["name"], len(os.listdir(refs.tmp)))
    path = os.path.join(refs.tmp, tag + "_spec.json")
    sets = [{"name": s, "start": SETS[s][0], "n": SETS[s][1], "hole": HOLE if s == "B17h" else None} for s in set_names]
    with open(path, "w") as f:
        json.dump({"root": ROOT, "bases": refs.bases_path, "sets": sets, "rounds": listed}, f)
    env = dict(os.environ)
    env.update(env_extra or {})
    env["SWM_TRACE"] = "1"
    try:
        out = subprocess.run([sys.executable, "-c", CHILD, path], env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        DEAD.append("the child of %s did not end within %d s" % (tag, timeout))
        pytest.fail(DEAD[0] + ": " + str(e.stdout)[-2000:])
    if out.returncode < 0 or out.returncode in (134, 139):
        DEAD.append("the child of %s ended with status %d" % (tag, out.returncode))
    assert out.returncode == 0, "status %d\n" % out.returncode + out.stdout[-2000:] + out.stderr[-4000:]
    recs = [json.loads(l[6:]) for l in out.stdout.splitlines() if l.startswith("ROUND ")]
    assert [r["name"] for r in recs] == [r["name"] for r in rounds], out.stdout[-2000:] + out.stderr[-4000:]
    for rec in recs:   # (every case prints its shape lines and twins count: pytest -s shows them)
        print("%s: twins=%s" % (rec["name"], rec["twins"]))
        for s in rec["shapes"]:
            print("    msm shape: " + s)
    return {r["name"]: r for r in recs}


def check_rounds(refs, vecs, rounds, recs):
    """twins count and every job's point of every round against its reference"""
    for r in rounds:
        rec = recs[r["name"]]
        assert rec["twins"] == r["twins"], "%s: %d jobs took a twin's sort, %d expected" % (r["name"], rec["twins"], r["twins"])
        for i, j in enumerate(r["jobs"]):
            xy = rec["points"][i]
            got = None if xy is None else refs.orc.points_from_mont(np.array(xy, dtype=np.uint64).reshape(1, 12))[0]
            assert got == refs.want(vecs, j), "%s: job %d %r" % (r["name"], i, j)


def pair(lead_set, lead_off, follow_set, follow_off, vec, n, follow_vec=None):
    return [(lead_set, lead_off, vec, n, "lead"), (follow_set, follow_off, follow_vec or vec, n, "follow")]


# ------------------------------------------------------------------------------------------------ cases that take the twin path
def one_table_rounds(vecs, fam, kinds=None, **knobs):
    """Case 1: lead at offset 0 and follower at |set| - n (doff > 0: the prover's situation), then the offsets swapped (doff < 0)."""
    a, c = "A%d" % fam, fam
    rounds = []
    for kind in kinds or vecs.kinds(c):
        n = vecs.v[kind].shape[0]
        hi = SETS[a][1] - n
        assert hi > 0
        rounds.append(dict(knobs, name="%s_%s_doff+" % (a, kind), jobs=pair(a, 0, a, hi, kind, n), claim=[("0", "+")], twins=1))
        rounds.append(dict(knobs, name="%s_%s_doff-" % (a, kind), jobs=pair(a, hi, a, 0, kind, n), claim=[("0", "-")], twins=1))
    return rounds


def several_pairs_rounds(vecs, fam, **knobs):
    """Case 3: two (three) pairs with different vectors in one round — the first `equal`, the second `uniform` (the third `witness`)."""
    a = "A%d" % fam
    jobs = []
    for kind in ("equal", "uniform", "witness"):
        n = vecs.v[kind].shape[0]
        jobs.append(pair(a, 0, a, SETS[a][1] - n, kind, n))
    return [dict(knobs, name="%s_two_pairs" % a, jobs=jobs[0] + jobs[1], claim=[("0", "+")] * 2, twins=2),
            dict(knobs, name="%s_three_pairs" % a, jobs=jobs[0] + jobs[1] + jobs[2], claim=[("0", "+")] * 3, twins=3)]


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [17, 16])
def test_one_table_two_offsets(refs, vecs, fam):
    """Case 1 on A17 and on A16 (quad bucket stage): uniform, equal (every bin oversized: the scattered branch of TwinOut::map),
    one_bucket (the follower's copied big list), mixed, cap_edge at and above FLAT_BIN_CAP, witness, signs — each with the follower
    above and below the lead.  Default knobs: the prover's rule defers both bucket stages to one joint launch."""
    rounds = one_table_rounds(vecs, fam)
    check_rounds(refs, vecs, rounds, run_rounds(refs, vecs, ["A%d" % fam], rounds))


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [17, 16])
def test_two_tables(refs, vecs, fam):
    """Case 2: lead on the wider table and follower on the narrower one (dstride < 0) and the reverse (dstride > 0), each with equal
    offsets (doff = 0) and with the follower above (doff > 0) and below (doff < 0) the lead: every sign combination of
    TwinOut::map, over uniform, equal and mixed scalars."""
    a, b = "A%d" % fam, "B%d" % fam
    rounds = []
    for kind in ("uniform_short", "equal", "mixed_short"):
        n = vecs.v[kind].shape[0]
        for lead, follow in ((a, b), (b, a)):
            ds = sign(SETS[follow][1] - SETS[lead][1])
            assert ds == ("-" if lead == a else "+")
            hi_l, hi_f = SETS[lead][1] - n, SETS[follow][1] - n
            for tag, lo, fo in (("0", 1234, 1234), ("+", 0, hi_f), ("-", hi_l, 0)):
                rounds.append({"name": "%s_%s_%s_doff%s" % (lead, follow, kind, tag), "jobs": pair(lead, lo, follow, fo, kind, n),
                               "claim": [(ds, tag)], "twins": 1})
    check_rounds(refs, vecs, rounds, run_rounds(refs, vecs, [a, b], rounds))


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [17, 16])
def test_pairs_share_a_round(refs, vecs, fam):
    """Case 3: the second (third) pair of a round reuses msmT.sorted / msmT.segs after the first follower's accumulation; the first
    pair's scalars are `equal`, the next `uniform`, so an array left over from the first pair gives the second a wrong point.  This
    holds the ordering between the pairs only as far as a wrong result shows it: a race that happens to go the right way passes.
    Case 4: a pair between two unrelated jobs, one below twin_min — the lane the follower hands back."""
    a = "A%d" % fam
    rounds = several_pairs_rounds(vecs, fam)
    mixed = vecs.mixed(fam)
    n = vecs.v[mixed].shape[0]
    inside = [(a, 5, "small_job", 20011, None)] + pair(a, 0, a, SETS[a][1] - n, mixed, n) + [(a, 77, "mid_job", 45007, None)]
    rounds.append({"name": "%s_pair_inside" % a, "jobs": inside, "claim": [("0", "+")], "twins": 1})
    check_rounds(refs, vecs, rounds, run_rounds(refs, vecs, [a], rounds))


KNOBS = (("defer_on", {"defer": "on"}), ("defer_off", {"defer": "off"}), ("pipe", {"defer": "off", "pipe_min": 1}),
         ("pipe_joint_mont", {"defer": "prover", "pipe_min": 1, "mont": True}))


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [17, 16])
def test_knobs_of_the_prover(refs, vecs, fam):
    """Case 5: cases 1 and 3 with every bucket stage in the round's joint launch (k = 2, 4 and 4 + 2 jobs per flush, an `equal` job
    beside a `uniform` one), with every job's own bucket stage, and on the three-stream pipeline with its two scratch sets
    (pipe_min = 1; three_pairs has three jobs that sort, so a set is reused) — own bucket stages, then joint ones with
    Montgomery-form device scalars."""
    a = "A%d" % fam
    rounds = []
    for tag, knobs in KNOBS:
        for r in one_table_rounds(vecs, fam, **knobs) + several_pairs_rounds(vecs, fam, **knobs):
            rounds.append(dict(r, name=tag + "_" + r["name"]))
    check_rounds(refs, vecs, rounds, run_rounds(refs, vecs, [a], rounds))


# ------------------------------------------------------------------------------------------------ cases that must NOT take it
@pytest.mark.gpu
def test_fallbacks_below_twin_min_and_on_other_widths(refs, vecs):
    """n = 32767 on either width, and a lead on A17 with its follower on A16: msm_twin_match refuses (the lead's second array is
    not even written for another width), every job sorts for itself, the points are right."""
    n = TWIN_MIN - 1
    rounds = [{"name": "%s_below_min" % a, "jobs": pair(a, 0, a, SETS[a][1] - n, "below_min", n), "claim": [("0", "+")], "twins": 0}
              for a in ("A17", "A16")]
    n = vecs.v["uniform"].shape[0]
    rounds.append({"name": "widths_differ", "jobs": pair("A17", 0, "A16", SETS["A16"][1] - n, "uniform", n), "claim": [("-", "+")], "twins": 0})
    rounds.append({"name": "widths_differ_equal", "jobs": pair("A16", 0, "A17", 1, "equal", N_EQUAL), "claim": [("+", "+")], "twins": 0})
    check_rounds(refs, vecs, rounds, run_rounds(refs, vecs, ["A17", "A16"], rounds))


@pytest.mark.gpu
def test_fallbacks_on_masks_vectors_and_ranges(refs, vecs):
    """The follower's set carries an infinity mask (the identity row outside the follower's range, then inside: the reference skips
    it); the lead's set carries it; the follower names another vector of the same length (the lead's second array goes unused,
    and the NEXT pair of the round still twins); a pair whose follower range does not fit its set, a FOLLOW with no job before it
    and a LEAD with no job after it are refused as argument errors, and the context works afterwards."""
    n = N_SHORT
    below, inside = 0, SETS["B17h"][1] - n
    assert below + n <= HOLE and inside <= HOLE < inside + n
    rounds = [
        {"name": "hole_outside", "jobs": pair("A17", 0, "B17h", below, "uniform_short", n), "claim": [("-", "0")], "twins": 0},
        {"name": "hole_inside", "jobs": pair("A17", 0, "B17h", inside, "uniform_short", n), "claim": [("-", "+")], "twins": 0},
        {"name": "hole_inside_equal", "jobs": pair("A17", 0, "B17h", SETS["B17h"][1] - N_EQUAL, "equal", N_EQUAL), "claim": [("-", "+")], "twins": 0},
        {"name": "hole_in_lead", "jobs": pair("B17h", inside, "A17", 0, "mixed_short", n), "claim": [("+", "-")], "twins": 0},
        {"name": "other_vector", "jobs": pair("A17", 0, "A17", SETS["A17"][1] - n, "uniform_short", n, follow_vec="other_short")
         + pair("A17", 3, "A17", 4, "mixed_short", n), "claim": [("0", "+")] * 2, "twins": 1},
        {"name": "range_does_not_fit", "jobs": pair("A17", 0, "A17", SETS["A17"][1] - n + 1, "uniform_short", n), "claim": [("0", "+")],
         "expect_error": True, "twins": None},
        {"name": "follow_without_a_lead", "jobs": [("A17", 0, "uniform_short", n, "follow")], "expect_error": True, "twins": None},
        {"name": "lead_without_a_follower", "jobs": [("A17", 0, "uniform_short", n, None), ("A17", 0, "uniform_short", n, "lead")],
         "expect_error": True, "twins": None},
        {"name": "after_the_errors", "jobs": pair("A17", 0, "A17", SETS["A17"][1] - n, "uniform_short", n), "claim": [("0", "+")], "twins": 1},
    ]
    recs = run_rounds(refs, vecs, ["A17", "B17h"], rounds)
    for name in ("range_does_not_fit", "follow_without_a_lead", "lead_without_a_follower"):
        assert recs[name]["error"] == SWM_ERR_INVALID_ARG, name
    ok = [r for r in rounds if not r.get("expect_error")]
    check_rounds(refs, vecs, ok, recs)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [17, 16])
def test_twin_switch_off(refs, vecs, fam):
    """SWM_MSM_TWIN=0 in the child's environment: the whole of case 1 on `equal` and `mixed` with no job taking a twin's sort, the
    same points as the default run and as the reference."""
    a = "A%d" % fam
    on = one_table_rounds(vecs, fam, kinds=("equal", vecs.mixed(fam)))
    off = [dict(r, twins=0) for r in on]
    recs_on = run_rounds(refs, vecs, [a], on)
    recs_off = run_rounds(refs, vecs, [a], off, env_extra={"SWM_MSM_TWIN": "0"})
    check_rounds(refs, vecs, on, recs_on)
    check_rounds(refs, vecs, off, recs_off)
    for r in on:
        assert recs_on[r["name"]]["points"] == recs_off[r["name"]]["points"], r["name"]

"""The MSM schedules that swm_srs_upload no longer hands to the K1 tests of test_gpu_kernels.py (every set of 512 points or more gets
a twisted Edwards table there, so those tests run the flat schedule on TE rows), each at the sizes it serves and each held to the
schedule it names:

  * the per-window schedule (SWM_MSM_NO_TABLE=1: what a set runs whose table could not be allocated) around its thresholds: the
    two-level sort (msm_bin_check, msm_partition, msm_bin_sort, with the per-window fallback into msm_scatter) from n = 262144, the
    c = 14 and c = 16 plans of msm_plan, ragged partition and sort tiles, the top window's bin plan;
  * the flat schedule on XYZZ rows (SWM_MSM_TE=0) in its throughput variant (n >= 262144);
  * the branches of msm_flat_bin_sort that depend on how the scalars cluster: more than FLAT_WIDE_Q many-segment buckets in one
    bin, with the bin placed in LDS and in HBM, and more than 1024 coarse bins (msm_flat_scan_bins<4>).

The switches are read once per process, so every schedule runs in a child process (one at a time, each with a timeout).  The
parent builds ONE base set ([tau^i]G, the tau of tests/golden/msm.json) and every reference with the CPU oracle (or the closed form
[s (tau^n - 1) / (tau - 1)]G for equal scalars); the child returns the affine result of each call, the `msm shape` line SWM_TRACE
printed for it and the kernels the profile saw.  EVERY case asserts its precondition first — the child holds the shape line of the
call against what the case claims to test and exits with "PRECONDITION ..." otherwise, the parent checks the launched kernels — so a
tuning change that moves a case onto another path fails here with that message instead of passing there.  All comparisons are
bit-exact on the affine point.

Known and NOT covered, because no small shape reaches them:
  * the 4096-bin / 8 K-tile form of msm_flat_partition (more than 57 M digits);
  * the `ns >= 2^24` clause of flat_seg_write.
(The second sorted array of a twin pair written from an oversized bin, and everything else only the asynchronous entry reaches, is
covered by tests/test_gpu_msm_async.py.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from msm_sort_model import buckets  # noqa: F401  (the digit model lives there; this module and its importers use it from here)
from oracle_lib import Oracle, golden, h2i, ints_to_limbs, limbs_to_ints, p64, R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_BASES = 393217                     # the first size on the c = 16 plan of msm_plan: the largest MSM below
N_RAGGED = 262144 + 8192 * 3 + 1     # last partition tile: one digit; last 65536-digit sort tile: not full
CUTS = (0, 100003, 131072, 262143, 262144, 262145, N_RAGGED, N_BASES)   # the uniform reference is computed per chunk
# constants of csrc/msm_sort.hip and csrc/msm_stages.h that the preconditions are stated in
BIN_CAP, FLAT_BIN_CAP, FLAT_WIDE_NS, FLAT_WIDE_Q = 24576, 32768, 16, 32
TWO_LEVEL_KERNELS = ("msm_bin_check", "msm_partition", "msm_bin_sort")
PER_WINDOW_KERNELS = ("msm_hist", "msm_scatter", "msm_accumulate", "msm_big_bucket_sum", "msm_bucket_reduce")
FLAT_KERNELS = ("msm_flat_hist", "msm_flat_partition", "msm_flat_bin_sort", "msm_accumulate", "msm_big_bucket_sum", "msm_bucket_reduce")
BIG253 = (1 << 252) | 0xDEADBEEFCAFEBABE1234567

CHILD = r"""
import json, os, sys, tempfile
spec = json.load(open(sys.argv[1]))
sys.path.insert(0, spec["root"])
import numpy as np
real_err = os.dup(2)
log = tempfile.TemporaryFile()
os.dup2(log.fileno(), 2)       # the library's trace lines: read back call by call
def trace_lines(pos):
    log.seek(pos)
    return log.read().decode(errors="replace").splitlines()
try:
    import simpleworks_amd as swm
    ctx = swm.Context(0)
    bases = np.load(spec["bases"], mmap_mode="r")[:spec["nbases"]].copy()
    if spec["holes"]:
        bases[spec["holes"]] = 0
    bh = ctx.srs_upload(bases)
    ctx.profile_enable(True)
    for case in spec["cases"]:
        sc = np.load(case["scalars"])
        n = sc.shape[0]
        ctx.profile_reset()
        pos = log.seek(0, 2)
        if case["dev_mont"]:     # the scalars are in Montgomery form already, resident on the device
            d = ctx.to_device(sc)
            jac = ctx.msm_g1_dev(bh, d, n, True, offset=case["offset"])
            d.free()
        else:
            jac = ctx.msm_g1(bh, sc, offset=case["offset"])
        lines = [l for l in trace_lines(pos) if "msm shape:" in l]
        assert len(lines) == 1, "PRECONDITION %s: expected one shape line, got %r" % (case["name"], lines)
        shape = {k: int(v) for k, v in (f.split("=") for f in lines[0].split("msm shape:")[1].split())}
        wrong = {k: (v, shape.get(k)) for k, v in case["expect"].items() if shape.get(k) != v}
        wrong.update({k: (">= %d" % v, shape.get(k)) for k, v in case["at_least"].items() if not shape.get(k, -1) >= v})
        if shape["n"] != n or wrong:
            raise SystemExit("PRECONDITION %s: the call ran another schedule than the case names: (wanted, got) %r in %r"
                             % (case["name"], wrong, shape))
        xy, inf = ctx.g1_normalize(jac)
        kernels = sorted(k for k, v in ctx.profile().items() if v["calls"] > 0)
        print("CASE " + json.dumps({"name": case["name"], "shape": shape, "inf": bool(inf), "xy": [int(v) for v in xy],
                                    "kernels": kernels}), flush=True)
    bh.free()
    ctx.close()
finally:
    os.dup2(real_err, 2)
    sys.stderr.write("\n".join(trace_lines(0)[-40:]) + "\n")
"""


def run_child(tmp, bases_path, nbases, env_extra, cases, holes=(), timeout=180):
    """One child process under env_extra + SWM_TRACE; cases: dicts with name, scalars (array), offset, dev_mont, expect, at_least.
    Returns {name: record}; the child has already held every call's shape line against expect / at_least."""
    tag = "%s_%d" % (cases[0]["name"], len(os.listdir(tmp)))
    listed = []
    for c in cases:
        path = os.path.join(tmp, "%s_%s.npy" % (tag, c["name"]))
        np.save(path, np.ascontiguousarray(c["scalars"], dtype=np.uint64))
        listed.append({"name": c["name"], "scalars": path, "offset": int(c.get("offset", 0)), "dev_mont": bool(c.get("dev_mont", False)),
                       "expect": c["expect"], "at_least": c.get("at_least", {})})
    spec = os.path.join(tmp, tag + "_spec.json")
    with open(spec, "w") as f:
        json.dump({"root": ROOT, "bases": bases_path, "nbases": int(nbases), "holes": [int(h) for h in holes], "cases": listed}, f)
    env = dict(os.environ)
    env.update(env_extra)
    env["SWM_TRACE"] = "1"
    out = subprocess.run([sys.executable, "-c", CHILD, spec], env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    recs = [json.loads(l[5:]) for l in out.stdout.splitlines() if l.startswith("CASE ")]
    assert [r["name"] for r in recs] == [c["name"] for c in cases], out.stdout[-2000:] + out.stderr[-4000:]
    return {r["name"]: r for r in recs}


# ------------------------------------------------------------------------------------------------ references
class Refs:
    """The base set, the uniform scalars and their MSM per chunk of CUTS (every prefix / sub-range reference is a sum of chunks),
    and the helpers that turn a small change of the scalars into a small change of the reference."""

    def __init__(self, tmp):
        from pyref.prng import fr_array
        self.orc = orc = Oracle()
        self.threads = orc.lib.oracle_max_threads()
        self.tmp = tmp
        self.tau = h2i(golden("msm.json")["tau"])
        self.G = orc.points_to_mont([tuple(h2i(v) for v in golden("g1.json")["generator"])])
        self.bases = orc.srs_bases(N_BASES, self.tau, self.G)
        self.bases_path = os.path.join(tmp, "bases.npy")
        np.save(self.bases_path, self.bases)
        self.uniform = fr_array(N_BASES, 2601)
        self.chunk = {(lo, hi): self.msm(self.uniform[lo:hi], lo) for lo, hi in zip(CUTS, CUTS[1:])}

    def msm(self, sc, offset=0):
        """oracle MSM of sc over bases[offset ...] (Jacobian)"""
        sc = np.ascontiguousarray(sc, dtype=np.uint64)
        return self.orc.msm(np.ascontiguousarray(self.bases[offset:offset + sc.shape[0]]), sc, threads=self.threads)

    def add(self, *jacs):
        acc = np.ascontiguousarray(jacs[0]).copy()
        for j in jacs[1:]:
            out = np.zeros(18, dtype=np.uint64)
            self.orc.lib.oracle_g1_add(p64(acc), p64(np.ascontiguousarray(j)), p64(out))
            acc = out
        return acc

    def uniform_range(self, lo, hi):
        """MSM(uniform[lo:hi], bases[lo:hi]), lo and hi in CUTS"""
        return self.add(*[v for (a, b), v in self.chunk.items() if lo <= a and b <= hi])

    def sparse(self, rows, values):
        """sum of values[k] * bases[rows[k]] (integers mod r) for a few rows"""
        rows = list(rows)
        return self.orc.msm(np.ascontiguousarray(self.bases[rows]), ints_to_limbs([v % R for v in values], 4), threads=1)

    def geometric(self, s, n, skip=()):
        """[s * (sum_{i < n, i not in skip} tau^i)]G: the MSM of n equal scalars over the base set (identity rows skipped)"""
        geo = (pow(self.tau, n, R) - 1) * pow(self.tau - 1, -1, R) - sum(pow(self.tau, h, R) for h in skip)
        pt = self.orc.fixed_base_mul(self.G, ints_to_limbs([s * geo % R], 4), threads=1)
        return self.orc.points_from_mont(np.ascontiguousarray(pt.reshape(1, 12)))[0]

    def affine(self, jac):
        return self.orc.jac_to_affine_int(jac)

    def got(self, rec):
        return None if rec["inf"] else self.orc.points_from_mont(np.array(rec["xy"], dtype=np.uint64).reshape(1, 12))[0]

    def child(self, n_bases, env, cases, holes=(), timeout=180):
        return run_child(self.tmp, self.bases_path, n_bases, env, cases, holes, timeout)


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return Refs(str(tmp_path_factory.mktemp("msm_schedules")))


def equal(s, n):
    return np.ascontiguousarray(np.tile(ints_to_limbs([s], 4), (n, 1)))


def witness_mix(n):
    """25 % zeros, 25 % ones, 50 % uniform: the witness shape of test_gpu_kernels.py"""
    from pyref.prng import fr_array
    st = fr_array(n, 2677)
    st[0::4] = 0
    st[1::4] = 0
    st[1::4, 0] = 1
    return st


@pytest.fixture(scope="module")
def witness_262144(refs):
    st = witness_mix(262144)
    return st, refs.affine(refs.msm(st))


def test_digit_model_matches_the_recoding():
    """The model the clustered cases are placed with, against plain integers: sum_w digit_w 2^bit_w == s for every layout used."""
    from pyref.prng import fr_array
    sc = np.concatenate([fr_array(500, 3), ints_to_limbs([0, 1, R - 1, R - 2, BIG253, (1 << 128) - 1, 1 << 13, (1 << 13) + 1], 4)])
    vals = limbs_to_ints(sc)
    for nwin in (19, 16, 15, 14, 12):
        base, extra = divmod(254, nwin)
        widths = [base + (1 if w < extra else 0) for w in range(nwin)]
        bk = buckets(sc, nwin)
        assert (bk < (1 << (widths[0] - 1))).all()
        # signs are not returned: rebuild them from the same rule, digit by digit, on integers
        for i, s in enumerate(vals):
            carry, bit, tot = 0, 0, 0
            for w, c in enumerate(widths):
                d = ((s >> bit) & ((1 << c) - 1)) + carry
                carry = 1 if d > (1 << (c - 1)) else 0
                d -= carry << c
                assert abs(d) - 1 == bk[w, i]
                tot += d << bit
                bit += c
            assert tot == s and carry == 0


# ------------------------------------------------------------------------------------------------ per-window schedule
NO_TABLE = {"SWM_MSM_NO_TABLE": "1"}
PW_ONE_LEVEL = {"flat": 0, "two_level": 0, "c": 14}
PW_C14 = {"flat": 0, "two_level": 1, "c": 14, "c_top": 13, "nwin": 19}
PW_C16 = {"flat": 0, "two_level": 1, "c": 16, "c_top": 15, "nwin": 16}


def check_kernels(rec, present, absent=()):
    missing = [k for k in present if k not in rec["kernels"]]
    extra = [k for k in absent if k in rec["kernels"]]
    assert not missing and not extra, "PRECONDITION %s: kernels not launched %r, launched against the case %r (%r)" % (
        rec["name"], missing, extra, rec["kernels"])


def check_two_level(recs):
    for rec in recs.values():
        check_kernels(rec, PER_WINDOW_KERNELS + TWO_LEVEL_KERNELS, ("msm_flat_bin_sort",))


@pytest.fixture(scope="module")
def pw_uniform(refs):
    """Uniform scalars at every size of the per-window plan; the other per-window tests take the bin plans from its shape lines."""
    u = refs.uniform
    cases = [
        {"name": "n262143", "scalars": u[:262143], "expect": PW_ONE_LEVEL},
        {"name": "n262144", "scalars": u[:262144], "expect": PW_C14},
        {"name": "n262144_dev_mont", "scalars": refs.orc.fr_to_mont(np.ascontiguousarray(u[:262144])), "dev_mont": True, "expect": PW_C14},
        {"name": "ragged", "scalars": u[:N_RAGGED], "expect": PW_C14},
        {"name": "n393217", "scalars": u[:N_BASES], "expect": PW_C16},
    ]
    return refs.child(N_BASES, NO_TABLE, cases)


@pytest.mark.gpu
def test_per_window_uniform_at_the_plan_thresholds(refs, pw_uniform):
    """n = 262143 (largest one-level sort), 262144 (first two-level sort, c = 14; standard-form host scalars and Montgomery-form
    device scalars), 262144 + 3 * 8192 + 1 (ragged tiles), 393217 (first size of the c = 16 plan)."""
    r = pw_uniform
    check_kernels(r["n262143"], PER_WINDOW_KERNELS, TWO_LEVEL_KERNELS + ("msm_flat_bin_sort",))
    check_two_level({k: v for k, v in r.items() if k != "n262143"})
    for name, n in (("n262143", 262143), ("n262144", 262144), ("n262144_dev_mont", 262144), ("ragged", N_RAGGED), ("n393217", N_BASES)):
        assert refs.got(r[name]) == refs.affine(refs.uniform_range(0, n)), name


@pytest.mark.gpu
def test_per_window_equal_scalars_every_window_falls_back(refs):
    """All scalars equal: one bucket per window holds every point, every window is marked bad by msm_bin_check and sorted by
    msm_scatter, every bucket folded by msm_big_bucket_sum.  Closed form."""
    cases = [{"name": "%s_%d" % (tag, n), "scalars": equal(s, n), "expect": exp}
             for n, exp in ((262144, PW_C14), (N_BASES, PW_C16)) for tag, s in (("one", 1), ("rm1", R - 1), ("big253", BIG253))]
    recs = refs.child(N_BASES, NO_TABLE, cases)
    check_two_level(recs)
    for c in cases:
        n = c["scalars"].shape[0]
        s = limbs_to_ints(c["scalars"][:1])[0]
        assert refs.got(recs[c["name"]]) == refs.geometric(s, n), c["name"]


@pytest.mark.gpu
def test_per_window_mixed_good_and_bad_windows(refs):
    """Low 128 bits equal and high bits uniform, and the mirror image: the windows below (above) bit 128 hold one bucket of n
    entries and take the msm_scatter fallback, the others go through msm_partition / msm_bin_sort in the same launches."""
    n = 262144
    u = refs.uniform[:n]
    lo_equal = u.copy()
    lo_equal[:, :2] = u[7, :2]
    hi_equal = u.copy()
    hi_equal[:, 2:] = u[7, 2:]
    bk = buckets(lo_equal, 19)
    # precondition on the inputs: windows entirely below bit 128 (14-bit windows 0 .. 6, 13-bit 7, 8) have ONE bucket, the top
    # windows have no bucket beyond a bin's capacity
    assert all(len(np.unique(bk[w])) == 1 for w in range(8)) and np.bincount(bk[18][bk[18] >= 0]).max() < 1000
    bk = buckets(hi_equal, 19)
    assert all(len(np.unique(bk[w])) == 1 for w in range(11, 19)) and np.bincount(bk[0][bk[0] >= 0]).max() < 256
    cases = [{"name": "low_equal", "scalars": lo_equal, "expect": PW_C14}, {"name": "high_equal", "scalars": hi_equal, "expect": PW_C14}]
    recs = refs.child(N_BASES, NO_TABLE, cases)
    check_two_level(recs)
    for c in cases:
        assert refs.got(recs[c["name"]]) == refs.affine(refs.msm(c["scalars"])), c["name"]


@pytest.mark.gpu
def test_per_window_bin_at_and_above_bin_cap(refs, pw_uniform):
    """Exactly BIN_CAP entries of window 0 in one coarse bin (the window stays on the bin sort), then BIN_CAP + 1 (msm_bin_check
    marks the window bad, it alone takes msm_scatter).  The bin is placed with the fb the shape line reports."""
    n = 262144
    fb = pw_uniform["n262144"]["shape"]["fb0"]
    assert pw_uniform["n262144"]["shape"]["nbins0"] == 8192 >> fb
    sc = refs.uniform[:n].copy()
    target = 17                                   # a bin in the positive half of window 0: digits target * 2^fb + 1 .. + 2^fb
    in_bin = lambda a: (buckets(a, 19)[0] >> fb) == target
    move = np.flatnonzero(~in_bin(sc))[:BIN_CAP + 1 - int(in_bin(sc).sum())]
    low = (target << fb) + 1 + (np.arange(len(move), dtype=np.uint64) * np.uint64(37)) % np.uint64(1 << fb)
    sc[move, 0] = (sc[move, 0] & ~np.uint64((1 << 14) - 1)) | low.astype(np.uint64)
    over = sc.copy()
    at = sc.copy()
    at[move[-1]] = refs.uniform[move[-1]]           # one entry fewer
    assert int(in_bin(at).sum()) == BIN_CAP and int(in_bin(over).sum()) == BIN_CAP + 1
    b0 = buckets(over, 19)[0]
    w0 = np.bincount(b0[b0 >= 0] >> fb)
    assert np.delete(w0, target).max() < BIN_CAP    # every other bin of the window is far below
    cases = [{"name": "at_cap", "scalars": at, "expect": dict(PW_C14, fb0=fb)}, {"name": "over_cap", "scalars": over, "expect": dict(PW_C14, fb0=fb)}]
    recs = refs.child(N_BASES, NO_TABLE, cases)
    check_two_level(recs)
    ref_at = refs.msm(at)
    j = int(move[-1])
    delta = limbs_to_ints(over[j:j + 1])[0] - limbs_to_ints(at[j:j + 1])[0]
    assert refs.got(recs["at_cap"]) == refs.affine(ref_at)
    assert refs.got(recs["over_cap"]) == refs.affine(refs.add(ref_at, refs.sparse([j], [delta])))


def top_heavy(n, seed):
    """r - 1, r - 2, values with the largest top digit the field allows (r - 1 - x, x < 2^200) and uniform values: 5000 each of
    the first three, so that the top window's bins stay below BIN_CAP and the window keeps the bin sort."""
    from pyref.prng import fr_array
    sc = fr_array(n, seed)
    x = limbs_to_ints(fr_array(5000, seed + 1))
    sc[3:20000:4] = ints_to_limbs([R - 1], 4)[0]
    sc[1:20000:4] = ints_to_limbs([R - 2], 4)[0]
    sc[2:20000:4] = ints_to_limbs([R - 1 - (v >> 53) for v in x], 4)
    return sc


@pytest.mark.gpu
def test_per_window_top_window_at_its_limit(refs, pw_uniform):
    """The top window only sees digits up to (r - 1) >> bit: its bin plan (beff, nbins_top) is sized for that, and the last bin is
    the one msm_bin_check lets nothing lie beyond.  Scalars whose top digit is the largest possible fill that last bin."""
    cases = []
    for name, n, exp, nwin, ctop in (("c14", 262144, PW_C14, 19, 13), ("c16", N_BASES, PW_C16, 16, 15)):
        shape = pw_uniform["n%d" % n]["shape"]
        fbt, nbt = shape["fb_top"], shape["nbins_top"]
        sc = top_heavy(n, 2700 + nwin)
        top = buckets(sc, nwin)[nwin - 1]
        # the largest top digit the field allows is that of r - 1 (the recoding is monotone): ((r - 1) >> bit) + 1, because the
        # window below carries — the "+ 1 for the carry" of the top window's plan in msm_shape
        top_max = int(buckets(ints_to_limbs([R - 1], 4), nwin)[nwin - 1, 0])
        assert top_max + 1 == ((R - 1) >> (254 - ctop)) + 1
        # precondition on the inputs: that digit occurs, it lies in the LAST bin of the plan, the plan is short of the window's
        # nominal bin count, and the last bin (15000 + its share of the uniform values) still fits the bin sort
        assert top.max() == top_max and (top_max >> fbt) == nbt - 1 and nbt < (1 << (ctop - 1)) >> fbt, (name, top.max(), fbt, nbt)
        last = int(((top >> fbt) == nbt - 1).sum())
        assert 15000 <= last <= BIN_CAP, (name, last)
        cases.append({"name": name, "scalars": sc, "expect": dict(exp, fb_top=fbt, nbins_top=nbt)})
    recs = refs.child(N_BASES, NO_TABLE, cases)
    check_two_level(recs)
    for c in cases:
        assert refs.got(recs[c["name"]]) == refs.affine(refs.msm(c["scalars"])), c["name"]


@pytest.mark.gpu
def test_per_window_witness_mix(refs, witness_262144):
    st, want = witness_262144
    recs = refs.child(N_BASES, NO_TABLE, [{"name": "witness", "scalars": st, "expect": PW_C14}])
    check_two_level(recs)
    assert refs.got(recs["witness"]) == want


@pytest.mark.gpu
def test_per_window_identity_bases(refs):
    """Rows of the base set zeroed (the point at infinity is a valid base): at the first and last point, on both sides of a
    partition tile (8192) and of a sort tile (65536), in the middle, and strided — their digits are dropped, so the bins they
    would have opened, closed or sat inside lose their first, last or a middle entry.  Uniform scalars (bin sort) and equal
    scalars (every window on the fallback, the holes first / inside / last in the one chain)."""
    n = 262144
    holes = sorted(set([0, 1, 8191, 8192, 65535, 65536, n // 2, n - 2, n - 1] + list(range(777, n, 4099))))
    u = refs.uniform[:n]
    cases = [{"name": "uniform", "scalars": u, "expect": PW_C14}, {"name": "equal", "scalars": equal(0xABCDEF123, n), "expect": PW_C14}]
    recs = refs.child(N_BASES, NO_TABLE, cases, holes=holes)
    check_two_level(recs)
    minus = refs.sparse(holes, [-v for v in limbs_to_ints(u[holes])])
    assert refs.got(recs["uniform"]) == refs.affine(refs.add(refs.uniform_range(0, n), minus))
    assert refs.got(recs["equal"]) == refs.geometric(0xABCDEF123, n, skip=holes)


# ------------------------------------------------------------------------------------------------ flat schedule on XYZZ rows
@pytest.mark.gpu
def test_flat_xyzz_throughput_variant(refs, witness_262144):
    """SWM_MSM_TE=0 (what a set outside the prime-order subgroup gets, and any set after a failed TE allocation) at the first
    size that is not low-latency: msm_accumulate on table rows, msm_big_bucket_sum<XYZZ>, msm_bucket_reduce<XYZZ>, SEG = 128."""
    n = 262144
    exp = {"flat": 1, "te": 0, "lat": 0, "SEG": 128}
    off = 100003
    cases = [
        {"name": "uniform", "scalars": refs.uniform[:n], "expect": exp},
        {"name": "equal_one", "scalars": equal(1, n), "expect": exp},
        {"name": "equal_big253", "scalars": equal(BIG253, n), "expect": exp},
        {"name": "witness", "scalars": witness_262144[0], "expect": exp},
        {"name": "offset_ragged", "scalars": refs.uniform[off:], "offset": off, "expect": exp},
    ]
    recs = refs.child(N_BASES, {"SWM_MSM_TE": "0"}, cases)
    for rec in recs.values():
        check_kernels(rec, FLAT_KERNELS, TWO_LEVEL_KERNELS + ("msm_scatter",))
    assert N_BASES - off >= 262144 and (N_BASES - off) % 128
    assert refs.got(recs["uniform"]) == refs.affine(refs.uniform_range(0, n))
    assert refs.got(recs["equal_one"]) == refs.geometric(1, n)
    assert refs.got(recs["equal_big253"]) == refs.geometric(BIG253, n)
    assert refs.got(recs["witness"]) == witness_262144[1]
    assert refs.got(recs["offset_ragged"]) == refs.affine(refs.uniform_range(off, N_BASES))


# ------------------------------------------------------------------------------------------------ flat schedule, clustered scalars
def clustered(n, shape, reps, bins, seed):
    """n scalars: per bin k of `bins`, FLAT_WIDE_Q + 4 adjacent small values v repeated `reps` times each — window 0 puts them into
    the buckets v - 1 at the LOWER edge of bin k (from bucket k 2^fb) — and as many at the UPPER edge of bin k - 1 (up to bucket
    k 2^fb - 1); half of each as v, half as r - (v + 1) (r = 1 mod 2^47, so that scalar's window-0 digit is -v: the same bucket,
    reached by a negative digit).  The rest uniform."""
    from pyref.prng import fr_array
    fb = shape["flat_fb"]
    per = FLAT_WIDE_Q + 4
    assert per <= 1 << fb
    sc = fr_array(n, seed)
    vals = []
    for k in bins:
        vals += [(k << fb) + 1 + j for j in range(per)] + [(k << fb) - j for j in range(per)]
    assert len(vals) * reps <= n - n // 4
    pick = np.repeat(np.array(vals, dtype=np.int64), reps)
    pos = np.random.default_rng(seed).permutation(n)[:len(pick)]
    signed = [int(v) if i % 2 else R - (int(v) + 1) for i, v in enumerate(pick)]
    sc[pos] = ints_to_limbs(signed, 4)
    return sc


def cluster_stats(sc, shape, bins):
    """(entries of the bin, buckets of the bin with more than FLAT_WIDE_NS segments) for every listed bin and its lower neighbour"""
    fb, seg = shape["flat_fb"], shape["SEG"]
    bk = buckets(sc, shape["nwin"])
    cnt = np.bincount(bk[bk >= 0], minlength=1 << (shape["c"] - 1))
    out = []
    for k in bins:
        for b in (k - 1, k):
            part = cnt[b << fb:(b + 1) << fb]
            out.append((int(part.sum()), int(((part + seg - 1) // seg > FLAT_WIDE_NS).sum())))
    return out


@pytest.mark.gpu
def test_flat_te_wide_bucket_queue_overflow_low_latency(refs):
    """A 2^17-point set (TE rows, low-latency variant): more than FLAT_WIDE_Q buckets of one bin with more than FLAT_WIDE_NS
    segments each, so that the queue of msm_flat_bin_sort overflows and the buckets beyond it are written by their own lane —
    once in bins that still fit LDS (<= FLAT_BIN_CAP entries), once in bins placed in HBM.  The clustered buckets sit at both
    edges of a bin, filled by positive and negative digits."""
    n = 1 << 17
    exp = {"flat": 1, "te": 1, "lat": 1}
    probe = refs.child(n, {}, [{"name": "uniform", "scalars": refs.uniform[:n], "expect": exp}])
    shape = probe["uniform"]["shape"]
    check_kernels(probe["uniform"], FLAT_KERNELS, TWO_LEVEL_KERNELS + ("msm_scatter",))
    assert refs.got(probe["uniform"]) == refs.affine(refs.uniform_range(0, n))
    seg = shape["SEG"]
    reps_lds = FLAT_WIDE_NS * seg + 2                      # each bucket: 17 segments (plus whatever the uniform rest adds)
    reps_hbm = -(-(FLAT_BIN_CAP + 1) // (FLAT_WIDE_Q + 4))  # each bin: above FLAT_BIN_CAP from the clustered values alone
    assert reps_hbm > reps_lds
    lds = clustered(n, shape, reps_lds, (5,), 2801)
    hbm = clustered(n, shape, reps_hbm, (9,), 2802)
    for entries, wide in cluster_stats(lds, shape, (5,)):
        assert entries <= FLAT_BIN_CAP and wide > FLAT_WIDE_Q, (entries, wide, shape)
    for entries, wide in cluster_stats(hbm, shape, (9,)):
        assert entries > FLAT_BIN_CAP and wide > FLAT_WIDE_Q, (entries, wide, shape)
    cases = [{"name": "lds", "scalars": lds, "expect": dict(exp, SEG=seg, flat_fb=shape["flat_fb"])},
             {"name": "hbm", "scalars": hbm, "expect": dict(exp, SEG=seg, flat_fb=shape["flat_fb"])}]
    recs = refs.child(n, {}, cases)
    for c in cases:
        check_kernels(recs[c["name"]], FLAT_KERNELS, TWO_LEVEL_KERNELS + ("msm_scatter",))
        assert refs.got(recs[c["name"]]) == refs.affine(refs.msm(c["scalars"])), c["name"]


@pytest.mark.gpu
def test_flat_te_more_than_1024_bins_and_queue_overflow(refs):
    """n = 262144 + 1 under SWM_MSM_TABLE_C=22: the size at which the coarse bin count of that width moves past 1024, so the
    four-bins-per-lane form msm_flat_scan_bins<4> runs (n = 262144 still has 1024 bins: one per lane).  Uniform scalars, and the
    queue overflow in a bin above FLAT_BIN_CAP — with SEG = 128 (throughput variant) FLAT_WIDE_Q + 1 buckets of more than
    FLAT_WIDE_NS segments are more than 69 000 entries, so no bin of this shape fits LDS: that form is covered on the
    low-latency set above."""
    n = 262145
    env = {"SWM_MSM_TABLE_C": "22"}
    exp = {"flat": 1, "te": 1, "lat": 0, "c": 22}
    probe = refs.child(n, env, [{"name": "n262144", "scalars": refs.uniform[:262144], "expect": dict(exp, flat_bins=1024)},
                                {"name": "uniform", "scalars": refs.uniform[:n], "expect": exp, "at_least": {"flat_bins": 1025}}])
    shape = probe["uniform"]["shape"]
    assert refs.got(probe["n262144"]) == refs.affine(refs.uniform_range(0, 262144))
    assert refs.got(probe["uniform"]) == refs.affine(refs.uniform_range(0, n))
    seg = shape["SEG"]
    sc = clustered(n, shape, FLAT_WIDE_NS * seg + 2, (3,), 2803)
    for entries, wide in cluster_stats(sc, shape, (3,)):
        assert entries > FLAT_BIN_CAP and wide > FLAT_WIDE_Q, (entries, wide, shape)
    case = {"name": "hbm", "scalars": sc, "expect": dict(exp, SEG=seg, flat_fb=shape["flat_fb"]), "at_least": {"flat_bins": 1025}}
    recs = refs.child(n, env, [case])
    check_kernels(recs["hbm"], FLAT_KERNELS, TWO_LEVEL_KERNELS + ("msm_scatter",))
    assert refs.got(recs["hbm"]) == refs.affine(refs.msm(sc))


# ------------------------------------------------------------------------------------------------ duplicate and opposite bases
# Equal and opposite bases are what sends an XYZZ accumulation off its generic formula: madd28 returns false and the segment is
# redone by the cold path of msm_accumulate (from the raw bases in the per-window schedule, from table rows rescaled by 2^376 in
# the flat one), p28_slot_add takes its pp == 0 branch in the bucket stage; the twisted Edwards schedules must not notice.  Rows of
# the [tau^i]G set are overwritten in place:
DUP_RUNS = ((100, 2), (110, 3), (200, 129))   # (first row, length) of runs of one point: 2, 3, and SEG + 1 for the largest SEG (128)
DUP_PAIR, DUP_TRIPLE, DUP_HOLE, DUP_ORDER2, DUP_SMALL_X = 400, 410, 420, 430, 440


def dup_bases(refs, n, order2):
    """bases[:n] with runs of equal points, P next to -P, (P, -P, P) and (P, O, P); order2: also (P, T2 - P, P, T2 - P) for
    T2 = (q - 1, 0) and the curve point (2, 3), which take the set out of the prime-order subgroup (XYZZ rows)."""
    from oracle_lib import Q
    from pyref.bls12_377 import g1_add, g1_neg
    b = np.ascontiguousarray(refs.bases[:n]).copy()

    def negated(row):
        out = row.copy()
        out[6:] = ints_to_limbs([(Q - limbs_to_ints(row[None, 6:])[0]) % Q], 6)[0]
        return out

    for first, length in DUP_RUNS:
        b[first:first + length] = b[first]
    b[DUP_PAIR + 1] = negated(b[DUP_PAIR])
    b[DUP_TRIPLE + 1] = negated(b[DUP_TRIPLE])
    b[DUP_TRIPLE + 2] = b[DUP_TRIPLE]
    b[DUP_HOLE + 1] = 0
    b[DUP_HOLE + 2] = b[DUP_HOLE]
    if order2:
        pt = refs.orc.points_from_mont(np.ascontiguousarray(b[DUP_ORDER2:DUP_ORDER2 + 1]))[0]
        other = refs.orc.points_to_mont([g1_add((Q - 1, 0), g1_neg(pt))])[0]
        b[DUP_ORDER2 + 1] = other
        b[DUP_ORDER2 + 2] = b[DUP_ORDER2]
        b[DUP_ORDER2 + 3] = other
        b[DUP_SMALL_X] = refs.orc.points_to_mont([(2, 3)])[0]
    return b


class DupSet:
    def __init__(self, refs, n, order2):
        self.refs, self.n = refs, n
        self.bases = dup_bases(refs, n, order2)
        self.path = os.path.join(refs.tmp, "dup_%d_%d.npy" % (n, int(order2)))
        np.save(self.path, self.bases)
        self.scalars = {"equal": equal(BIG253, n), "uniform": np.ascontiguousarray(refs.uniform[:n])}   # BIG253 is odd
        self.want = {k: refs.affine(refs.orc.msm(self.bases, sc, threads=refs.threads)) for k, sc in self.scalars.items()}

    def run(self, env, expect, present, absent=()):
        cases = [{"name": k, "scalars": sc, "expect": expect} for k, sc in self.scalars.items()]
        recs = run_child(self.refs.tmp, self.path, self.n, env, cases)
        for k in self.scalars:
            check_kernels(recs[k], present, absent)
            assert self.refs.got(recs[k]) == self.want[k], k


@pytest.fixture(scope="module")
def dup_small(refs):
    return {order2: DupSet(refs, 2048, order2) for order2 in (False, True)}


@pytest.fixture(scope="module")
def dup_large(refs):
    return {order2: DupSet(refs, 262144, order2) for order2 in (False, True)}


def test_duplicate_base_sets_are_what_they_claim():
    """No device: the rows of the duplicate sets are the points the cases are named after, and on the curve (on the first 512
    points of the set, which hold every overwritten row)."""
    import types
    from oracle_lib import Q
    from pyref.bls12_377 import g1_add, g1_is_on_curve, g1_neg
    orc = Oracle()
    G = orc.points_to_mont([tuple(h2i(v) for v in golden("g1.json")["generator"])])
    small = types.SimpleNamespace(orc=orc, bases=orc.srs_bases(512, h2i(golden("msm.json")["tau"]), G))
    pts = orc.points_from_mont(dup_bases(small, 512, True))
    assert BIG253 & 1 and all(g1_is_on_curve(p) for p in pts)
    for first, length in DUP_RUNS:
        assert len(set(pts[first:first + length])) == 1 and pts[first - 1] != pts[first] != pts[first + length]
    assert pts[DUP_PAIR + 1] == g1_neg(pts[DUP_PAIR]) and pts[DUP_TRIPLE + 1] == g1_neg(pts[DUP_TRIPLE]) and pts[DUP_TRIPLE + 2] == pts[DUP_TRIPLE]
    assert pts[DUP_HOLE + 1] is None and pts[DUP_HOLE + 2] == pts[DUP_HOLE]
    assert g1_add(pts[DUP_ORDER2], pts[DUP_ORDER2 + 1]) == (Q - 1, 0) and g1_add((Q - 1, 0), (Q - 1, 0)) is None
    assert pts[DUP_ORDER2 + 2] == pts[DUP_ORDER2] and pts[DUP_ORDER2 + 3] == pts[DUP_ORDER2 + 1] and pts[DUP_SMALL_X] == (2, 3)


DUP_XYZZ_ABSENT = TWO_LEVEL_KERNELS + ("msm_flat_bin_sort",)


@pytest.mark.gpu
def test_duplicates_per_window_raw_bases(dup_small):
    """SWM_MSM_NO_TABLE at 2048 points: msm_accumulate on the raw bases — its cold path with bases != nullptr — and
    msm_bucket_reduce<XYZZ>; the subgroup set and the set with (P, T2 - P, P, T2 - P) under equal odd and uniform scalars."""
    for order2 in (False, True):
        dup_small[order2].run(NO_TABLE, {"flat": 0, "te": 0, "two_level": 0}, PER_WINDOW_KERNELS, DUP_XYZZ_ABSENT)


@pytest.mark.gpu
def test_duplicates_xyzz_table_rows(dup_small):
    """A set with one point outside the subgroup gets XYZZ table rows: the cold path rescales rows by 2^376 (bases == nullptr)."""
    dup_small[True].run({}, {"flat": 1, "te": 0, "lat": 1}, FLAT_KERNELS, TWO_LEVEL_KERNELS + ("msm_scatter",))


@pytest.mark.gpu
def test_duplicates_flat_xyzz_throughput(dup_large):
    for order2 in (False, True):
        dup_large[order2].run({"SWM_MSM_TE": "0"}, {"flat": 1, "te": 0, "lat": 0, "SEG": 128}, FLAT_KERNELS, TWO_LEVEL_KERNELS + ("msm_scatter",))


@pytest.mark.gpu
def test_duplicates_flat_te_low_latency_quad(dup_small):
    """twisted Edwards rows, four lanes per segment and per chain: the unified law takes equal, opposite and identity rows."""
    dup_small[False].run({}, {"flat": 1, "te": 1, "lat": 1}, FLAT_KERNELS, TWO_LEVEL_KERNELS + ("msm_scatter",))


@pytest.mark.gpu
def test_duplicates_flat_te_throughput(dup_large):
    dup_large[False].run({}, {"flat": 1, "te": 1, "lat": 0}, FLAT_KERNELS, TWO_LEVEL_KERNELS + ("msm_scatter",))

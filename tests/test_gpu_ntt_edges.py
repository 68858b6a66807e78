"""The transform (ntt.hip: ntt_pass_lazy on fr29.cuh, and the two older paths) on the inputs at which the host plan's value bounds
are tight, where uniformly random residues never come: constants, combs of r - 1 and 0 at every butterfly distance (largest and
most negative differences), single elements at the tile boundaries of the first pass, the tight fill and root orbits (n - 1 outputs
exactly zero: they must come out as 0, never as r).  The values are raw MEMORY integers: the lazy kernel works on the 256-bit words
as they come, so r - 1 in memory is the extreme.  The inputs are the descriptions of tools/check_ntt29.py (edge_inputs), which
feeds the same ones to the bit-level emulation of the kernel on the CPU (tests/test_ntt29_emulation.py).

References, bit for bit: the C oracle (all host threads) at every size; up to 2^13 also the closed forms in Python integers
(check_ntt29.closed_form: constants, single elements, fills and orbits at every size, the combs up to 2^10, where the product of
log n factors per point still takes well under a second per size).

Sizes and the plan each gets from ntt_run_multi (radices per pass; J columns per tile; b_in = 1 in the first pass of a plain or
inverse transform, 2 in a forward coset transform and in every later pass):
   1 .. 5     one pass, J = 1: a radix-2 level only (1), one radix-4 step (2), radix-2 + one step (3), two steps (4, 5)
   6, 7       three steps: with b_in = 2 the first plans whose chain passes 4B > 64 (B = 32 / 64 going into the last step)
   8, 9, 10   one pass, J = 1, four / five steps: the b_in = 1 chain reaches B = 64; odd and even log_r
   11         6 + 5, J = 8 / 16; 12: 6 + 6, J = 8; 13: 7 + 6, J = 4 / 8: two passes, pass tables
   19         10 + 9: the J rule switches to 1024 >> log_r (J = 1 / 2)
   20         10 + 10, J = 1
   21         7 + 7 + 7, J = 8: three passes through the second scratch buffer
   22         8 + 7 + 7, J = 4 / 8
Above 2^13 the combs run at p in {0, radices[0] - 1, radices[0], log n - 1} and the single-element and fill inputs are left to the
small sizes.  An oracle reference is computed once per (size, input, direction, variant) in this process; its digest is kept so
that the two child processes (SWM_NTT_PASS_TABLES=0: the two-level twiddle product inside the lazy kernel; SWM_NTT_LAZY=0: the
32-bit-limb kernel; both switches are read once per process) are checked against the references the tests before them computed."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_lib import Oracle, ints_to_limbs, p64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ntt29 as C  # noqa: E402

pytestmark = pytest.mark.gpu

VARIANTS = ((0, 0), (0, 1), (1, 0), (1, 1))  # (inverse, coset)
SMALL = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13)
LARGE = (19, 20, 21, 22)
DRIVER_LOGS = (4, 5, 10, 11, 12, 16)
CHILD_LOGS = (5, 10, 11, 13, 20, 21)
CLOSED_MAX, CLOSED_COMB_MAX = 13, 10
TOPL = ints_to_limbs([C.TOP], 4)[0]


def inputs(log_n):
    return C.edge_inputs(log_n, reduced=log_n > CLOSED_MAX)


def build(orc, d, log_n):
    """input d as n x 4 uint64 memory words (numpy: the Python lists of check_ntt29.materialize are too slow at 2^22)"""
    n = 1 << log_n
    x = np.zeros((n, 4), dtype=np.uint64)
    if d[0] == "const":
        x[:] = ints_to_limbs([d[1]], 4)[0]
    elif d[0] == "comb":
        x[((np.arange(n) >> d[1]) & 1) != d[2]] = TOPL
    elif d[0] == "single" or (d[0] == "fill" and d[2]):
        x[d[1]] = TOPL
    elif d[0] == "fill":
        x[:] = TOPL
        x[d[1]] = 0
    else:  # orbit: x[k .. 2k) = x[0 .. k) w^(s k), the Montgomery product of memory integers with the Montgomery form of w^(s k)
        assert d[0] == "orbit"
        ws = pow(C.root(log_n, False), d[1], C.R)
        x[0] = TOPL
        k = 1
        while k < n:
            rep = np.ascontiguousarray(np.repeat(orc.fr_mont_from_ints([pow(ws, k, C.R)]), k, axis=0))
            seg, out = np.ascontiguousarray(x[:k]), np.empty((k, 4), dtype=np.uint64)
            orc.lib.oracle_fr_mul(p64(seg), p64(rep), p64(out), k)
            x[k:2 * k] = out
            k *= 2
        for i in (1, n // 2, n - 1):  # the builder itself, against Python integers
            assert np.array_equal(x[i], ints_to_limbs([C.TOP * pow(ws, i, C.R) % C.R], 4)[0])
    return x


_DIGEST = {}


def digest(a):
    return hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).hexdigest()


def oracle_ref(orc, x, log_n, d, inverse, coset):
    y = orc.ntt(x, log_n, inverse, coset, threads=orc.lib.oracle_max_threads())
    _DIGEST[(log_n, d, inverse, coset)] = digest(y)
    return y


def ref_digest(orc, log_n, d, inverse, coset):
    key = (log_n, d, inverse, coset)
    if key not in _DIGEST:
        oracle_ref(orc, build(orc, d, log_n), log_n, d, inverse, coset)
    return _DIGEST[key]


def has_closed_form(d, log_n):
    return log_n <= (CLOSED_COMB_MAX if d[0] == "comb" else CLOSED_MAX)


def check_transform(ctx, orc, d, log_n, on_device=False):
    x = build(orc, d, log_n)
    for inverse, coset in VARIANTS:
        if on_device:
            buf = ctx.to_device(x)
            ctx.ntt_fr_dev(buf, log_n, bool(inverse), bool(coset))
            got = buf.download(x.shape)
            buf.free()
        else:
            got = ctx.ntt_fr(x, log_n, bool(inverse), bool(coset))
        assert np.array_equal(got, oracle_ref(orc, x, log_n, d, inverse, coset)), ("oracle", d, log_n, inverse, coset)
        if has_closed_form(d, log_n):
            want = ints_to_limbs(C.closed_form(d, log_n, bool(inverse), bool(coset)), 4)
            assert np.array_equal(got, want), ("closed form", d, log_n, inverse, coset)
        if d[0] == "orbit" and not inverse and not coset:  # at every size: n (r - 1) at -s mod n, the rest exactly zero
            n = 1 << log_n
            at = (-d[1]) % n
            assert np.array_equal(got[at], ints_to_limbs([n * C.TOP % C.R], 4)[0]) and not np.delete(got, at, axis=0).any(), (d, log_n)
        if d == ("const", 0):
            assert not got.any(), (d, log_n, inverse, coset)


@pytest.fixture(scope="module")
def ctx():
    import simpleworks_amd as swm
    c = swm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def test_the_numpy_inputs_are_the_emulators(orc):
    for log_n in (1, 7):
        for d in C.edge_inputs(log_n):
            assert np.array_equal(build(orc, d, log_n), ints_to_limbs(C.materialize(d, log_n), 4)), (d, log_n)


def test_the_plans_are_the_ones_the_docstring_names():
    want = {1: [1], 5: [5], 10: [10], 11: [6, 5], 12: [6, 6], 13: [7, 6], 16: [8, 8], 19: [10, 9], 20: [10, 10], 21: [7, 7, 7], 22: [8, 7, 7]}
    for log_n, radices in want.items():
        assert C.pass_radices(log_n) == radices


@pytest.mark.parametrize("log_n", SMALL)
def test_edges_small(ctx, orc, log_n):
    """every input family, every comb level, forward / inverse x plain / coset, through swm_ntt_fr"""
    for d in inputs(log_n):
        check_transform(ctx, orc, d, log_n)


@pytest.mark.parametrize("log_n, which", [(lg, w) for lg in LARGE for w in range(len(C.edge_inputs(lg, reduced=True)))])
def test_edges_large(ctx, orc, log_n, which):
    """one input per case (four transforms and four oracle references), on a resident buffer through swm_ntt_fr_dev"""
    check_transform(ctx, orc, inputs(log_n)[which], log_n, on_device=True)


# ------------------------------------------------------------------------------------------------ the other drivers
@pytest.mark.parametrize("log_n", DRIVER_LOGS)
def test_from_a_shorter_source(ctx, orc, log_n):
    """ntt_run_from: the first pass reads a source of 1, n/2 + 1, n - 1 or n elements, extremal in the part that exists"""
    n = 1 << log_n
    threads = orc.lib.oracle_max_threads()
    for d in inputs(log_n):
        full = build(orc, d, log_n)
        for ln in sorted({1, n // 2 + 1, n - 1, n}):
            src = np.ascontiguousarray(full[:ln])
            padded = np.zeros((n, 4), dtype=np.uint64)
            padded[:ln] = src
            for inverse, coset in VARIANTS:
                out, back = ctx.selftest_ntt_from(src, log_n, inverse, coset)
                assert np.array_equal(back, src), "source changed"
                assert np.array_equal(out, orc.ntt(padded, log_n, inverse, coset, threads=threads)), (d, log_n, ln, inverse, coset)


@pytest.mark.parametrize("log_n", DRIVER_LOGS)
def test_cosets_forward(ctx, orc, log_n):
    """ntt_cosets_fwd of n + 1 and 2n extremal coefficients: the fold x_i + s_k^n x_(i + n) in canonical arithmetic in front of the
    lazy load, against the entries k mod 4 of the oracle's 4n-point transform"""
    n = 1 << log_n
    threads = orc.lib.oracle_max_threads()
    for d in inputs(log_n + 1):
        full = build(orc, d, log_n + 1)
        for ln in (n + 1, 2 * n):
            padded = np.zeros((4 * n, 4), dtype=np.uint64)
            padded[:ln] = full[:ln]
            big = orc.ntt(padded, log_n + 2, 0, 0, threads=threads)
            for ks in ([1, 2, 3], [3, 0, 2, 1]):
                got = ctx.selftest_ntt_cosets(full[:ln], log_n, ks)
                for c, k in enumerate(ks):
                    assert np.array_equal(got[c], big[k::4]), (d, log_n, ln, ks, k)


@pytest.mark.parametrize("log_n", DRIVER_LOGS)
def test_cosets_inverse_round_trip(ctx, orc, log_n):
    """ntt_cosets_inv + cosets3_solve: the all-(r - 1) polynomial of degree < 3n, and the one with only coefficients 0 and 3n - 1"""
    n = 1 << log_n
    ends = np.zeros((3 * n, 4), dtype=np.uint64)
    ends[0] = ends[3 * n - 1] = TOPL
    for coeffs in (np.tile(TOPL, (3 * n, 1)), ends):
        padded = np.zeros((4 * n, 4), dtype=np.uint64)
        padded[:3 * n] = coeffs
        big = orc.ntt(padded, log_n + 2, 0, 0, threads=orc.lib.oracle_max_threads())
        evals = np.concatenate([big[k::4] for k in range(3)])
        assert np.array_equal(ctx.selftest_intt_cosets3(evals, log_n), coeffs), log_n


# ------------------------------------------------------------------------------------------------ the two older paths
def child_inputs(log_n):
    return [d for d in inputs(log_n) if d[0] in ("const", "comb", "orbit")]


def child_main():
    """in a fresh process (the switch is read once): digests of every transform, one JSON line each, then ok"""
    import simpleworks_amd as swm
    ctx, orc = swm.Context(0), Oracle()
    for log_n in CHILD_LOGS:
        for i, d in enumerate(child_inputs(log_n)):
            x = build(orc, d, log_n)
            for inverse, coset in VARIANTS:
                print(json.dumps([log_n, i, inverse, coset, digest(ctx.ntt_fr(x, log_n, bool(inverse), bool(coset)))]), flush=True)
    ctx.close()
    print("ok")


SCRIPT = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import test_gpu_ntt_edges as T
T.child_main()
"""


@pytest.mark.parametrize("switch", ["SWM_NTT_PASS_TABLES", "SWM_NTT_LAZY"])
def test_edges_on_the_older_paths(orc, switch):
    """constants, combs and orbits at 2^5 .. 2^21 with the switch at 0, one child process per switch, against the oracle"""
    env = dict(os.environ)
    env[switch] = "0"
    out = subprocess.run([sys.executable, "-c", SCRIPT % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))],
                         env=env, capture_output=True, text=True, timeout=600)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "ok", out.stdout[-2000:] + out.stderr[-3000:]
    seen = 0
    for line in lines[:-1]:
        log_n, i, inverse, coset, got = json.loads(line)
        d = child_inputs(log_n)[i]
        assert got == ref_digest(orc, log_n, d, inverse, coset), (switch, d, log_n, inverse, coset)
        seen += 1
    assert seen == sum(len(child_inputs(lg)) for lg in CHILD_LOGS) * len(VARIANTS)

"""The coset transforms of ntt.hip that round 2 (and the tests) use instead of 4n-point transforms: ntt_cosets_fwd (a polynomial of
up to 2n coefficients on the cosets w_4n^k <w_n>) against the entries i = k mod 4 of the C oracle's 4n-point transform, and
ntt_cosets_inv with the prover's recombination (cosets3_solve) as the round trip of polynomials of degree < 3n.  Both the lazy
9 x 29-bit transform and the 8 x 32-bit one (SWM_NTT_LAZY=0, read once per process: a subprocess)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGS = (4, 5, 10, 11, 12, 16, 20)


def _check(ctx, orc, log_n, seed):
    from pyref.prng import fr_array
    n = 1 << log_n
    threads = orc.lib.oracle_max_threads()
    full = orc.fr_to_mont(fr_array(4 * n, seed))
    # forward: n + 1 and 2n coefficients (and n, where nothing folds), several coset lists
    for ln in (n, n + 1, 2 * n):
        padded = np.zeros((4 * n, 4), dtype=np.uint64)
        padded[:ln] = full[:ln]
        big = orc.ntt(padded, log_n + 2, 0, 0, threads=threads)
        for ks in ([1, 2], [1, 2, 3], [0], [3, 0, 2, 1]):
            got = ctx.selftest_ntt_cosets(full[:ln], log_n, ks)
            for c, k in enumerate(ks):
                assert np.array_equal(got[c], big[k::4]), (log_n, ln, ks, k)
    # inverse: degree < 3n round trips (random, zero, only coefficient 3n - 1)
    top = np.zeros((3 * n, 4), dtype=np.uint64)
    top[3 * n - 1] = full[0]
    for coeffs in (full[:3 * n], np.zeros((3 * n, 4), dtype=np.uint64), top):
        padded = np.zeros((4 * n, 4), dtype=np.uint64)
        padded[:3 * n] = coeffs
        big = orc.ntt(padded, log_n + 2, 0, 0, threads=threads)
        evals = np.concatenate([big[k::4] for k in range(3)])
        assert np.array_equal(ctx.selftest_intt_cosets3(evals, log_n), coeffs), log_n


@pytest.fixture(scope="module")
def ctx():
    import simpleworks_amd as swm
    c = swm.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("log_n", LOGS)
def test_cosets_forward_and_inverse(ctx, log_n):
    _check(ctx, Oracle(), log_n, 4200 + log_n)


SCRIPT = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import simpleworks_amd as swm
from oracle_lib import Oracle
import test_gpu_cosets as T
ctx = swm.Context(0)
orc = Oracle()
for lg in T.LOGS:
    T._check(ctx, orc, lg, 4300 + lg)
ctx.close()
print("ok")
"""


def test_cosets_with_the_32_bit_limb_transform():
    env = dict(os.environ)
    env["SWM_NTT_LAZY"] = "0"
    out = subprocess.run([sys.executable, "-c", SCRIPT % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))],
                         env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-3000:]

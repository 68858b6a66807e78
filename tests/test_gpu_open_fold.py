"""The opening round's folded witnesses (marlin_prove.hip, open_combinations / SWM_OPEN_FOLD): under a committer key whose shifted powers
are a sub-range of its powers, a query point's shifted witness is added into the plain quotient at its offset and the point
costs ONE MSM job instead of two.  The proof bytes must not move, the job count must drop by exactly one per query point, and a
key with shifted powers on a table of their own must keep the two-job path.

The two-job path enqueues 15 jobs per proof at every size, by the code: round 1 w, z_A, z_B, mask; round 2 t, g_1 (plain and
shifted), h_1; round 3 g_2 (plain and shifted), h_2; openings: plain and shifted witness at beta and at gamma.  (The mask is
committed in pieces only for a caller-owned generator, which no case here uses.)"""
import hashlib
import os
import subprocess
import sys

import pytest

from oracle_lib import golden, h2i

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_JOB_CALLS = 15
# the -DSWM_OPEN_FOLD=0 build of the library (bash tools/buildvar.sh nofold -DSWM_OPEN_FOLD=0), when someone has built it
NOFOLD_LIB = os.path.join(ROOT, "build", "libswmarlin_nofold.so")


@pytest.fixture(scope="module")
def M():
    from simpleworks_amd import marlin
    return marlin


@pytest.fixture(scope="module")
def S():
    from simpleworks_amd import serialization
    return serialization


@pytest.fixture(scope="module")
def W():
    from simpleworks_amd import workloads
    return workloads


def _prove_counted(M, cs, pk, rng):
    ctx = M.default_context()
    ctx.profile_reset()
    proof = M.generate_proof(cs, pk, rng)
    ctx.profile()
    return proof, dict(ctx.last_work)


# msm_twins: the pairs (g_1, g_2: plain + shifted COMMITMENT) that shared a sort, as the two-job path counts them: none at 2^12
# (jobs too small for the table schedule's twin path), both pairs from 2^16 on.  The fold does not touch commitments.
@pytest.mark.parametrize("log_n,twins", [(12, 0), (16, 2), (20, 2)])
def test_same_bytes_fewer_jobs(M, S, W, log_n, twins):
    """2^12 and 2^16 run the single-stream schedule, 2^20 the pipelined one."""
    case = golden("marlin_large.json")["synthetic_2p%d" % log_n]
    rng = M.generate_rand()
    srs = M.generate_universal_srs(*case["srs"], rng)
    cs, public = W.synthetic_r1cs(case["num_constraints"], h2i(case["a"]), h2i(case["b"]))
    pk, vk = M.generate_proving_and_verifying_keys(srs, cs)
    proof, work = _prove_counted(M, cs, pk, rng)
    print("2^%d:" % log_n, work)
    assert S.serialize_proof(proof).hex() == case["proof"]
    assert work["msm_calls"] == TWO_JOB_CALLS - 2
    assert work["msm_twins"] == twins
    assert M.verify_proof(vk, public, proof, rng)
    pk.free()
    srs.free()


_FALLBACK_SCRIPT = r"""
import hashlib, sys
sys.path.insert(0, %r)
from simpleworks_amd import marlin as M, workloads as W, serialization as S
n = 1 << 12
srs = M.generate_universal_srs(2 * n, 2 * n, 2 * n, M.generate_rand())
cs, public = W.synthetic_r1cs(n, 15, 5)
pk, vk = M.generate_proving_and_verifying_keys(srs, cs)
print("sha", hashlib.sha256(S.serialize_proof(M.generate_proof(cs, pk, M.generate_rand()))).hexdigest())
"""


def test_larger_srs_keeps_the_two_job_path(M, S, W):
    """A key cut from an SRS larger than the circuit's degree has its shifted powers on a table of their own: nothing folds."""
    n = 1 << 12
    srs = M.generate_universal_srs(2 * n, 2 * n, 2 * n, M.generate_rand())
    cs, public = W.synthetic_r1cs(n, 15, 5)
    pk, vk = M.generate_proving_and_verifying_keys(srs, cs)
    proof, work = _prove_counted(M, cs, pk, M.generate_rand())
    print("larger SRS:", work)
    assert work["msm_calls"] == TWO_JOB_CALLS
    data = S.serialize_proof(proof)
    assert M.verify_proof(vk, public, S.deserialize_proof(data), M.generate_rand())
    bad = list(public)
    bad[0] = (bad[0] + 1) % M.R_MODULUS
    assert not M.verify_proof(vk, bad, S.deserialize_proof(data), M.generate_rand())
    pk.free()
    srs.free()
    if os.path.exists(NOFOLD_LIB):  # the same proof from the build without the fold
        out = subprocess.run([sys.executable, "-c", _FALLBACK_SCRIPT % ROOT], env=dict(os.environ, SWM_LIB_PATH=NOFOLD_LIB),
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        assert out.stdout.split("sha ")[1].split()[0] == hashlib.sha256(data).hexdigest()


@pytest.mark.parametrize("name", ["wide_K", "wide_H"])
def test_merged_vector_longer_than_the_plain_quotient(M, S, W, name):
    """The merged witness vector ends at the SRS degree D = max(3|H| - 1, 3|K| - 3) at both query points; the plain quotient has
    3|H| - 1 coefficients at beta (the mask) and fewer than 3|K| - 3 at gamma.  wide_K (|K| = 2|H|): the vector grows at both
    points; wide_H (|K| = |H| / 4): the shifted range lies inside the beta quotient and far above the gamma one.  Bytes of the
    Python model (tests/golden/gen_golden_open_fold.py), and two jobs fewer than the same circuit under a larger SRS."""
    case = golden("marlin_open_fold.json")[name]
    H, K, D = case["H"], case["K"], case["max_degree"]
    assert D == max(3 * H - 1, 3 * K - 3)
    assert (D > 3 * H - 1) == (name == "wide_K") and D > 3 * K - 4   # beta grows only for wide_K; gamma always
    cs = W.random_sparse_circuit(**case["circuit"])
    assert cs.is_satisfied()
    public = [h2i(x) for x in case["public_input"]]
    rng = M.generate_rand()
    srs = M.generate_universal_srs(*case["srs"], rng)
    assert srs.max_degree == D
    pk, vk = M.generate_proving_and_verifying_keys(srs, cs)
    assert S.serialize_verifying_key(vk).hex() == case["vk"]
    proof, work = _prove_counted(M, cs, pk, rng)
    assert S.serialize_proof(proof).hex() == case["proof"]
    assert M.verify_proof(vk, public, proof, rng)
    pk.free()
    srs.free()
    srs = M.generate_universal_srs(*[2 * v for v in case["srs"]], M.generate_rand())
    pk, vk = M.generate_proving_and_verifying_keys(srs, cs)
    proof2, work2 = _prove_counted(M, cs, pk, M.generate_rand())
    print(name, work, work2)
    assert M.verify_proof(vk, public, proof2, M.generate_rand())
    assert work["msm_calls"] == work2["msm_calls"] - 2
    pk.free()
    srs.free()


def test_sharded_three_ranks_golden_bytes(M, S, W):
    """Three thread-ranks with uneven shares, default (block-cyclic) split of every commitment, the merged witness vectors
    included: the golden bytes of the 2^17 proof on every rank."""
    from test_gpu_marlin import _run_sharded
    case = golden("marlin_large.json")["synthetic_2p17"]
    cs, public = W.synthetic_r1cs(case["num_constraints"], h2i(case["a"]), h2i(case["b"]))

    def build(ctx):
        rng = M.generate_rand()
        srs = M.generate_universal_srs(*case["srs"], rng, ctx=ctx)
        pk, vk = M.generate_proving_and_verifying_keys(srs, cs)
        srs.free()
        proof = M.generate_proof(cs, pk, rng)
        out = (S.serialize_verifying_key(vk).hex(), S.serialize_proof(proof).hex())
        pk.free()
        return out

    for vk_hex, proof_hex in _run_sharded(3, build):
        assert vk_hex == case["vk"]
        assert proof_hex == case["proof"]

"""GPU tests (-m gpu) of the prover's pieces that stopped computing what is already known (csrc/devops.cuh, csrc/marlin_prove.hip):
the division by (X - z) out of place (no copy in front, the source left alone, the buffer's tail cleared), polynomial
evaluation at the tile edges with extremal coefficients and points (the kernels every proof's evaluations and the openings'
values come from), and whole proofs over the shapes at which round 1 (no transform of x), round 3 (zero on
K) and the openings (combination written into the division's buffer) take their different paths.  Every expectation is Python
integers or the Python model's bytes, compared bit for bit."""
import random

import numpy as np
import pytest

import differential_model as D
from oracle_lib import R, golden, h2i, ints_to_limbs

pytestmark = pytest.mark.gpu

RM = (1 << 256) % R          # Montgomery factor of the memory format
Z_RANDOM = 0x0B5A2D3C4E5F60718293A4B5C6D7E8F90112233445566778899AABBCCDDEEFF1
POINTS = [0, 1, R - 1, Z_RANDOM]


@pytest.fixture(scope="module")
def ctx():
    import simpleworks_amd as swm
    c = swm.Context(0)
    yield c
    c.close()


def mont(vals):
    return ints_to_limbs([v % R * RM % R for v in vals], 4)


def _coeffs(kind, n, seed):
    rnd = random.Random(seed)
    return [0] * n if kind == "zero" else [R - 1] * n if kind == "r-1" else [rnd.randrange(R) for _ in range(n)]


def _synthetic_division(P, z):
    """[p(z)] + the quotient of p by (X - z): s[k] = P[k] + z s[k + 1]"""
    out, acc = [0] * len(P), 0
    for k in range(len(P) - 1, -1, -1):
        acc = (P[k] + z * acc) % R
        out[k] = acc
    return out


def _horner(c, x):
    acc = 0
    for v in reversed(c):
        acc = (acc * x + v) % R
    return acc


# ------------------------------------------------------------------------------------------------ division out of place
@pytest.mark.parametrize("n", [1, 2, 8191, 8192, 8193, 5 * 2048 + 1])
def test_division_out_of_place(ctx, n):
    """suffix_recurrence_from on both sides of the tiled threshold (8192): the copy kernel + in-place passes below it, the
    tiled passes reading the source above it; the buffer starts as bytes 0xFF and has n, n + 1 or n + 2049 elements (a tail
    inside the last tile, and one that needs workgroups of its own).  Value and quotient equal Python's synthetic division
    limb for limb, the tail is zero, the source is unchanged."""
    P = _coeffs("random", n, 1100 + n)
    p = mont(P)
    for z in POINTS:
        want = mont(_synthetic_division(P, z))
        for cap in (n, n + 1, n + 2049):
            out, src = ctx.selftest_div_linear_from(p, mont([z])[0], cap)
            assert np.array_equal(src, p), (n, cap, z)
            assert np.array_equal(out[:n], want), (n, cap, z)
            assert not out[n:].any(), (n, cap, z)


def test_division_out_of_place_extremal_coefficients(ctx):
    """all r - 1 and all zero coefficients through the tiled form (the lazy sums at their largest)"""
    n = 5 * 2048 + 1
    for kind in ("r-1", "zero"):
        P = _coeffs(kind, n, 0)
        p = mont(P)
        for z in (R - 1, Z_RANDOM):
            out, src = ctx.selftest_div_linear_from(p, mont([z])[0], n + 2049)
            assert np.array_equal(src, p)
            assert np.array_equal(out[:n], mont(_synthetic_division(P, z))), (kind, z)
            assert not out[n:].any()


# ------------------------------------------------------------------------------------------------ evaluation
EVAL_LENGTHS = [1, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 1]


@pytest.mark.parametrize("kind", ["r-1", "zero", "random"])
@pytest.mark.parametrize("n", EVAL_LENGTHS)
def test_evaluation_one_and_many(ctx, n, kind):
    """poly_eval (op 2) and poly_eval_many (op 3, the polynomial as one piece and cut in two) at x = 0, 1, r - 1, random: the
    canonical memory form of Python's Horner value, limb for limb"""
    P = _coeffs(kind, n, 1200 + n)
    p = mont(P)
    cut = n // 2
    for x in POINTS:
        xm = mont([x])[0]
        want = mont([_horner(P, x), _horner(P[:cut], x), _horner(P[cut:], x)])
        assert np.array_equal(ctx.selftest_poly_eval(p, xm), want[0]), (n, kind, x)
        got = ctx.selftest_poly_eval_many(p, [(0, n), (0, cut), (cut, n - cut)], xm)
        assert np.array_equal(got, want), (n, kind, x)


def test_evaluation_batch_mixes_lengths_1_and_4097(ctx):
    """one launch over pieces of 1 and 4097 coefficients (one tile beside two: the short piece's second workgroup leaves early)"""
    P = _coeffs("random", 4097 + 1 + 4097, 1300)
    p = mont(P)
    pieces = [(0, 4097), (4097, 1), (4098, 4097), (4097, 1)]
    for x in POINTS:
        got = ctx.selftest_poly_eval_many(p, pieces, mont([x])[0])
        assert np.array_equal(got, mont([_horner(P[o:o + ln], x) for o, ln in pieces])), x


def test_evaluation_three_levels(ctx):
    """4096^2 + 1 coefficients (three levels), non-zero at the level boundaries, at the random point"""
    n = 4096 * 4096 + 1
    rnd = random.Random(n)
    idx = sorted({0, 255, 256, 4095, 4096, 4096 * 4095, n - 4097, n - 2, n - 1})
    coef = [rnd.randrange(R) for _ in idx]
    p = np.zeros((n, 4), dtype=np.uint64)
    p[idx] = mont(coef)
    want = sum(c * pow(Z_RANDOM, i, R) for c, i in zip(coef, idx)) % R
    assert np.array_equal(ctx.selftest_poly_eval(p, mont([Z_RANDOM])[0]), mont([want])[0])


# ------------------------------------------------------------------------------------------------ proof bytes
def _fixture_cases():
    cases = {c["name"]: c for c in golden("differential.json")["cases"]}
    cases.update({c["name"]: c for c in golden("known_work.json")["cases"]})
    return cases


# name -> (|X|, |H|, |K|) of the padded system
CARRIERS = {"k_lt_h": (1, 64, 4), "in16": (32, 64, 64), "k_gt_h": (4, 32, 128), "k_8": (2, 16, 8), "k_eq_h": (4, 16, 16)}


@pytest.mark.parametrize("name", sorted(CARRIERS))
def test_proof_bytes_are_the_model_s(name):
    """Verifying key and proof equal the Python model's bytes and the proof is accepted.  Carriers (differential.json, and
    known_work.json for the shape it lacks): k_lt_h — instance length 1 (|X| = 1: x is a constant) and |K| = 4; in16 — instance
    length 17, |X| = 32 = |H| / 2; k_gt_h — |K| = 128 > |H| = 32; k_8 — |K| = 8, below the size from which round 3 lays f out by
    cosets (dense 4|K| domain); k_eq_h — |K| = 16, the first size on cosets."""
    from simpleworks_amd import marlin as M, serialization as S
    case = _fixture_cases()[name]
    X, H, K = CARRIERS[name]
    pow2 = lambda v: 1 << max(v - 1, 0).bit_length()  # noqa: E731
    assert (pow2(len(case["public_input"]) + 1), pow2(case["num_constraints"]), pow2(case["num_non_zero"])) == (X, H, K)
    cs = M.ConstraintSystem()
    public = D.emit(cs, case["params"])
    assert public == [h2i(x) for x in case["public_input"]]
    rng = M.generate_rand()
    srs = M.generate_universal_srs(*case["srs"], rng)
    pk = None
    try:
        pk, vk = M.generate_proving_and_verifying_keys(srs, cs)
        assert S.serialize_verifying_key(vk).hex() == case["vk"]
        proof = M.generate_proof(cs, pk, rng)
        assert S.serialize_proof(proof).hex() == case["proof"]
        assert M.verify_proof(vk, public, proof, M.generate_rand())
    finally:
        if pk is not None:
            pk.free()
        srs.free()

"""The general addition of the 29-bit domain (csrc/fq29.cuh: what the one-lane bucket stage runs on partial sums that stay in the
accumulation's limb form) routine by routine on the device, through ops 27 - 36 of swm_selftest_p28, on operands chosen limb for
limb.

Reference: the group law on Python integers (pyref.bls12_377) and the twisted Edwards map derived in tests/test_gpu_p28.py — never
an emulation of the code under test.  A result is judged on the Weierstrass point the device's back-map gives for it and on its
form: all four coordinates N (below p (1 + 2^-23)), T Z = X Y.  Operands come in every accepted form — N; X + kp for k < 3; Y + kp
for k < 2; T and Z in [p, p (1 + 2^-23)) — each on its own and together, on both operands, for P + Q, P + P, P + (-P), P + O and
O + O."""
import random

import numpy as np
import pytest

from pyref.bls12_377 import g1_add, g1_neg
from test_gpu_p28 import P, R384, jac_points, pack, unpack
from test_gpu_te29 import INV406, N_MAX, R406, check_acc, enc29, points

# (kx, ky, sliver): the accepted representatives of one operand
FORMS = [(0, 0, None), (1, 0, None), (2, 0, None), (0, 1, None), (2, 1, None), (0, 0, "T"), (0, 0, "Z"), (2, 1, "T"), (2, 1, "Z")]
KINDS = ("P + Q", "P + P", "P + (-P)", "P + O", "O + O")
IDENTITY = (0, R406, 0, R406)
_CACHE = {}


def pair_cases(seed=2941):
    """(raw a, raw b, A + B, kind, A, B): every pair of forms for every kind; O also as the slot te29_store_identity writes"""
    if "pairs" in _CACHE:
        return _CACHE["pairs"]
    rng = random.Random(seed)
    pts = points()
    cases = []
    for fa in FORMS:
        for fb in FORMS:
            for kind in KINDS:
                A, B = rng.sample(pts, 2)
                if kind == "P + P":
                    B = A
                elif kind == "P + (-P)":
                    B = g1_neg(A)
                elif kind == "P + O":
                    B = None
                elif kind == "O + O":
                    A = B = None
                a, b = enc29(A, rng, *fa), enc29(B, rng, *fb)
                if rng.random() < 0.5:          # either way round: the first operand's sum and difference are the normalised ones
                    a, b, A, B = b, a, B, A
                cases.append((a, b, g1_add(A, B), kind, A, B))
    for A in (pts[0], pts[7], None):
        cases.append((enc29(A, rng), IDENTITY, A, "P + O", A, None))
        cases.append((IDENTITY, enc29(A, rng, 2, 1), A, "P + O", None, A))
    cases.append((IDENTITY, IDENTITY, None, "O + O", None, None))
    _CACHE["pairs"] = cases
    return cases


def test_operands_on_the_host():
    """No device: every generated operand is in an accepted form and stands for its point's image; every form meets every form in
    every kind."""
    cases = pair_cases()
    assert len(cases) == len(FORMS) ** 2 * len(KINDS) + 7
    for a, b, want, kind, _, _ in cases:
        for raw in (a, b):
            assert raw[0] < 3 * P and raw[1] < 2 * P and raw[2] < N_MAX and raw[3] < N_MAX
            X, Y, T, Z = (v * INV406 % P for v in raw)
            assert T * Z % P == X * Y % P and Z != 0
    assert {c[3] for c in cases} == set(KINDS)
    for idx, pick in ((0, lambda raw: raw[0] >= 2 * P), (1, lambda raw: raw[1] >= P), (2, lambda raw: raw[2] >= P), (3, lambda raw: raw[3] >= P)):
        assert sum(1 for c in cases if pick(c[0])) >= 40 and sum(1 for c in cases if pick(c[1])) >= 40, idx


@pytest.fixture(scope="module")
def ctx():
    import simpleworks_amd as swm
    c = swm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sums(ctx):
    """te29_slot_add out of place on every pair: shared by the tests below, not changed by them"""
    cases = pair_cases()
    a, b = pack([c[0] for c in cases]), pack([c[1] for c in cases])
    out, _, jac = ctx.selftest_p28("te29_slot_add", a, b, backmap=True)
    return a, b, out, jac


@pytest.mark.gpu
def test_slot_add_every_form_and_kind(sums):
    """te29_slot_add: the reference's point and a result in form (N, T Z = X Y) for every pair of accepted forms and every kind"""
    _, _, out, jac = sums
    check_acc(out, jac, [c[2] for c in pair_cases()], "te29_slot_add")


@pytest.mark.gpu
def test_in_place_and_quad_give_the_same_limbs(ctx, sums):
    """dst == pa, dst == pq and the four-lane form: bit for bit the out-of-place result"""
    a, b, out, jac = sums
    for op in ("te29_slot_add_inplace_a", "te29_slot_add_inplace_q", "te29_quad_add"):
        got, _, gjac = ctx.selftest_p28(op, a, b, backmap=True)
        assert np.array_equal(got, out) and np.array_equal(gjac, jac), op


@pytest.mark.gpu
def test_self_is_doubling(ctx, sums):
    """pa == pq: 2 P for P in every form (the shift phase's step), the identity included; one lane and quad bit for bit"""
    a, b, _, _ = sums
    cases = pair_cases()
    for arr, which in ((a, 4), (b, 5)):
        wants = [g1_add(c[which], c[which]) for c in cases]
        one, _, jac = ctx.selftest_p28("te29_slot_add_self", arr, backmap=True)
        check_acc(one, jac, wants, "te29_slot_add_self")
        quad, _, jacq = ctx.selftest_p28("te29_quad_add_self", arr, backmap=True)
        assert np.array_equal(quad, one) and np.array_equal(jacq, jac)


@pytest.mark.gpu
def test_sync_form_with_lanes_sitting_out(ctx, sums):
    """te29_slot_add_sync with the barrier on: the lanes that take part give te29_slot_add's limbs, a slot whose lane sits out keeps
    the bytes it was filled with"""
    a, b, out, _ = sums
    n = out.shape[0]
    flags = np.array([(i * 7 + 3) % 5 != 0 for i in range(n)], dtype=np.uint32)
    got = ctx.selftest_p28("te29_slot_add_sync", a, b, flags)[0]
    on = flags != 0
    assert on.sum() and (~on).sum()
    assert np.array_equal(got[on], out[on])
    assert (got[~on].view(np.uint8) == 0xA5).all()


@pytest.mark.gpu
def test_identity_stores(ctx):
    """te29_store_identity and the quad form: (0 : 1 : 0 : 1) with Y = Z the constant ONE, standing for the point at infinity"""
    for op in ("te29_store_identity", "te29_quad_store_identity"):
        out, _, jac = ctx.selftest_p28(op, None, n=5, backmap=True)
        assert unpack(out) == [IDENTITY] * 5, op
        assert jac_points(jac) == [None] * 5, op


@pytest.mark.gpu
def test_store_384_equals_the_28_bit_store(ctx, sums):
    """te29_store_384 of operands in every accepted form and of sums: the canonical radix-2^384 coordinates, which are what
    te28_store_384 gives for the same point in the 28-bit domain (each coordinate times 2^-14: te29_to_slot's slot)."""
    a, b, out, _ = sums
    inv14 = pow(1 << 14, -1, P)
    for arr in (a, b, out):
        raws = unpack(arr)
        got = unpack(ctx.selftest_p28("te29_store_384", arr)[0])
        assert got == [tuple(v * INV406 * R384 % P for v in raw) for raw in raws]
        slots = pack([tuple(v * inv14 % P for v in raw) for raw in raws])
        assert got == unpack(ctx.selftest_p28("te_store_384", slots)[0])

"""The 29-bit limb form of the table rows and of msm_accumulate_te (csrc/fq29.cuh) routine by routine on the device, through ops
21 - 26 of swm_selftest_p28, on operands chosen limb for limb.

Reference: the group law on Python integers (pyref.bls12_377) and the twisted Edwards map derived in tests/test_gpu_p28.py as
tools/gen_constants.py derives it — never an emulation of the code under test.  A result is judged on the Weierstrass point the
device's back-map gives for it (out_jac) and on the documented form of the raw accumulator (fq29.cuh): four integers, a field
element times 2^406 each; after an addition every coordinate is N — below p (1 + 2^-23), hence all thirteen limbs below 2^29;
te29_from_row leaves X in (p, 3p), Y below 2p, T in N and Z the constant 2.  What te29_madd_row and te29_to_slot accept is that
same set: X + kp for k < 3 while below 3p, Y + kp for k < 2, T and Z in N (canonical, and in [p, p (1 + 2^-23)) with the
scaling solved for it) — each shift on its own and together.  The
epilogue's slot must be an N value of the 28-bit domain (below 2p, bits 364 and up below 2^15) that the existing te_slot_add
and te_store_384 ops take to the reference's point."""
import random

import numpy as np
import pytest

from pyref.bls12_377 import G1_GEN, R as R_ORDER, g1_add, g1_mul_fast, g1_neg
from test_gpu_p28 import P, R384, R392, jac_points, pack, subgroup_points, te_consts, to_te, unpack

M29 = (1 << 29) - 1
R406 = (1 << 406) % P
INV406 = pow(R406, -1, P)
N_MAX = P + (P >> 23)
_CACHE = {}


def points():
    """k G for k = 1 .. 48 and for 24 random k"""
    if "pts" not in _CACHE:
        rng = random.Random(2900)
        _CACHE["pts"] = subgroup_points() + [g1_mul_fast(G1_GEN, rng.randrange(1, R_ORDER)) for _ in range(24)]
    return _CACHE["pts"]


def row29_ints(pt):
    x, y = to_te(pt)
    return ((y - x) * R406 % P, (y + x) * R406 % P, 2 * te_consts()[2] * x * y * R406 % P)


def pack_rows29(pts):
    """table rows as the device reads them: 3 x (13 limbs of 29 bits + 3 zero words), n x 24 uint64"""
    w = np.array([[(v >> (29 * i)) & M29 if i < 13 else 0 for v in row29_ints(pt) for i in range(16)] for pt in pts], dtype=np.uint32)
    return w.view(np.uint64).reshape(len(pts), 24).copy()


def enc29(pt, rng, kx=0, ky=0, sliver=None):
    """a raw accumulator of the 29-bit domain: (l x, l y, l x y, l) 2^406 mod p, X + kx p (while below 3p), Y + ky p.  sliver
    "T" / "Z": that coordinate in the part of N above p — the scaling l is solved so that its residue is below p / 2^23, and p is
    added (the identity has T = 0: its T becomes p itself)."""
    x, y = to_te(pt)
    lam = rng.randrange(1, P)
    if sliver:
        small = rng.randrange(1, P >> 23)
        den = R406 if sliver == "Z" or pt is None else x * y * R406
        lam = small * pow(den, -1, P) % P
    X, Y, T, Z = (v * lam * R406 % P for v in (x, y, x * y, 1))
    if sliver == "T":
        T += P
    if sliver == "Z":
        Z += P
    assert T < N_MAX and Z < N_MAX
    return (X + kx * P, Y + ky * P, T, Z)


def check_acc(out, jac, wants, what, after_addition=True):
    raws, pts = unpack(out), jac_points(jac)
    assert len(raws) == len(pts) == len(wants)
    for i, (raw, got, want) in enumerate(zip(raws, pts, wants)):
        if after_addition:
            assert all(v < N_MAX for v in raw), (what, i, "form")
        else:
            assert P < raw[0] < 3 * P and raw[1] < 2 * P and raw[2] < N_MAX and raw[3] == 2 * R406 % P, (what, i, "form")
        X, Y, T, Z = (v * INV406 % P for v in raw)
        assert T * Z % P == X * Y % P, (what, i, "T Z != X Y")
        assert got == want, (what, i)


def madd_cases(seed=2902):
    """(acc raw, point of the row, neg, acc +- point)"""
    rng = random.Random(seed)
    pts = points()
    cases = []
    for kx, ky in ((0, 0), (1, 0), (2, 0), (0, 1), (2, 1), (1, 1)):
        for i in range(48):
            A, B = rng.sample(pts, 2)
            if i % 8 == 4:
                B = A                 # the row of the accumulator's own point: P + P (neg off), P + (-P) (neg on)
            if i % 8 == 5:
                B = g1_neg(A)         # and the other way round
            if i % 8 == 6:
                A = None              # O + P
            if i % 8 == 7:
                B = None              # P + O: the identity row (1, 1, 0)
            neg = (i >> 3) & 1
            cases.append((enc29(A, rng, kx, ky), B, neg, g1_add(A, g1_neg(B) if neg else B)))
    for sliver in ("T", "Z"):             # T, Z in [p, p (1 + 2^-23)): the rest of N, alone and with the X and Y shifts
        for i in range(24):
            A, B = rng.sample(pts, 2)
            if i % 8 == 6:
                A = None
            kx, ky = ((0, 0), (2, 1))[i & 1]
            neg = (i >> 1) & 1
            cases.append((enc29(A, rng, kx, ky, sliver), B, neg, g1_add(A, g1_neg(B) if neg else B)))
    return cases


def test_operands_on_the_host():
    """No device: the generated accumulators are in the accepted form and stand for their points; the 29-bit row of the identity."""
    for a, B, neg, want in madd_cases():
        assert a[0] < 3 * P and a[1] < 2 * P and a[2] < N_MAX and a[3] < N_MAX
        X, Y, T, Z = (v * INV406 % P for v in a)
        assert T * Z % P == X * Y % P
    assert row29_ints(None) == (R406, R406, 0)
    assert any(c[3] is None for c in madd_cases()) and len(madd_cases()) == 336
    assert sum(1 for c in madd_cases() if c[0][2] >= P) == 24 and sum(1 for c in madd_cases() if c[0][3] >= P) == 24


@pytest.fixture(scope="module")
def ctx():
    import simpleworks_amd as swm
    c = swm.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_rows29_and_from_row(ctx):
    """msm_te_convert in the 29-bit form on a count that is no multiple of its chunk, identities inside a chunk: every row
    (y - x, y + x, 2dxy) 2^406 canonical in thirteen limbs with words 13 - 15 zero, equal to the Python map; *bad for the
    order-two point only; te29_from_row of a device row, both signs, one lane and quad bit for bit, maps back to +-the point."""
    pts = list(points()[:48 + 13])
    for i in (3, 17, 18, 36, 60):
        pts[i] = None
    n = len(pts)
    mont = pack([(0, 0, 0, 0) if pt is None else (pt[0] * R384 % P, pt[1] * R384 % P, 0, 0) for pt in pts])[:, :12].copy()
    rows, status, _ = ctx.selftest_p28("rows29", mont)
    assert status[0] == 0
    assert np.array_equal(rows, pack_rows29(pts))
    assert not rows.view(np.uint32).reshape(n, 3, 16)[:, :, 13:].any()
    with_t2 = mont.copy()
    with_t2[20] = pack([((P - 1) * R384 % P, 0, 0, 0)])[0, :12]
    rows2, status2, _ = ctx.selftest_p28("rows29", with_t2)
    assert status2[0] != 0
    keep_rows = [i for i in range(n) if i != 20]
    assert np.array_equal(rows2[keep_rows], rows[keep_rows])
    for neg in (0, 1):
        flags = np.full(n, neg, dtype=np.uint32)
        one, _, jac = ctx.selftest_p28("te29_from_row", rows, flags=flags, backmap=True)
        check_acc(one, jac, [g1_neg(pt) if neg else pt for pt in pts], "te29_from_row", after_addition=False)
        quad, _, jacq = ctx.selftest_p28("te29_quad_from_row", rows, flags=flags, backmap=True)
        assert np.array_equal(quad, one) and np.array_equal(jacq, jac)


@pytest.mark.gpu
def test_madd_row_one_lane_and_quad(ctx):
    """te29_madd_row and te29_quad_madd_row: acc +- the row's point with the accumulator in every accepted representative, each
    shift alone and both together; P + P, P + (-P), O + P and P + O through the unified law; the quad form bit for bit."""
    cases = madd_cases()
    a, rows = pack([c[0] for c in cases]), pack_rows29([c[1] for c in cases])
    flags = np.array([c[2] for c in cases], dtype=np.uint32)
    one, _, jac = ctx.selftest_p28("te29_madd_row", a, rows, flags, backmap=True)
    check_acc(one, jac, [c[3] for c in cases], "te29_madd_row")
    quad, _, jacq = ctx.selftest_p28("te29_quad_madd_row", a, rows, flags, backmap=True)
    assert np.array_equal(quad, one) and np.array_equal(jacq, jac)


@pytest.mark.gpu
def test_chains_of_64_steps(ctx):
    """A segment as the kernel runs it: te29_from_row, then 64 te29_madd_row / te29_quad_madd_row steps with every output fed back
    in: the form after every step, one lane and quad bit for bit, the group element at steps 16, 32 and 64."""
    pts = points()
    lanes = 64
    start = [pts[(5 * i) % len(pts)] for i in range(lanes)]
    steps = [[pts[(7 * i + 11 * j) % len(pts)] for i in range(lanes)] for j in range(64)]
    sflags = np.array([i & 1 for i in range(lanes)], dtype=np.uint32)
    acc = ctx.selftest_p28("te29_from_row", pack_rows29(start), flags=sflags)[0]
    accq = acc
    want = [g1_neg(pt) if fl else pt for pt, fl in zip(start, sflags)]
    for j, qs in enumerate(steps):
        flags = np.array([(i * (j + 1) >> 1) & 1 for i in range(lanes)], dtype=np.uint32)
        rows = pack_rows29(qs)
        acc, _, jac = ctx.selftest_p28("te29_madd_row", acc, rows, flags, backmap=True)
        accq = ctx.selftest_p28("te29_quad_madd_row", accq, rows, flags)[0]
        assert np.array_equal(acc, accq), j
        want = [g1_add(w, g1_neg(pt) if fl else pt) for w, pt, fl in zip(want, qs, flags)]
        if j + 1 in (16, 32, 64):
            check_acc(acc, jac, want, "te29 chain step %d" % (j + 1))
        else:
            assert all(v < N_MAX for raw in unpack(acc) for v in raw), j


@pytest.mark.gpu
def test_epilogue_slot_feeds_the_bucket_stage(ctx):
    """te29_to_slot on accumulators in every accepted representative, results of te29_from_row and of an addition among them:
    each slot is the coordinate times 2^-14 mod p as an N value of the 28-bit domain; te_slot_add of two such slots and
    te_store_384 of one give the reference's point and residues."""
    rng = random.Random(2903)
    cases = madd_cases()
    raws = [c[0] for c in cases]
    a = pack(raws)
    rows = pack_rows29([c[1] for c in cases])
    flags = np.array([c[2] for c in cases], dtype=np.uint32)
    summed = ctx.selftest_p28("te29_madd_row", a, rows, flags)[0]
    first = ctx.selftest_p28("te29_from_row", rows, flags=flags)[0]
    for what, acc, wants in (("given", a, None), ("after an addition", summed, [c[3] for c in cases]),
                             ("first of a segment", first, [g1_neg(c[1]) if c[2] else c[1] for c in cases])):
        slot, _, jac = ctx.selftest_p28("te29_to_slot", acc, backmap=True)
        inv14 = pow(1 << 14, -1, P)
        for i, (raw, got) in enumerate(zip(unpack(acc), unpack(slot))):
            for v, s in zip(raw, got):
                assert s < 2 * P and s >> 364 < 1 << 15 and s % P == v * inv14 % P, (what, i)
        if wants is not None:
            assert jac_points(jac) == wants, what
            other = [rng.choice(points()) for _ in wants]
            b = pack([tuple(v * lam * R392 % P for v in (x, y, x * y, 1))
                      for (x, y), lam in ((to_te(pt), rng.randrange(1, P)) for pt in other)])
            _, _, jsum = ctx.selftest_p28("te_slot_add", slot, b, backmap=True)
            assert jac_points(jsum) == [g1_add(w, o) for w, o in zip(wants, other)], what
        inv256 = pow(256, -1, P)
        st = unpack(ctx.selftest_p28("te_store_384", slot)[0])
        assert st == [tuple(v * inv256 % P for v in raw) for raw in unpack(slot)], what

"""The MSM's 28-bit point layer (csrc/fq28.cuh, the streamed forms and madd28 of csrc/msm_points.cuh, msm_te_convert of csrc/msm_table.hip) routine by routine on
the device, through swm_selftest_p28, on operands chosen limb for limb.

Reference: the group law on Python integers (pyref.bls12_377: g1_add, g1_neg, fq_sqrt) — never the 32-bit device adders, never an
emulation of the code under test.  The twisted Edwards map and the table rows are derived here as tools/gen_constants.py derives
them (the smaller square root of 3 and of -a'), not read from constants_gen.h; a twisted Edwards RESULT is judged on the
Weierstrass point the device's own back-map (te28_store_384, g1te_to_xyzz, g1_to_jacobian) gives for it.

What a raw XYZZ result must satisfy (fq28.cuh, "point form"): x < 18p, y < 6p, zz and zzz < 2p; limbs below 2^28, which the packed
slot gives by construction, and the top limb (bits 364 ..) within what the next SPREAD subtraction borrows (x: SPREAD32's, y:
SPREAD8's, zz / zzz: below 2^15); the identity if and only if the zz slot is the INTEGER 0 — a zz that is a non-zero multiple of p
is neither.  Decoded (x = X / ZZ, y = Y / ZZZ, ZZ^3 = ZZZ^2) it must be the reference's group element.  A twisted Edwards result
at rest has every raw coordinate below 2p (form N); the one documented exception is te28_from_row, whose X lies in (p, 3p).

Operands: subgroup points k G in scaled projective form (l^2 X, l^3 Y, l^2, l^3), every coordinate in every representative the
comments allow (x + kp for k < 18, y + kp for k < 6, zz / zzz + p), each shift on its own and all together; identity operands;
q = a and q = -a in another scaling and representative; curve points outside the subgroup, and the point of order two (q - 1, 0)
with its y slot holding 0, p, ..., 5p (XYZZ ops only: the twisted Edwards law is used for subgroup points alone).  The generators
need no device: test_generators_and_reference_on_the_host holds them to the bounds above and the reference to itself.
"""
import random

import numpy as np
import pytest

from pyref.bls12_377 import G1_GEN, Q, fq_sqrt, g1_add, g1_is_on_curve, g1_neg

P = Q
M28 = (1 << 28) - 1
R392, R384 = (1 << 392) % P, (1 << 384) % P
INV392, INV384 = pow(R392, -1, P), pow(R384, -1, P)
T2 = (P - 1, 0)                               # the point of order two of y^2 = x^3 + 1
XYZZ_BOUND = (18, 6, 2, 2)                    # value of x, y, zz, zzz below this many p
XYZZ_TOP = ((32 * P >> 364) - 1, (8 * P >> 364) - 1, (1 << 15) - 1, (1 << 15) - 1)   # largest legal top limb
STATS = {"made": 0, "dropped": 0}


# ------------------------------------------------------------------------------------------------ raw slots
def pack(raws):
    """4-tuples of integers < 2^384 -> n x 24 uint64"""
    buf = b"".join(v.to_bytes(48, "little") for raw in raws for v in raw)
    return np.frombuffer(buf, dtype=np.uint64).reshape(len(raws), 24).copy()


def unpack(arr):
    b = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [tuple(int.from_bytes(b[(4 * i + c) * 48:(4 * i + c + 1) * 48], "little") for c in range(4)) for i in range(len(b) // 192)]


def legal_xyzz(raw):
    return all(v < k * P and (v >> 364) <= top for v, k, top in zip(raw, XYZZ_BOUND, XYZZ_TOP))


def keep(raw):
    """The discard rule of the generators: a representative outside the documented form is dropped (and counted)."""
    STATS["made"] += 1
    if not legal_xyzz(raw):
        STATS["dropped"] += 1
        return False
    return True


def enc_xyzz(pt, rng, shifts=None):
    """An affine point (None: the identity) as a raw XYZZ slot set: random scaling, the coordinates shifted by shifts[c] * p."""
    kx, ky, kzz, kzzz = shifts if shifts is not None else (rng.randrange(18), rng.randrange(6), rng.randrange(2), rng.randrange(2))
    if pt is None:  # zz exactly 0; x, y anything in form; zzz zero (p28_identity) or any N value
        return (rng.randrange(P) + kx * P, rng.randrange(P) + ky * P, 0, (rng.randrange(P) + kzzz * P) * rng.randrange(2))
    lam = rng.randrange(1, P)
    l2 = lam * lam % P
    l3 = l2 * lam % P
    return tuple(v * R392 % P + k * P for v, k in zip((pt[0] * l2, pt[1] * l3, l2, l3), (kx, ky, kzz, kzzz)))


def enc_xyzz_full(pt, rng, coord, top):
    """A finite point with slot `coord` (0: x, 2: zz) holding top limb `top` above thirteen FULL limbs: the scaling is solved for
    (l^2 = that value over x, or that value itself), so only values whose l^2 is a square have such a form — None otherwise.  The
    candidate may lie above the bound of its coordinate: keep() then drops it."""
    full = (top << 364) | ((1 << 364) - 1)
    l2 = full * INV392 % P * (pow(pt[0], -1, P) if coord == 0 else 1) % P
    lam = fq_sqrt(l2)
    if lam is None:
        return None
    l3 = l2 * lam % P
    sh = (rng.randrange(18), rng.randrange(6), rng.randrange(2), rng.randrange(2))
    raw = [v * R392 % P + k * P for v, k in zip((pt[0] * l2, pt[1] * l3, l2, l3), sh)]
    assert full % P == raw[coord] % P
    raw[coord] = full
    return tuple(raw)


def decode_xyzz(raw):
    X, Y, ZZ, ZZZ = raw
    if ZZ == 0:
        return None
    assert ZZ % P != 0, "zz is a non-zero multiple of p: not the identity's exact zero, not a finite point"
    zz, zzz = ZZ * INV392 % P, ZZZ * INV392 % P
    assert pow(zz, 3, P) == zzz * zzz % P, "ZZ^3 != ZZZ^2"
    return (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)


def check_xyzz(out, wants, what):
    raws = unpack(out)
    assert len(raws) == len(wants)
    for i, (raw, want) in enumerate(zip(raws, wants)):
        assert legal_xyzz(raw), (what, i, "form", [hex(v) for v in raw])
        assert decode_xyzz(raw) == want, (what, i)   # want None <=> zz slot exactly 0


# ------------------------------------------------------------------------------------------------ points
_CACHE = {}


def subgroup_points():
    if "sub" not in _CACHE:
        acc, out = None, []
        for _ in range(48):
            acc = g1_add(acc, G1_GEN)
            out.append(acc)
        _CACHE["sub"] = out
    return _CACHE["sub"]


def small_x_points():
    """curve points with small x: cofactor not cleared (the base set of test_msm_bases_outside_the_prime_order_subgroup)"""
    if "small" not in _CACHE:
        out, x = [], 2
        while len(out) < 8:
            y = fq_sqrt((x * x * x + 1) % P)
            if y is not None:
                out.append((x, y))
            x += 1
        _CACHE["small"] = out
    return _CACHE["small"]


def xyzz_pair_cases(seed=2801):
    """(a raw, b raw, a + b) for the binary XYZZ ops"""
    rng = random.Random(seed)
    sub, small = subgroup_points(), small_x_points()
    cases = []

    def case(A, B, sa=None, sb=None):
        a, b = enc_xyzz(A, rng, sa), enc_xyzz(B, rng, sb)
        if keep(a) and keep(b):
            cases.append((a, b, g1_add(A, B)))

    for coord, kmax in enumerate(XYZZ_BOUND):          # every shift of every coordinate, on either operand, the rest random
        for k in range(kmax):
            for side in (0, 1):
                for rest in (0, None, None, None, None, None, None, None):
                    A, B = rng.sample(sub, 2)
                    sh = [0 if rest == 0 else rng.randrange(m) for m in XYZZ_BOUND]
                    sh[coord] = k
                    case(A, B, tuple(sh) if side == 0 else None, tuple(sh) if side == 1 else None)
    for coord in (0, 2):                               # thirteen full limbs under the largest top limbs the bound allows
        for top in range(XYZZ_BOUND[coord] * P >> 364, (XYZZ_BOUND[coord] * P >> 364) - 6, -1):
            for side in (0, 1):
                for _ in range(4):
                    A, B = rng.sample(sub, 2)
                    a = enc_xyzz_full(A, rng, coord, top)
                    if a is not None and keep(a):
                        b = enc_xyzz(B, rng)
                        cases.append((a, b, g1_add(A, B)) if side == 0 else (b, a, g1_add(B, A)))
    top = tuple(k - 1 for k in XYZZ_BOUND)
    for _ in range(8):
        A, B = rng.sample(sub, 2)
        case(A, B, top, top)
        case(A, B, (0, 0, 0, 0), (0, 0, 0, 0))
    for _ in range(1200):
        A, B = rng.sample(sub, 2)
        case(A, B)
    for _ in range(12):                                # identity operands
        case(None, rng.choice(sub))
        case(rng.choice(sub), None)
        case(None, None)
    for i in range(120):                               # q = a and q = -a: another scaling, another representative
        A = rng.choice(sub)
        sa, sb = ((top, (0, 0, 0, 0)), ((0, 0, 0, 0), top), (top, top), (None, None))[i % 4]
        case(A, A, sa, sb)
        case(A, g1_neg(A), sa, sb)
    for S in small:                                    # outside the subgroup
        case(S, rng.choice(small))
        case(S, S)
        case(S, g1_neg(S))
        case(S, rng.choice(sub))
        case(rng.choice(sub), S)
    for k in range(6):                                 # the point of order two, y slot = k p
        for B in (rng.choice(sub), rng.choice(small), None):
            case(T2, B, (rng.randrange(18), k, rng.randrange(2), rng.randrange(2)))
            case(B, T2, None, (rng.randrange(18), k, rng.randrange(2), rng.randrange(2)))
        for k2 in (0, 1, 5):                           # T2 + T2 = O through the doubling
            case(T2, T2, (rng.randrange(18), k, 0, 1), (rng.randrange(18), k2, 1, 0))
        A = rng.choice(sub)                            # a + q = T2
        case(A, g1_add(T2, g1_neg(A)))
    return cases


def xyzz_single_cases(seed=2802):
    """(a raw, a) for the doublings and the store"""
    rng = random.Random(seed)
    sub, small = subgroup_points(), small_x_points()
    cases = []

    def case(A, sa=None):
        a = enc_xyzz(A, rng, sa)
        if keep(a):
            cases.append((a, A))

    for coord, kmax in enumerate(XYZZ_BOUND):
        for k in range(kmax):
            for rest in (0,) + (None,) * 15:
                sh = [0 if rest == 0 else rng.randrange(m) for m in XYZZ_BOUND]
                sh[coord] = k
                case(rng.choice(sub), tuple(sh))
    for coord in (0, 2):
        for top in range(XYZZ_BOUND[coord] * P >> 364, (XYZZ_BOUND[coord] * P >> 364) - 6, -1):
            for _ in range(8):
                A = rng.choice(sub)
                a = enc_xyzz_full(A, rng, coord, top)
                if a is not None and keep(a):
                    cases.append((a, A))
    for _ in range(1500):
        case(rng.choice(sub))
    for _ in range(8):
        case(rng.choice(sub), tuple(k - 1 for k in XYZZ_BOUND))
        case(None)
    for S in small:
        case(S)
    for k in range(6):
        for _ in range(4):
            case(T2, (rng.randrange(18), k, rng.randrange(2), rng.randrange(2)))
    return cases


# ------------------------------------------------------------------------------------------------ twisted Edwards model
def _root(a):
    r = fq_sqrt(a % P)
    return min(r, P - r)


def te_consts():
    """s, f, d of the map of csrc/g1.cuh, derived as tools/gen_constants.py derives them"""
    if "te" not in _CACHE:
        s = pow(_root(3), -1, P)
        A, B = -3 * s % P, s
        a1, d1 = (A + 2) * pow(B, -1, P) % P, (A - 2) * pow(B, -1, P) % P
        _CACHE["te"] = (s, _root(-a1), d1 * pow(-a1, -1, P) % P)
    return _CACHE["te"]


def to_te(pt):
    s, f, _ = te_consts()
    if pt is None:
        return (0, 1)
    u = s * (pt[0] + 1) % P
    return (f * (pt[0] + 1) * pow(pt[1], -1, P) % P, (u - 1) * pow(u + 1, -1, P) % P)


def te_row_ints(pt):
    x, y = to_te(pt)
    return ((y - x) * R392 % P, (y + x) * R392 % P, 2 * te_consts()[2] * x * y * R392 % P)


def pack_rows(pts):
    """table rows of the points as the device reads them: 3 x (14 limbs of 28 bits + 2 zero words), n x 24 uint64"""
    w = np.array([[(v >> (28 * i)) & M28 if i < 14 else 0 for v in te_row_ints(pt) for i in range(16)] for pt in pts], dtype=np.uint32)
    return w.view(np.uint64).reshape(len(pts), 24).copy()


def enc_te(pt, rng, shifts=None, x_reps=2):
    """extended coordinates (l x, l y, l x y, l) of the image, each + k p (k < 2; X: k < x_reps)"""
    x, y = to_te(pt)
    lam = rng.randrange(1, P)
    sh = shifts if shifts is not None else (rng.randrange(x_reps), rng.randrange(2), rng.randrange(2), rng.randrange(2))
    return tuple(v * lam * R392 % P + k * P for v, k in zip((x, y, x * y, 1), sh))


def jac_points(jac):
    out = []
    for row in np.asarray(jac, dtype=np.uint64).reshape(-1, 18):
        X, Y, Z = (int.from_bytes(row[6 * c:6 * c + 6].tobytes(), "little") for c in range(3))
        if Z == 0:
            out.append(None)
            continue
        zi = pow(Z * INV384 % P, -1, P)
        out.append((X * INV384 * zi * zi % P, Y * INV384 * zi * zi * zi % P))
    return out


def check_te(out, jac, wants, what, x_bound=2):
    raws, pts = unpack(out), jac_points(jac)
    assert len(raws) == len(pts) == len(wants)
    for i, (raw, got, want) in enumerate(zip(raws, pts, wants)):
        assert raw[0] < x_bound * P and all(v < 2 * P for v in raw[1:]), (what, i, "form")
        assert got == want, (what, i)


def te_pair_cases(seed=2803):
    """(a raw, b raw, a + b, a): subgroup points only, every N representative — and X also in the (p, 3p) form that te28_from_row
    leaves and a one-entry segment hands to the bucket stage — the exceptional pairs of a non-unified law included"""
    rng = random.Random(seed)
    sub = subgroup_points()
    cases = []
    for coord in range(4):
        for k in (0, 1, 2) if coord == 0 else (0, 1):
            for side in (0, 1):
                for _ in range(16):
                    A, B = rng.sample(sub, 2)
                    sh = [rng.randrange(2) for _ in range(4)]
                    sh[coord] = k
                    sa, sb = (tuple(sh), None) if side == 0 else (None, tuple(sh))
                    cases.append((enc_te(A, rng, sa), enc_te(B, rng, sb), g1_add(A, B), A))
    for _ in range(1200):
        A, B = rng.sample(sub, 2)
        cases.append((enc_te(A, rng, x_reps=3), enc_te(B, rng, x_reps=3), g1_add(A, B), A))
    for i in range(64):
        A = rng.choice(sub)
        sh = ((0, 0, 0, 0), (1, 1, 1, 1), (2, 1, 1, 1), None)[i % 4]
        cases.append((enc_te(A, rng, sh), enc_te(A, rng, sh), g1_add(A, A), A))       # doubling
        cases.append((enc_te(A, rng, sh), enc_te(g1_neg(A), rng, sh), None, A))       # P + (-P)
        cases.append((enc_te(None, rng, sh), enc_te(A, rng, sh), A, None))            # identity operands
        cases.append((enc_te(A, rng, sh), enc_te(None, rng, sh), A, A))
        cases.append((enc_te(None, rng, sh), enc_te(None, rng, sh), None, None))
    return cases


def te_row_cases(seed=2804):
    """(acc raw, point of the row, neg, acc +- point): the accumulator also in the (p, 3p) form te28_from_row leaves its X in"""
    rng = random.Random(seed)
    sub = subgroup_points()
    cases = []
    for i in range(2000):
        A, B = rng.sample(sub, 2)
        if i % 8 == 5:
            B = A                 # the row of the accumulator's own point: doubling (neg off) or cancellation (neg on)
        if i % 8 == 6:
            A = None
        if i % 8 == 7:
            B = None              # the identity row (1, 1, 0)
        neg = (i >> 3) & 1
        cases.append((enc_te(A, rng, x_reps=3), B, neg, g1_add(A, g1_neg(B) if neg else B)))
    return cases


# ------------------------------------------------------------------------------------------------ host-only checks
def test_generators_and_reference_on_the_host():
    """No device: every generated operand is in the documented form, at most 10 % of what the generators made was dropped (the
    full-limb candidates above their bound are: the rule does fire),
    decode(encode(P)) = P for every representative, and the twisted Edwards model is a homomorphism onto its curve."""
    STATS["made"] = STATS["dropped"] = 0
    pairs, singles = xyzz_pair_cases(), xyzz_single_cases()
    assert STATS["made"] >= 5000 and 0 < STATS["dropped"] <= STATS["made"] // 10, STATS
    assert len(pairs) >= 2000 and len(singles) >= 2000 and len(te_pair_cases()) >= 1500 and len(te_row_cases()) >= 2000
    top_x, top_zz = 18 * P >> 364, 2 * P >> 364
    full = lambda v: v & ((1 << 364) - 1) == (1 << 364) - 1
    assert any(full(a[0]) and a[0] >> 364 == top_x - 1 for a, _ in singles) and any(full(a[2]) and a[2] >> 364 == top_zz - 1 for a, _ in singles)
    assert any(full(c[0][0]) or full(c[1][0]) for c in pairs) and any(full(c[0][2]) or full(c[1][2]) for c in pairs)
    for a, b, want in pairs:
        assert legal_xyzz(a) and legal_xyzz(b) and g1_is_on_curve(want)
        assert g1_add(decode_xyzz(a), decode_xyzz(b)) == want
    for a, want in singles:
        assert legal_xyzz(a) and decode_xyzz(a) == want
    rng = random.Random(1)
    for pt in subgroup_points()[:6] + small_x_points()[:3] + [T2, None]:
        for kx in range(18):
            for ky in range(6):
                for kz in range(4):
                    raw = enc_xyzz(pt, rng, (kx, ky, kz & 1, kz >> 1))
                    assert legal_xyzz(raw) and decode_xyzz(raw) == pt and np.array_equal(pack(unpack(pack([raw]))), pack([raw]))
    assert [enc_xyzz(T2, rng, (0, k, 0, 0))[1] for k in range(6)] == [k * P for k in range(6)]
    # the twisted Edwards model: images lie on -x^2 + y^2 = 1 + d x^2 y^2 and add as the Weierstrass points do
    s, f, d = te_consts()
    sub = subgroup_points()
    for A, B in ((sub[0], sub[1]), (sub[4], sub[4]), (sub[7], g1_neg(sub[7])), (None, sub[3])):
        (x1, y1), (x2, y2), (x3, y3) = to_te(A), to_te(B), to_te(g1_add(A, B))
        assert (-x1 * x1 + y1 * y1 - 1 - d * x1 * x1 * y1 * y1) % P == 0
        den = d * x1 * x2 * y1 * y2 % P
        assert (x1 * y2 + y1 * x2) * pow(1 + den, -1, P) % P == x3 and (y1 * y2 + x1 * x2) * pow(1 - den, -1, P) % P == y3
    assert te_row_ints(None) == (R392, R392, 0)
    for a, b, want, _ in te_pair_cases():
        assert a[0] < 3 * P and b[0] < 3 * P and all(v < 2 * P for v in a[1:] + b[1:]) and g1_is_on_curve(want)
    for a, B, neg, want in te_row_cases():
        assert a[0] < 3 * P and all(v < 2 * P for v in a[1:])
        X, Y, T, Z = (v * INV392 % P for v in a)
        assert T * Z % P == X * Y % P


# ------------------------------------------------------------------------------------------------ device
@pytest.fixture(scope="module")
def ctx():
    import simpleworks_amd as swm
    c = swm.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_xyzz_additions(ctx):
    """p28_add<MulInline>, p28_add<MulFenced>, p28_slot_add with dst apart and dst == pa: the sum as a group element and the
    documented form for every representative and edge; the aliased form equals the other one slot for slot."""
    cases = xyzz_pair_cases()
    a, b, wants = pack([c[0] for c in cases]), pack([c[1] for c in cases]), [c[2] for c in cases]
    outs = {}
    for op in ("add", "add_ool", "slot_add", "slot_add_inplace"):
        outs[op] = ctx.selftest_p28(op, a, b)[0]
        check_xyzz(outs[op], wants, op)
    assert np.array_equal(outs["slot_add"], outs["slot_add_inplace"])


@pytest.mark.gpu
def test_xyzz_doublings(ctx):
    """p28_dbl and p28_slot_dbl, the point of order two included: its double is the identity with the zz slot EXACTLY 0 whatever
    multiple of p its y slot holds."""
    cases = xyzz_single_cases()
    a, wants = pack([c[0] for c in cases]), [g1_add(c[1], c[1]) for c in cases]
    assert sum(1 for c in cases if c[1] == T2) >= 24 and all(w is None for c, w in zip(cases, wants) if c[1] == T2)
    for op in ("dbl", "slot_dbl"):
        check_xyzz(ctx.selftest_p28(op, a)[0], wants, op)


@pytest.mark.gpu
def test_xyzz_sum_of_order_two_is_doubled(ctx):
    """a + q = (q - 1, 0) by the generic addition — whose mul2 leaves y as the device leaves it — and that result doubled and added
    to itself: the identity, exactly, and the identity then behaves as one (O + P = P)."""
    rng = random.Random(2805)
    sub = subgroup_points()
    A = [sub[i] for i in range(0, 48, 2)]
    a = pack([enc_xyzz(pt, rng) for pt in A])
    b = pack([enc_xyzz(g1_add(T2, g1_neg(pt)), rng) for pt in A])
    c = pack([enc_xyzz(pt, rng) for pt in A])
    for add, dbl in (("add", "dbl"), ("add_ool", "dbl"), ("slot_add", "slot_dbl")):
        t2 = ctx.selftest_p28(add, a, b)[0]
        check_xyzz(t2, [T2] * len(A), add)
        for what, o in ((dbl, ctx.selftest_p28(dbl, t2)[0]), (add + " t2 t2", ctx.selftest_p28(add, t2, t2)[0])):
            check_xyzz(o, [None] * len(A), what)
            check_xyzz(ctx.selftest_p28(add, o, c)[0], A, what + " then + P")


@pytest.mark.gpu
def test_xyzz_store_384(ctx):
    """p28_store_384(p28_load(.)): every coordinate times 2^-8 as a canonical residue; the identity as (R, R, 0, 0)."""
    cases = xyzz_single_cases()
    out = unpack(ctx.selftest_p28("store_384", pack([c[0] for c in cases]))[0])
    inv256 = pow(256, -1, P)
    for (raw, pt), got in zip(cases, out):
        assert got == ((R384, R384, 0, 0) if pt is None else tuple(v * inv256 % P for v in raw))


@pytest.mark.gpu
def test_madd28(ctx):
    """One madd28 on an accumulator built as msm_accumulate builds a segment's first entry: ok == false exactly when the second
    point is + or - the first (by its coordinates or through either sign bit), else the sum in point form; the lazy y2 = 4p - y
    at y = 1, y = p - 1 and y = 0."""
    rng = random.Random(2806)
    sub, small = subgroup_points(), small_x_points()
    aff = lambda pt: (pt[0] * R392 % P, pt[1] * R392 % P, 0, 0)
    signed = lambda pt, s: g1_neg(pt) if s else pt
    cases = []
    for i in range(200):
        A, B = rng.sample(sub + small, 2)
        cases.append((A, B, i & 3))
    for i in range(32):
        A = rng.choice(sub + small)
        cases.append((A, A if i & 4 else g1_neg(A), i & 3))        # +- the first point, every pair of sign bits
    for edge in ((0, 1), (0, P - 1), T2):                          # second point with y = 1, p - 1, 0; first point likewise
        assert g1_is_on_curve(edge)
        for fl in range(4):
            for other in (sub[3], small[1]):
                cases.append((other, edge, fl))
                cases.append((edge, other, fl))
    a, b = pack([aff(c[0]) for c in cases]), pack([aff(c[1]) for c in cases])
    flags = np.array([c[2] for c in cases], dtype=np.uint32)
    out, ok, _ = ctx.selftest_p28("madd28", a, b, flags)
    raws = unpack(out)
    n_false = 0
    for i, (A, B, fl) in enumerate(cases):
        same_x = A[0] == B[0]
        assert bool(ok[i]) == (not same_x), (i, fl)
        n_false += same_x
        if not same_x:
            assert legal_xyzz(raws[i]), (i, "form")
            assert decode_xyzz(raws[i]) == g1_add(signed(A, fl & 1), signed(B, fl & 2)), (i, fl)
    assert n_false == 32


@pytest.mark.gpu
def test_te_rows(ctx):
    """msm_te_convert on a count that is no multiple of its chunk, identities inside a chunk: every row (y - x, y + x, 2dxy) 2^392
    canonical with limbs 14, 15 zero, equal to the Python map; the identity row (1, 1, 0); *bad for the order-two point only;
    te28_from_row (one lane and quad, bit for bit) of a device row maps back to the point."""
    sub = subgroup_points()
    pts = list(sub[:37])
    for i in (3, 17, 18, 36):
        pts[i] = None
    mont = pack([(0, 0, 0, 0) if pt is None else (pt[0] * R384 % P, pt[1] * R384 % P, 0, 0) for pt in pts])[:, :12].copy()
    rows, status, _ = ctx.selftest_p28("rows", mont)
    assert status[0] == 0
    assert np.array_equal(rows, pack_rows(pts))
    assert not rows.view(np.uint32).reshape(37, 3, 16)[:, :, 14:].any()
    with_t2 = mont.copy()
    with_t2[20] = pack([((P - 1) * R384 % P, 0, 0, 0)])[0, :12]
    rows2, status2, _ = ctx.selftest_p28("rows", with_t2)
    assert status2[0] != 0
    keep_rows = [i for i in range(37) if i != 20]
    assert np.array_equal(rows2[keep_rows], rows[keep_rows])
    for neg in (0, 1):
        flags = np.full(37, neg, dtype=np.uint32)
        one, _, jac = ctx.selftest_p28("te_from_row", rows, flags=flags, backmap=True)
        check_te(one, jac, [g1_neg(pt) if neg else pt for pt in pts], "te_from_row", x_bound=3)
        assert all(raw[0] > P for raw in unpack(one))
        quad, _, jacq = ctx.selftest_p28("quad_from_row", rows, flags=flags, backmap=True)
        assert np.array_equal(quad, one) and np.array_equal(jacq, jac)


@pytest.mark.gpu
def test_te_additions_one_lane_and_quad(ctx):
    """te28_slot_add (dst apart, dst == pa, pa == pq) and te28_quad_add against the group law through the back-map, on every N
    representative and on the pairs a non-unified law would trip over; the aliased and the quad forms equal te28_slot_add raw slot
    for raw slot; te28_store_384 and te28_quad_store_identity."""
    cases = te_pair_cases()
    a, b, wants = pack([c[0] for c in cases]), pack([c[1] for c in cases]), [c[2] for c in cases]
    ref, _, jac = ctx.selftest_p28("te_slot_add", a, b, backmap=True)
    check_te(ref, jac, wants, "te_slot_add")
    for op in ("te_slot_add_inplace", "quad_add"):
        out, _, j2 = ctx.selftest_p28(op, a, b, backmap=True)
        assert np.array_equal(out, ref) and np.array_equal(j2, jac), op
    dbl, _, jd = ctx.selftest_p28("te_slot_add_self", a, backmap=True)
    check_te(dbl, jd, [g1_add(c[3], c[3]) for c in cases], "te_slot_add a a")
    assert np.array_equal(ctx.selftest_p28("te_slot_add", a, a)[0], dbl)
    assert np.array_equal(ctx.selftest_p28("quad_add_self", a)[0], dbl)
    inv256 = pow(256, -1, P)
    st = unpack(ctx.selftest_p28("te_store_384", ref)[0])
    assert st == [tuple(v * inv256 % P for v in raw) for raw in unpack(ref)]
    ident, _, ji = ctx.selftest_p28("quad_store_identity", None, backmap=True, n=5)
    assert unpack(ident) == [(0, R392, 0, R392)] * 5 and jac_points(ji) == [None] * 5


@pytest.mark.gpu
def test_te_madd_row_one_lane_and_quad(ctx):
    """te28_madd_row and te28_quad_madd_row: acc +- the row's point, the accumulator in every representative te28_from_row and the
    products leave it in, doubling / cancellation / identity rows included; the quad form bit for bit."""
    cases = te_row_cases()
    a, rows = pack([c[0] for c in cases]), pack_rows([c[1] for c in cases])
    flags = np.array([c[2] for c in cases], dtype=np.uint32)
    one, _, jac = ctx.selftest_p28("te_madd_row", a, rows, flags, backmap=True)
    check_te(one, jac, [c[3] for c in cases], "te_madd_row")
    quad = ctx.selftest_p28("quad_madd_row", a, rows, flags)[0]
    assert np.array_equal(quad, one)


@pytest.mark.gpu
def test_te_slot_add_sync_mixed_lanes(ctx):
    """te28_slot_add_sync with the barrier on: in one launch a workgroup with interleaved `act` lanes, one all on, one all off and
    a ragged last one — active lanes equal te28_slot_add slot for slot, the others leave dst untouched."""
    rng = random.Random(2807)
    sub = subgroup_points()
    n = 3 * 256 + 37
    pts = [rng.sample(sub, 2) for _ in range(n)]
    a, b = pack([enc_te(p[0], rng) for p in pts]), pack([enc_te(p[1], rng) for p in pts])
    act = np.array([(i & 1) if i < 256 else (1 if i < 512 else (0 if i < 768 else int(i % 3 == 0))) for i in range(n)], dtype=np.uint32)
    ref = ctx.selftest_p28("te_slot_add", a, b)[0]
    out = ctx.selftest_p28("te_slot_add_sync", a, b, act)[0]
    on = act.astype(bool)
    assert on[:256].sum() == 128 and on[256:512].all() and not on[512:768].any() and 0 < on[768:].sum() < 37
    assert np.array_equal(out[on], ref[on])
    assert (out[~on] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()


@pytest.mark.gpu
def test_chains_of_64_steps(ctx):
    """64 successive p28_add / p28_slot_add and te28_madd_row / te28_quad_madd_row steps, every output fed back in, so that the
    representatives drift as in a segment: the form after every step, the group element against the sum at steps 16, 32, 64."""
    rng = random.Random(2808)
    sub = subgroup_points()
    lanes = 64
    start = [sub[(5 * i) % 48] for i in range(lanes)]
    steps = [[sub[(7 * i + 11 * j) % 48] for i in range(lanes)] for j in range(64)]
    for op in ("add", "slot_add"):
        acc, want = pack([enc_xyzz(pt, rng) for pt in start]), list(start)
        for j, qs in enumerate(steps):
            acc = ctx.selftest_p28(op, acc, pack([enc_xyzz(pt, rng) for pt in qs]))[0]
            want = [g1_add(w, pt) for w, pt in zip(want, qs)]
            if j + 1 in (16, 32, 64):
                check_xyzz(acc, want, "%s chain step %d" % (op, j + 1))
            else:
                assert all(legal_xyzz(raw) for raw in unpack(acc)), (op, j)
    acc, want = pack([enc_te(pt, rng) for pt in start]), list(start)
    accq = acc
    for j, qs in enumerate(steps):
        flags = np.array([(i * (j + 1) >> 1) & 1 for i in range(lanes)], dtype=np.uint32)
        rows = pack_rows(qs)
        acc, _, jac = ctx.selftest_p28("te_madd_row", acc, rows, flags, backmap=True)
        accq = ctx.selftest_p28("quad_madd_row", accq, rows, flags)[0]
        assert np.array_equal(acc, accq), j
        want = [g1_add(w, g1_neg(pt) if fl else pt) for w, pt, fl in zip(want, qs, flags)]
        if j + 1 in (16, 32, 64):
            check_te(acc, jac, want, "te chain step %d" % (j + 1))
        else:
            assert all(v < 2 * P for raw in unpack(acc) for v in raw), j

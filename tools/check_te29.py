#!/usr/bin/env python3
"""Bit-level emulation of the lazy 29-bit twisted Edwards arithmetic of simpleworks_amd/csrc/fq29.cuh (te29_from_row,
te29_madd_row / te29_quad_madd_row through their shared te29_efgh, te29_to_slot): every uint32 limb operation and every 64-bit
column sum — with the `+ 2^29 - 1` of the asm multiplier's carry rule — is checked for wrap-around, and the results are compared
with the group law computed with Python integers on y^2 = x^3 + 1.  worst_case() evaluates the column sums of every product with
each limb at its documented maximum (interval bounds, the real constants).  The sibling of tools/check_te28.py.
`tail`: the same for the general addition the one-lane bucket stage runs (te29_slot_add and its sync / quad forms, te29_store_384):
worst_case_tail() for the nine products and the store's, and bucket stages emulated step by step — running sum, weighted sum,
scan, the shift phase's doublings, fold, tree — on partial sums of every accepted form and on extremal slots.
`header`: writes tail_operands(), the operand maxima of those products, as csrc/te29_bounds_gen.inc, which fq29.cuh evaluates in a
static_assert: one table for the tool and the build.
CPU only; run: python tools/check_te29.py [chains]   |   python tools/check_te29.py tail [chains]   |   python tools/check_te29.py header"""
import os, random, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_te28 as c28
from check_te28 import Q, R, g1_add, g1_mul_fast, g1_neg, inv, te_d, w2te, te2w

NL, BITS, STEPS = 13, 29, 14
M29 = (1 << BITS) - 1
R406 = (1 << (BITS * STEPS)) % Q
LIM = 1 << 64
peak = [0]          # the largest column sum (carry rule included) any emulated product has seen


def limbs(v):
    assert 0 <= v < 1 << (BITS * NL)
    return [(v >> (BITS * i)) & M29 for i in range(NL)]


def val(l):
    return sum(x << (BITS * i) for i, x in enumerate(l))


def spread(kp):
    q = [(kp >> (BITS * i)) & M29 for i in range(NL - 1)] + [kp >> (BITS * (NL - 1))]
    l = [q[0] + (1 << BITS)] + [q[i] + (1 << BITS) - 1 for i in range(1, NL - 1)] + [q[NL - 1] - 1]
    assert val(l) == kp
    return l


P29 = limbs(Q)
assert P29[0] == 1
SPREAD2, SPREAD4 = spread(2 * Q), spread(4 * Q)
ONE, TWO = limbs(R406), limbs(2 * R406 % Q)
INVD = limbs(inv(te_d) * R406 % Q)
TO392 = limbs((1 << 392) % Q)
N_MAX = Q + (Q >> 23)       # what fq29_mul returns stays below this for operands below 8p


def u32(x):
    assert 0 <= x < 1 << 32, "uint32 wrap"
    return x


def columns(a, b):
    """(k, pairs a_i b_(k-i), pairs m_i p_(k-i)) for the 26 columns of fq29_mul"""
    for k in range(NL + STEPS - 1):
        ab = [(i, k - i) for i in range(max(0, k - NL + 1), min(k, NL - 1) + 1)]
        mp = [(i, k - i) for i in range(max(0, k - NL + 1), min(STEPS - 1, k - 1) + 1)]
        yield k, ab, mp


def mul(a, b):
    """fq29_mul / fq29_mul_asm, column by column"""
    assert all(x < 1 << 32 for x in a + b) and val(a) < 8 * Q and val(b) < 8 * Q, "operand outside L"
    m, r, acc = [0] * STEPS, [0] * NL, 0
    for k, ab, mp in columns(a, b):
        acc += sum(a[i] * b[j] for i, j in ab) + sum(m[i] * P29[j] for i, j in mp)
        if k < STEPS:
            t = acc + M29                      # the asm carry rule: one 64-bit add, one bit-select, one shift
            assert t < LIM, "column wrap"
            peak[0] = max(peak[0], t)
            m[k] = (-acc) & M29
            assert (~t) & M29 == m[k] and t >> BITS == (acc + m[k]) >> BITS
            acc = (acc + m[k]) >> BITS
        else:
            assert acc < LIM, "column wrap"
            peak[0] = max(peak[0], acc)
            r[k - STEPS] = acc & M29
            acc >>= BITS
    r[NL - 1] = acc
    assert acc <= M29 and val(r) < N_MAX, "result is not N"
    assert (val(r) * (1 << (BITS * STEPS)) - val(a) * val(b)) % Q == 0
    return r


def column_bound(amax, bmax):
    """largest value any column sum can take (as a fraction of 2^64) when a_i <= amax[i], b_i <= bmax[i], m_i <= 2^29 - 1"""
    carry, worst = 0, 0
    for k, ab, mp in columns(amax, bmax):
        acc = carry + sum(amax[i] * bmax[j] for i, j in ab) + sum(M29 * P29[j] for i, j in mp)
        if k < STEPS:
            acc += M29
        worst = max(worst, acc)
        carry = acc >> BITS
    return worst / LIM


def sub(a, b, sp):
    return [u32(a[i] + sp[i] - b[i]) for i in range(NL)]


def add(a, b):
    return [u32(a[i] + b[i]) for i in range(NL)]


def normalize(a):
    r, c = [0] * NL, 0
    for i in range(NL - 1):
        t = u32(a[i] + c)
        r[i] = t & M29
        c = t >> BITS
    r[NL - 1] = u32(a[NL - 1] + c)
    return r


def row_of(P):  # table row in the 29-bit domain (coordinates x 2^406, canonical)
    x, y = w2te(P)
    return [limbs(v * R406 % Q) for v in ((y - x) % Q, (y + x) % Q, 2 * te_d * x * y % Q)]


def from_row(m2, s2, k2, neg):
    d = [u32(SPREAD2[i] + m2[i] - s2[i]) if neg else u32(SPREAD2[i] + s2[i] - m2[i]) for i in range(NL)]
    ks = [u32(SPREAD2[i] - k2[i]) if neg else k2[i] for i in range(NL)]
    return [normalize(d), normalize(add(s2, m2)), mul(ks, INVD), TWO]


def efgh(A, B, C, Z1, neg, norm="FH"):
    E, h = sub(B, A, SPREAD2), add(A, B)
    D = add(Z1, Z1)
    dm, dp = sub(D, C, SPREAD2), add(D, C)
    F, G, H = (dp, dm, h) if neg else (dm, dp, h)
    E, F, G, H = (normalize(v) if n in norm else v for n, v in zip("EFGH", (E, F, G, H)))
    return E, F, G, H


def madd_row(a, row, neg, norm="FH"):
    x, y, t, z = a
    d = sub(y, x, SPREAD4)
    s = add(y, x)
    A, B, C = mul(d, row[1] if neg else row[0]), mul(s, row[0] if neg else row[1]), mul(t, row[2])
    E, F, G, H = efgh(A, B, C, z, neg, norm)
    return [mul(E, F), mul(G, H), mul(E, H), mul(F, G)]


def pack_words(l):
    assert all(x <= M29 for x in l)
    v = val(l)
    return [(v >> (32 * w)) & 0xffffffff for w in range(12)]


def to_slot(c):
    """te29_to_slot: the 28-bit-domain limbs fq28_unpack reads from the stored words; asserts they are an N value of fq28.cuh"""
    r = mul(c, TO392)
    v = sum(w << (32 * i) for i, w in enumerate(pack_words(r)))
    assert v == val(r) and v < 2 * Q and v >> (28 * 13) < 1 << 15
    return c28.limbs(v)


def to_w(a):  # extended point in the 29-bit domain -> affine on the Weierstrass curve (None = identity)
    X, Y, T, Z = (val(c) * inv(R406) % Q for c in a)
    assert T * Z % Q == X * Y % Q, "T Z != X Y"
    zi = inv(Z)
    return te2w((X * zi % Q, Y * zi % Q))


def worst_case(norm="FH", verbose=False):
    """column bound of every product of te29_from_row / te29_madd_row / te29_to_slot with each limb at its documented maximum"""
    full = [M29] * (NL - 1)
    canon = full + [Q >> (BITS * (NL - 1))]                         # C: the top limb of a value below p
    nmax = full + [N_MAX >> (BITS * (NL - 1))]                      # N
    x1 = full + [3 * Q >> (BITS * (NL - 1))]                        # te29_from_row's X: normalised, below 3p
    y1 = full + [2 * Q >> (BITS * (NL - 1))]                        # Y1 as accepted: normalised, below 2p (te29_from_row's 2y)
    plus = lambda a, b: [x + y for x, y in zip(a, b)]
    nrm = lambda a, top: full + [top >> (BITS * (NL - 1))]          # after fq29_normalize, value below `top`
    out = {}
    out["(Y1-X1+4p) row"] = column_bound(plus(y1, SPREAD4), canon)
    out["(Y1+X1) row"] = column_bound(plus(y1, x1), canon)
    out["T1 row"] = column_bound(nmax, canon)
    out["k2 1/d"] = column_bound(plus([0] * NL, SPREAD2), canon)
    out["coord 2^392"] = column_bound(x1, canon)
    E = plus(nmax, SPREAD2)
    H = plus(nmax, nmax)
    D = plus(nmax, nmax)                                            # 2 Z1, Z1: N (with Z1 up to 2p, F G would reach 1.05 x 2^64)
    dm, dp = plus(D, SPREAD2), plus(D, nmax)
    raw = {"E": E, "H": H}
    top = {"E": 4 * Q, "H": 3 * Q, "F": 5 * Q, "G": 5 * Q}
    for neg in (False, True):
        raw["F"], raw["G"] = (dp, dm) if neg else (dm, dp)
        v = {n: (nrm(raw[n], top[n]) if n in norm else raw[n]) for n in "EFGH"}
        for a, b in ("EF", "GH", "EH", "FG"):
            key = "%s %s%s" % (a, b, " (subtracted)" if neg else "")
            out[key] = column_bound(v[a], v[b])
    if verbose:
        for k, b in out.items():
            print("  %-22s %.3f x 2^64" % (k, b))
    return out


G = (81937999373150964239938255573465948239988671502647976594219695644855304257327692006745978603320413799295628339695,
     241266749859715473739788878240585681733927191168601896383759122102112907357779751001206799952863815012735208165030)
IDENT_ROW = [ONE, ONE, limbs(0)]     # (y - x, y + x, 2 d x y) of (0, 1)


def extremal_rows():
    """rows that are no curve points but the widest limb patterns a sector can hold, and the narrowest"""
    return [[[M29] * NL] * 3, [limbs(Q - 1)] * 3, [limbs(0)] * 3, [limbs(1)] * 3, IDENT_ROW]


def run_chain(pts, signs):
    """a chain on real points, every step compared with the group law; returns the accumulator and the reference"""
    acc = from_row(*row_of(pts[0]), signs[0])
    ref = g1_neg(pts[0]) if signs[0] else pts[0]
    assert to_w(acc) == ref
    for P, sg in zip(pts[1:], signs[1:]):
        acc = madd_row(acc, row_of(P), sg)
        ref = g1_add(ref, g1_neg(P) if sg else P)
        assert to_w(acc) == ref, "madd mismatch"
    return acc, ref


def run_extremal(steps=6):
    """chains on the extremal rows: no group law to compare with (mul checks every product's congruence), only wrap-around"""
    rows = extremal_rows()
    n = 0
    for first in rows:
        for neg0 in (False, True):
            for row in rows:
                for neg in (False, True):
                    acc = from_row(*first, neg0)
                    for _ in range(steps):
                        acc = madd_row(acc, row, neg)
                        n += 1
                    for c in acc:
                        to_slot(c)
    return n


# ------------------------------------------------------------------------------------------------ the general addition (bucket stage)
# te29_slot_add / te29_slot_add_sync / te29_quad_add and te29_store_384 of fq29.cuh: points at rest in memory, four coordinates of
# thirteen limbs.  Accepted operand forms: all four N (what an addition leaves); te29_from_row's (X normalised in (p, 3p), Y
# normalised below 2p, T: N, Z: the constant); the identity (0 : 1 : 0 : 1).
K2D = limbs(2 * te_d * R406 % Q)
TO384 = limbs((1 << 384) % Q)
IDENT = [limbs(0), ONE, limbs(0), ONE]
TOP = BITS * (NL - 1)


def at_rest(p):
    """asserts p is a point a slot may hold: limbs below the top one under 2^29, X < 3p, Y < 2p, T and Z: N"""
    for c, bound in zip(p, (3 * Q, 2 * Q, N_MAX, N_MAX)):
        assert all(x <= M29 for x in c[:NL - 1]) and val(c) < bound, "operand form"
    return p


def slot_add(a, q):
    """te29_slot_add: nine products, (Y1 - X1 + 4p) and (Y1 + X1) of the FIRST operand carry-normalised, the second operand's raw"""
    (ax, ay, at, az), (qx, qy, qt, qz) = at_rest(a), at_rest(q)
    A = mul(normalize(sub(ay, ax, SPREAD4)), sub(qy, qx, SPREAD4))
    B = mul(normalize(add(ay, ax)), add(qy, qx))
    C = mul(mul(at, qt), K2D)
    ZZ = mul(az, qz)
    E, F, G, H = efgh(A, B, C, ZZ, False)
    return at_rest([mul(E, F), mul(G, H), mul(E, H), mul(F, G)])


def store_384(p):
    """te29_store_384: canonical coordinates in radix 2^384"""
    out = []
    for c in at_rest(p):
        r = val(mul(c, TO384))
        r -= Q if r >= Q else 0
        assert 0 <= r < Q and r == val(c) * inv(R406) * (1 << 384) % Q
        out.append(r)
    return out


def tail_operands(norm_first=True):
    """(a_max, b_max) of each of the nine products of te29_slot_add and of te29_store_384's: every limb at the maximum of the widest
    accepted operand form (which covers doubling and the identity: they are operands of those forms)"""
    full = [M29] * (NL - 1)
    canon = full + [Q >> TOP]
    nmax = full + [N_MAX >> TOP]
    x1 = full + [3 * Q >> TOP]
    y1 = full + [2 * Q >> TOP]
    plus = lambda a, b: [x + y for x, y in zip(a, b)]
    nrm = lambda top: full + [top >> TOP]
    d_raw, s_raw = plus(y1, SPREAD4), plus(y1, x1)          # Y - X + 4p (X down to 0), Y + X
    # second round (te29_efgh, a point that is added): A, B, C: N and D = 2 Z1 Z2 with Z1 Z2: N
    D = plus(nmax, nmax)
    E, H, F, G = plus(nmax, SPREAD2), nrm(3 * Q), nrm(5 * Q), plus(D, nmax)
    return {"A (Y1-X1+4p)(Y2-X2+4p)": (nrm(6 * Q) if norm_first else d_raw, d_raw),
            "B (Y1+X1)(Y2+X2)": (nrm(5 * Q) if norm_first else s_raw, s_raw),
            "T1 T2": (nmax, nmax), "(T1 T2) 2d": (nmax, canon), "Z1 Z2": (nmax, nmax),
            "E F": (E, F), "G H": (G, H), "E H": (E, H), "F G": (F, G), "coord 2^384": (x1, canon)}


def worst_case_tail(verbose=False, norm_first=True):
    """column bound of each product of tail_operands()"""
    out = {k: column_bound(a, b) for k, (a, b) in tail_operands(norm_first).items()}
    second = worst_case("FH")                                # the mixed addition's second round has the same operands
    assert all(out[k] == second[k] for k in ("E F", "G H", "E H", "F G"))
    if verbose:
        for k, b in out.items():
            print("  %-24s %.3f x 2^64" % (k, b))
    return out


def bounds_header():
    """csrc/te29_bounds_gen.inc: tail_operands() as the table fq29.cuh evaluates at build time (te29_slot_add_bounds_ok)"""
    rows = ["// generated by tools/check_te29.py (python tools/check_te29.py header): operand maxima of the nine products of te29_slot_add and of",
            "// te29_store_384's, {name, a_max[13], b_max[13]} — tools/check_te29.py tail_operands(); tests/test_te29_tail_bounds.py holds",
            "// this file to the tool.", "#define SWM_TE29_TAIL_BOUNDS \\"]
    items = list(tail_operands().items())
    for n, (k, (a, b)) in enumerate(items):
        arr = lambda l: "{" + ", ".join("0x%08xu" % x for x in l) + "}"
        rows.append('    {"%s", %s, \\' % (k, arr(a)))
        rows.append("     %s}%s" % (arr(b), ", \\" if n + 1 < len(items) else ""))
    return "\n".join(rows) + "\n"


def nl(v):
    """limbs of a value that may exceed 2^377: the top limb takes what is left (a normalised coordinate)"""
    return [(v >> (BITS * i)) & M29 for i in range(NL - 1)] + [v >> TOP]


def extremal_points():
    """slots that are no curve points: every coordinate at the edge of its accepted form, in value and in limb pattern"""
    def edge(bound):
        top = (bound - 1) >> TOP
        return [nl(bound - 1), [M29] * (NL - 1) + [top - 1], [M29] * (NL - 1) + [0], nl(0), nl(1)]
    xs, ys, ns = edge(3 * Q), edge(2 * Q), edge(N_MAX)
    return [[xs[i], ys[i], ns[i], ns[i]] for i in range(5)] + [[xs[0], ys[4], ns[1], ns[3]], [xs[3], ys[0], ns[0], ns[1]], IDENT]


def bucket_stage(parts, lanes, log_m, wref):
    """The micro-operations of msm_bucket_reduce on 2^log_m buckets per lane: running sum, weighted sum, suffix scan, the shift
    phase's doublings, the fold and the tree — all by slot_add.  parts[b]: the partial sums of bucket b (slots); wref[b]: the
    bucket's sum on the Weierstrass curve, or None when the points are extremal slots (then only wrap-around is checked).
    Returns (A, R) of the workgroup and the number of additions."""
    m, n = 1 << log_m, 0
    run, acc = [IDENT] * lanes, [IDENT] * lanes
    ref_run, ref_acc = [None] * lanes, [None] * lanes
    check = wref is not None
    for t in range(lanes):
        for b in range((t + 1) * m - 1, t * m - 1, -1):
            for p in parts[b]:
                run[t] = slot_add(run[t], p)
                n += 1
            acc[t] = slot_add(acc[t], run[t])
            n += 1
            if check:
                ref_run[t] = g1_add(ref_run[t], wref[b])
                ref_acc[t] = g1_add(ref_acc[t], ref_run[t])
                assert to_w(run[t]) == ref_run[t] and to_w(acc[t]) == ref_acc[t], "walk mismatch"
    d = 1
    while d < lanes:                                         # inclusive suffix scan (Hillis-Steele)
        nxt, nref = list(run), list(ref_run)
        for t in range(lanes - d):
            nxt[t] = slot_add(run[t], run[t + d])
            nref[t] = g1_add(ref_run[t], ref_run[t + d]) if check else None
            n += 1
        run, ref_run = nxt, nref
        d <<= 1
    r_blk, ref_r = run[0], ref_run[0]
    sh = run[1:] + [IDENT]
    ref_sh = ref_run[1:] + [None]
    for _ in range(log_m):                                   # the shift phase: doublings, pa == pq
        sh = [slot_add(p, p) for p in sh]
        ref_sh = [g1_add(p, p) for p in ref_sh] if check else ref_sh
        n += lanes
    acc = [slot_add(a, s) for a, s in zip(acc, sh)]          # fold
    ref_acc = [g1_add(a, s) for a, s in zip(ref_acc, ref_sh)] if check else ref_acc
    n += lanes
    d = lanes // 2
    while d:                                                 # tree
        for t in range(d):
            acc[t] = slot_add(acc[t], acc[t + d])
            ref_acc[t] = g1_add(ref_acc[t], ref_acc[t + d]) if check else None
            n += 1
        d >>= 1
    if check:
        assert to_w(r_blk) == ref_r and to_w(acc[0]) == ref_acc[0], "stage mismatch"
        # the workgroup's results as the weighted sum of its buckets
        want_a = want_r = None
        for b in range(lanes * m):
            want_r = g1_add(want_r, wref[b])
            want_a = g1_add(want_a, g1_mul_fast(wref[b], b + 1) if wref[b] is not None else None)
        assert ref_r == want_r and ref_acc[0] == want_a
    for p in (r_blk, acc[0]):
        store_384(p)
    return acc[0], r_blk, n


def run_tail(chains=3):
    """bucket stages on real points — partial sums of every accepted form: one-entry segments (te29_from_row), longer ones (after
    te29_madd_row), empty ones (the identity), a bucket that cancels, a bucket whose two partial sums are equal — and on extremal
    slots; plus every pair of extremal slots through one addition, either way round and doubled.  Returns the additions emulated."""
    n = 0
    for c in range(chains):
        lanes, log_m = 4, 1
        parts, wref = [], []
        for b in range(lanes << log_m):
            kind = (b + c) % 5
            segs, ref = [], None
            for s in range((0, 2, 1, 1, 1)[kind]):              # kind 0: an empty bucket, the identity
                pts = [g1_mul_fast(G, random.randrange(1, R)) for _ in range(1 if kind == 2 else 3)]
                signs = [random.random() < 0.5 for _ in pts]
                a, r = run_chain(pts, signs)
                segs.append(a)
                ref = g1_add(ref, r)
            if kind == 3:                                    # the same partial sum twice: the unified law doubles
                segs.append(segs[0])
                ref = g1_add(ref, ref)
            if kind == 4:                                    # P + (-P): the bucket's running sum returns to where it was
                P = g1_mul_fast(G, random.randrange(1, R))
                segs += [from_row(*row_of(P), False), from_row(*row_of(P), True)]
            if not segs:
                segs = [IDENT]
            parts.append(segs)
            wref.append(ref)
        n += bucket_stage(parts, lanes, log_m, wref)[2]
    ext = extremal_points()
    for a in ext:
        for q in ext:
            r = slot_add(a, q)
            r = slot_add(r, r)
            slot_add(q, r)
            n += 3
    n += bucket_stage([[ext[b % len(ext)], ext[(3 * b + 1) % len(ext)]] for b in range(8)], 4, 1, None)[2]
    return n


def tail_main(chains=3, verbose=True):
    """the general addition: emulated chains and worst-case columns; returns (worst column as a fraction of 2^64, additions)"""
    random.seed(2929)
    peak[0] = 0
    n = run_tail(chains)
    wc = worst_case_tail(verbose)
    worst = max(wc.values())
    if verbose:
        print("te29 general addition OK: %d additions on points and extremal slots; no uint32 / uint64 wrap; peak column %.3f x 2^64"
              % (n, peak[0] / LIM))
        print("worst column of the nine products and of te29_store_384: %.3f x 2^64 (limit %.9f)" % (worst, (LIM - (1 << BITS)) / LIM))
        raw = worst_case_tail(False, norm_first=False)
        print("  with neither first-round operand normalised: A %.3f, B %.3f x 2^64  -> overflow"
              % (raw["A (Y1-X1+4p)(Y2-X2+4p)"], raw["B (Y1+X1)(Y2+X2)"]))
    assert worst * LIM < LIM - (1 << BITS) and peak[0] < LIM - (1 << BITS)
    return worst, n


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "header":
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "simpleworks_amd", "csrc", "te29_bounds_gen.inc")
        with open(path, "w") as f:
            f.write(bounds_header())
        print("wrote", os.path.normpath(path))
        return
    if len(sys.argv) > 1 and sys.argv[1] == "tail":
        tail_main(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
        return
    chains = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    random.seed(29)
    n_add = 0
    for c in range(chains):
        pts = [g1_mul_fast(G, random.randrange(1, R)) for _ in range(8)]
        if c == 1:
            pts[3] = pts[2]            # doubling inside a chain
        if c == 2:
            pts[1] = g1_neg(pts[0])    # cancellation: the running sum passes through the identity
        if c == 3:
            pts[4] = None              # the identity row
        signs = [random.random() < 0.5 for _ in pts]
        acc, ref = run_chain(pts, signs)
        n_add += len(pts) - 1
        # the epilogue's slot is the 28-bit-domain point check_te28 knows
        assert c28.to_w([to_slot(v) for v in acc]) == ref
    n_ext = run_extremal()
    print("te29 emulation OK: %d mixed additions on points, %d on extremal rows; no uint32 / uint64 wrap; peak column %.3f x 2^64"
          % (n_add, n_ext, peak[0] / LIM))
    print("worst-case column bounds, F and H normalised:")
    wc = worst_case("FH", True)
    assert max(wc.values()) < 1.0
    for alt in ("", "F", "H", "EG"):
        w = worst_case(alt)
        print("  normalised {%s}: max %.3f x 2^64%s" % (alt, max(w.values()), "" if max(w.values()) < 1 else "  -> overflows"))


if __name__ == "__main__":
    main()

"""GPU parity tests (-m gpu) of the K4 polynomial drivers (csrc/devops.cuh) and of the arithmetic under the transform
(csrc/fr29.cuh, csrc/frinv.cuh), called through the self-test entry points of the C ABI (include/swmarlin.h:
swm_selftest_fr29, swm_selftest_poly, swm_selftest_sample_fr).  Every expectation comes from Python integers or from the C
oracle, at the shapes and operands where lazy reduction, carries and tiling go wrong: values at the stated bounds, lengths
at tile and block edges, single nonzero coefficients at the boundaries, draws across ChaCha blocks and across the host ring
of a caller-owned generator."""
import random

import numpy as np
import pytest

from oracle_lib import Oracle, R, expected_bytes, golden, h2i, ints_to_limbs, limbs_to_ints, p64

pytestmark = pytest.mark.gpu

M29 = (1 << 29) - 1
RM = (1 << 256) % R          # Montgomery factor of the memory format
INV261 = pow(1 << 261, -1, R)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def ctx():
    import simpleworks_amd as swm
    c = swm.Context(0)
    yield c
    c.close()


def mont(vals):
    """standard integers -> n x 4 memory-format limbs"""
    return ints_to_limbs([v % R * RM % R for v in vals], 4)


def unmont(arr):
    inv = pow(RM, -1, R)
    return [v * inv % R for v in limbs_to_ints(np.asarray(arr).reshape(-1, 4))]


def raw_ints(arr):
    return limbs_to_ints(np.asarray(arr).reshape(-1, 4))


def mont1(v):
    return mont([v])[0]


# ------------------------------------------------------------------------------------------------ 29-bit limbs
def l9(v):
    """normalised limbs of v (limbs 0..7 < 2^29, limb 8 takes the rest)"""
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def v9(limbs):
    return sum(int(x) << (29 * i) for i, x in enumerate(limbs))


def arr9(rows):
    return np.array(rows, dtype=np.uint64).astype(np.uint32).reshape(-1, 9)


def words9(v):
    """an 8-word (memory format) operand in limbs 0..7 of a 9-limb row"""
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0]


def lazy_spread(k, borrows):
    """limbs of k r with `borrows` x 2^29 moved into every limb below the top one (the spreads ntt.hip passes to fr29_sub)"""
    sp = l9(k * R)
    sp[0] += borrows << 29
    for i in range(1, 8):
        sp[i] += (borrows << 29) - borrows
    sp[8] -= borrows
    assert v9(sp) == k * R
    return sp


def ntt_spreads():
    """every spread lazy_plan (ntt.hip) builds: r2 / s1 = 2 B r with one borrow, s2 = 4 B r with two, s4 = 4 r with one"""
    out = {(4, 1)}
    for b in (1, 2, 4, 8, 16, 32, 64):
        out |= {(2 * b, 1), (4 * b, 2)}
    return sorted(out)


def _mul_pairs():
    """(a, b) limb lists inside fr29_mul's contract: a lazy with limbs < 3 * 2^30, b normalised, a b < 2^261 r"""
    rnd = random.Random(29)
    bound = R << 261
    edge = [0, 1, 2, R - 1, R, R + 1, 2 * R - 1, 2 * R, 3 * R, 4 * R - 1, (1 << 253) - 1, (1 << 256) - 1]
    bs = [l9(v) for v in edge] + [[M29] * 9]                                  # normalised b: all limbs 2^29 - 1 included
    bs += [l9(rnd.randrange(4 * R)) for _ in range(40)]
    As = [l9(v) for v in edge] + [[M29] * 9]
    As += [[x + y for x, y in zip(l9(u), l9(w))] for u in (2 * R - 1, R - 1, 0) for w in (2 * R - 1, 1 << 252)]  # lazy sums
    As += [[x + y for x, y in zip(l9(rnd.randrange(2 * R)), l9(rnd.randrange(2 * R)))] for _ in range(40)]
    As += [[2 * M29] * 8 + [l9(2 * R - 1)[8] * 2]]                                # the largest sum of two values below 2r
    # differences a - b + k r of fr29_sub at every spread of the transform: a a lazy sum of two values < B r, b likewise
    for k, borrows in ntt_spreads():
        sp = lazy_spread(k, borrows)
        for _ in range(3):
            hi = max(1, k // (2 * borrows)) * R
            a = [x + y for x, y in zip(l9(rnd.randrange(hi)), l9(rnd.randrange(hi)))] if borrows == 2 else l9(rnd.randrange(hi))
            b = [x + y for x, y in zip(l9(rnd.randrange(hi)), l9(rnd.randrange(hi)))] if borrows == 2 else l9(rnd.randrange(hi))
            As.append([x + s - y for x, s, y in zip(a, sp, b)])
        As.append([M29 * borrows + s for s in sp[:8]] + [sp[8]])   # a at its limb maximum, b = 0
    top = 3 * (1 << 30) - 1
    As += [[top] * 9, [top] * 8 + [0], [top] * 8 + [1 << 20], [(1 << 32) - 1] * 9, [(1 << 32) - 1] * 8 + [0]]
    As += [[rnd.randrange(top + 1) for _ in range(9)] for _ in range(20)]
    pairs = []
    for a in As:
        va = v9(a)
        small = max(a) < 3 << 30
        for b in bs:
            if va * v9(b) < bound and small:
                pairs.append((a, b))
        if va:
            # just under the product bound: the largest normalised b (all limbs full or not), and one 2^64 below it
            vb = (bound - 1) // va
            for cand in (vb, vb - (1 << 64), min(vb, (1 << 249) - 1)):
                if 0 <= cand < 1 << 261 and small:
                    pairs.append((a, l9(cand)))
        if max(a) >= 3 << 30:  # limbs up to 2^32 - 1: only against a single-limb b (the column sums stay below 2^64)
            for b in (0, 1, M29):
                pairs.append((a, l9(b)))
    pairs += [(l9(rnd.randrange(2 * R)), l9(rnd.randrange(2 * R))) for _ in range(3000)]
    return pairs


def test_fr29_mul_at_its_bounds(ctx):
    """fr29_mul_fenced (asm) and fr29_mul (C): a b 2^-261 mod r, normalised, < 2r, and the two equal limb for limb, for a
    lazy (limbs < 3 * 2^30), b normalised and a b < 2^261 r: edge values, lazy sums, the differences the transform forms,
    limbs at the top of the lazy range and pairs just under the product bound."""
    pairs = _mul_pairs()
    A = arr9([p[0] for p in pairs])
    B = arr9([p[1] for p in pairs])
    asm = ctx.selftest_fr29("mul", A, B)
    cf = ctx.selftest_fr29("mul_c", A, B)
    assert np.array_equal(asm, cf), "asm multiplier differs from fr29_mul"
    for (a, b), o in zip(pairs, asm):
        vo = v9(o)
        assert all(int(x) <= M29 for x in o[:8]), (a, b)
        assert vo < 2 * R, (a, b)
        assert vo % R == v9(a) * v9(b) * INV261 % R, (a, b)


def test_fr29_sub_at_the_transform_spreads(ctx):
    """fr29_sub(a, b, spread) = a + spread - b limb by limb, with the spreads of the transform and operands at their top"""
    rnd = random.Random(30)
    for k, borrows in ntt_spreads():
        sp = lazy_spread(k, borrows)
        hi = max(1, k // (2 * borrows)) * R
        A, B = [], []
        for _ in range(64):
            A.append(l9(rnd.randrange(hi)))
            b = l9(rnd.randrange(hi))
            if borrows == 2:
                b = [x + y for x, y in zip(b, l9(rnd.randrange(hi)))]
            B.append(b)
        A.append([0] * 9)
        B.append([M29 * borrows] * 8 + [sp[8]])  # the largest subtrahend the spread covers limb by limb
        out = ctx.selftest_fr29("sub", arr9(A), arr9(B), np.array(sp, dtype=np.uint32))
        for a, b, o in zip(A, B, out):
            assert [int(x) for x in o] == [x + s - y for x, s, y in zip(a, sp, b)], (k, borrows)
            assert v9(o) == v9(a) - v9(b) + k * R


def test_fr29_reductions_and_packing(ctx):
    """normalize, cond_sub by 2r and by r, canonical (below_2r true / false), unpack and pack at r - 1, r, 2r - 1, 2r, 4r - 1"""
    rnd = random.Random(31)
    vals = [0, 1, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 3 * R, 4 * R - 1] + [rnd.randrange(4 * R) for _ in range(200)]
    A = arr9([l9(v) for v in vals])
    for op, k in (("cond_sub_2r", 2 * R), ("cond_sub_r", R)):
        out = ctx.selftest_fr29(op, A)
        assert [v9(o) for o in out] == [v - k if v >= k else v for v in vals], op
        assert all(int(x) <= M29 for o in out for x in o[:8])
    below2 = [v for v in vals if v < 2 * R]
    out = ctx.selftest_fr29("canonical_below_2r", arr9([l9(v) for v in below2]))
    assert [v9(o) for o in out] == [v % R for v in below2]
    out = ctx.selftest_fr29("canonical", A)
    assert [v9(o) for o in out] == [v % R for v in vals]
    # normalize: lazy limbs up to 2^32 - 8 (a carry out of a limb is at most 7; the top limb keeps what is left)
    top = (1 << 32) - 8
    lazy = [l9(v) for v in vals] + [[top] * 8 + [1 << 24], [(1 << 30) - 1] * 9, [top, 0] * 4 + [0], [0, top] * 4 + [top]]
    lazy += [[rnd.randrange(top + 1) for _ in range(8)] + [rnd.randrange(1 << 26)] for _ in range(50)]
    out = ctx.selftest_fr29("normalize", arr9(lazy))
    for a, o in zip(lazy, out):
        assert all(int(x) <= M29 for x in o[:8]) and v9(o) == v9(a)
    # unpack / pack of 8-word values
    words = vals + [(1 << 256) - 1, 1 << 255, (1 << 232) - 1, 1 << 232]
    words = [w for w in words if w < 1 << 256]
    out = ctx.selftest_fr29("unpack", arr9([words9(w) for w in words]))
    assert [[int(x) for x in o] for o in out] == [l9(w) for w in words]
    out = ctx.selftest_fr29("pack", arr9([l9(w) for w in words]))
    assert [[int(x) for x in o] for o in out] == [words9(w) for w in words]


# ------------------------------------------------------------------------------------------------ single-element inversion
def _inverse_edges():
    """raw memory-format words where the binary GCD's 64-bit approximations are weakest, plus long runs of trailing zeros"""
    rnd = random.Random(32)
    v = [1, 2, 3, R - 1, R - 2, (R + 1) // 2, (R - 1) // 2, (R + 3) // 2, 1 << 252, (1 << 252) - 1, (1 << 31) - 1, 1 << 31,
         (1 << 64) + 1, 1 << 32, 1 << 33, 1 << 63, 1 << 64, (1 << 31) * 3, (1 << 95) + (1 << 40)]
    v += [R - (1 << k) for k in range(0, 252, 7)] + [R - (1 << k) - 1 for k in (1, 31, 32, 63, 64)]
    v += [(R >> 1) + d for d in range(-3, 4)] + [(R >> 1) + (1 << k) for k in (31, 32, 64, 128)]
    v += [1 << k for k in range(0, 253, 5)]
    v += [(rnd.randrange(1, R >> 40) << 40) for _ in range(20)]
    v += [rnd.randrange(1, R) for _ in range(300)]
    return sorted({x for x in v if 0 < x < R})


def test_device_single_inversion_and_exact_fallback(ctx):
    """fr_inv_single (binary GCD on approximations) and fr_inv_single_exact (the fallback loop, run directly) on the device,
    against pow(a, -1, r) on the memory form: out = (a 2^-256)^-1 2^256."""
    W = _inverse_edges()
    A = arr9([words9(w) for w in W])
    want = [pow(w, -1, R) * RM * RM % R for w in W]
    for op in ("inv", "inv_exact"):
        out = ctx.selftest_fr29(op, A)
        got = [sum(int(o[i]) << (32 * i) for i in range(8)) for o in out]
        assert got == want, op


@pytest.mark.parametrize("n,group", [(37 * 1024 + 3, 1024), ((1 << 18) + 4096 * 3 + 17, 4096)])
def test_batch_inverse_one_element_per_workgroup(ctx, n, group):
    """batch_inverse_fr with a single nonzero element per workgroup (the rest zeros): the workgroup's one inversion runs on
    exactly that element, set to the edge values above, at both chunk sizes (n <= 2^18: 1024 per workgroup, else 4096)."""
    W = _inverse_edges()
    x = np.zeros((n, 4), dtype=np.uint64)
    pos, vals = [], []
    for g in range((n + group - 1) // group):
        p = min(n - 1, g * group + (g * 37) % group)
        pos.append(p)
        vals.append(W[g % len(W)])
    x[pos] = ints_to_limbs(vals, 4)
    out = ctx.batch_inverse_fr(x)
    got = raw_ints(out[pos])
    assert got == [pow(w, -1, R) * RM * RM % R for w in vals]
    mask = np.ones(n, dtype=bool)
    mask[pos] = False
    assert not out[mask].any(), "zeros must stay zero"


# ------------------------------------------------------------------------------------------------ suffix recurrence
def _rec_python(a, m, z):
    out = list(a)
    for k in range(len(out) - m - 1, -1, -1):
        out[k] = (out[k] + z * out[k + m]) % R
    return out


def _rec_check(orc, a_m, out_m, m, z):
    """out[k] = a[k] + z out[k + m] for k < n - m and out[k] = a[k] above: determines the result (memory form, oracle)"""
    n = a_m.shape[0]
    assert out_m.shape == a_m.shape
    if n <= m:
        assert np.array_equal(out_m, a_m)
        return
    assert np.array_equal(out_m[n - m:], a_m[n - m:])
    k = n - m
    zr = np.ascontiguousarray(np.broadcast_to(mont1(z), (k, 4)))
    prod = np.empty((k, 4), dtype=np.uint64)
    orc.lib.oracle_fr_mul(p64(zr), p64(np.ascontiguousarray(out_m[m:])), p64(prod), k)
    exp = np.empty_like(prod)
    orc.lib.oracle_fr_add(p64(np.ascontiguousarray(a_m[:k])), p64(prod), p64(exp), k)
    bad = np.nonzero((exp != out_m[:k]).any(axis=1))[0]
    assert bad.size == 0, "first mismatch at %d of %d (m = %d)" % (int(bad[0]), n, m)


def _data(orc, kind, n, seed):
    from pyref.prng import fr_array
    if kind == "random":
        return np.ascontiguousarray(orc.fr_to_mont(fr_array(n, seed))) if n else np.zeros((0, 4), np.uint64)
    if kind == "r-1":
        return np.ascontiguousarray(np.broadcast_to(mont1(R - 1), (n, 4)))
    return np.zeros((n, 4), dtype=np.uint64)


Z_SET = [0, 1, 2, R - 1, 0x0B5A2D3C4E5F60718293A4B5C6D7E8F90112233445566778899AABBCCDDEEFF1]
M1_LENGTHS = [0, 1, 2, 15, 16, 17, 255, 256, 257, 8191, 8192, 8193, 2048 * 5 - 1, 2048 * 5 + 1, 2048 * 64 - 1,
              2048 * 64 + 1, (1 << 20) + 3]
STRIDES = [2, 3, 7, 37, 1023, 4096]


def _rec_cases():
    cases = [(1, n) for n in M1_LENGTHS]
    for m in STRIDES:
        cases += [(m, n) for n in (m - 1, m, m + 1, 16 * m, 16 * m + 1, 256 * m + 5)]
    return cases


@pytest.mark.parametrize("m,n", _rec_cases())
def test_suffix_recurrence_shapes(ctx, orc, m, n):
    """division by X^m - z on every path (rec_serial; rec_local / rec_fix with the heads' recursion; the tiled lazy-limb
    passes for m = 1, n >= 8192) at the block and tile edges, z in {0, 1, 2, r - 1, random}, random / all r - 1 / zero data;
    Python integers up to 20 000 elements, the oracle's relation beyond"""
    for i, z in enumerate(Z_SET):
        kinds = ["random"] + (["r-1"] if i in (1, 3) else []) + (["zero"] if i == 4 else [])
        for kind in kinds:
            a = _data(orc, kind, n, 700 + i)
            out = ctx.selftest_suffix_recurrence(a, m, mont1(z))
            _rec_check(orc, a, out, m, z)
            if n <= 20000 and kind == "random":
                assert unmont(out) == _rec_python(unmont(a), m, z), (m, n, z)


def _edge_positions(n, m):
    ps = set()
    if m == 1:
        for b in (1, 2, 3, n // 2048, n // 2048 - 1):
            ps |= {2048 * b - 1, 2048 * b, 2048 * b + 1, 8 * b - 1, 8 * b, 256 * b}
    for b in (1, 2, n // (16 * m), n // (16 * m) - 1):
        ps |= {16 * m * b - 1, 16 * m * b, 16 * m * b + 1}
    ps |= {0, n - 1, n - m, n - m - 1}
    return sorted(p for p in ps if 0 <= p < n)


@pytest.mark.parametrize("m,n", [(1, 8192), (1, 2048 * 7 + 1), (1, (1 << 18) + 5), (3, 16 * 3 * 19 + 2), (37, 256 * 37 + 5),
                                 (1023, 16 * 1023 * 3 + 1)])
def test_suffix_recurrence_single_nonzero_at_edges(ctx, m, n):
    """one nonzero coefficient c at a tile / block edge: out[k] = c z^((p - k) / m) for k = p mod m, k <= p, else zero"""
    z = Z_SET[4]
    c = 0xDEADBEEF
    for p in _edge_positions(n, m):
        a = np.zeros((n, 4), dtype=np.uint64)
        a[p] = mont1(c)
        out = ctx.selftest_suffix_recurrence(a, m, mont1(z))
        nz = np.nonzero(out.any(axis=1))[0]
        want_idx = np.arange(p % m, p + 1, m)
        assert np.array_equal(nz, want_idx), (m, n, p)
        # values: c z^j at index p - j m, checked at the ends and at a spread of points
        js = sorted(j for j in {0, 1, 2, len(want_idx) - 1, len(want_idx) // 2, len(want_idx) // 3} if j < len(want_idx))
        got = unmont(out[[p - j * m for j in js]])
        assert got == [c * pow(z, j, R) % R for j in js], (m, n, p)


def test_suffix_recurrence_tiles_recurse_into_the_tiled_path(ctx, orc):
    """n = 2^24 + 1: 8193 tiles, so the tiles' totals run through the tiled path again; the whole result is checked
    against the relation with the oracle's multiplication and addition"""
    from pyref.prng import fr_array
    n = (1 << 24) + 1
    a = orc.fr_to_mont(fr_array(n, 741))
    z = Z_SET[4]
    out = ctx.selftest_suffix_recurrence(a, 1, mont1(z))
    _rec_check(orc, a, out, 1, z)


# ------------------------------------------------------------------------------------------------ div_linear
@pytest.mark.parametrize("n", [0, 1, 2, 17, 257, 8191, 8192, 8193, 2048 * 9 + 1])
def test_div_linear(ctx, n):
    """p = q (X - z) + p(z) in Python integers"""
    from pyref.prng import fr_array
    p = Oracle().fr_to_mont(fr_array(n, 800 + n)) if n else np.zeros((0, 4), np.uint64)
    P = unmont(p)
    for z in Z_SET:
        out = ctx.selftest_div_linear(p, mont1(z))
        w = unmont(out)
        if n == 0:
            continue
        val, q = w[0], w[1:]
        # q (X - z) + val, coefficient by coefficient (this fixes q and val)
        recon = [(val - z * q[0]) % R if q else val] + [((q[i - 1] if i - 1 < len(q) else 0) - z * (q[i] if i < len(q) else 0)) % R
                                                         for i in range(1, n)]
        assert recon == P, (n, z)


# ------------------------------------------------------------------------------------------------ Horner
def _horner(c, x):
    acc = 0
    for v in reversed(c):
        acc = (acc * x + v) % R
    return acc


W4096 = pow(22, (R - 1) // 4096, R)   # a primitive 4096-th root of unity (22 generates Fr^*): every higher-level point is 1
X_SET = [0, 1, R - 1, Z_SET[4], W4096]


def test_root_of_unity_is_primitive():
    assert pow(W4096, 4096, R) == 1 and pow(W4096, 2048, R) != 1


@pytest.mark.parametrize("n", [0, 1, 255, 256, 4095, 4096, 4097, 3 * 4096 + 5])
def test_poly_eval_dense(ctx, n):
    from pyref.prng import fr_array
    p = Oracle().fr_to_mont(fr_array(n, 900 + n)) if n else np.zeros((0, 4), np.uint64)
    P = unmont(p)
    for x in X_SET:
        assert unmont(ctx.selftest_poly_eval(p, mont1(x)))[0] == _horner(P, x), (n, x)


@pytest.mark.parametrize("n", [4096 * 4096, 4096 * 4096 + 1])
def test_poly_eval_two_and_three_levels(ctx, n):
    """sparse coefficients at the level boundaries of a 2-level (4096^2) and a 3-level (4096^2 + 1) evaluation"""
    rnd = random.Random(n)
    idx = sorted({0, 1, 255, 256, 4095, 4096, 4097, 4096 * 17 - 1, 4096 * 4095, n - 4097, n - 4096, n - 2, n - 1})
    coef = [rnd.randrange(R) for _ in idx]
    p = np.zeros((n, 4), dtype=np.uint64)
    p[idx] = mont(coef)
    for x in X_SET:
        want = sum(c * pow(x, i, R) for c, i in zip(coef, idx)) % R
        assert unmont(ctx.selftest_poly_eval(p, mont1(x)))[0] == want, (n, x)


@pytest.mark.parametrize("count", [1, 32, 33, 70])
def test_poly_eval_many_matches_poly_eval(ctx, count):
    """batches of 1, 32, 33 and 70 pieces of one buffer, mixed lengths (0, one tile, several tiles, more than one level of
    several tiles each): equal to poly_eval bit for bit and to Python"""
    from pyref.prng import fr_array
    rnd = random.Random(count)
    lens = [3 * 4096 + 7, 0, 1, 4096, 4097, 9000, 255, 2 * 4096][:count] + [rnd.choice([0, 5, 4096, 4097, 12289, 20000, 300])
                                                                              for _ in range(max(0, count - 8))]
    offs, o = [], 0
    for ln in lens:
        offs.append(o)
        o += ln + rnd.randrange(3)
    buf = Oracle().fr_to_mont(fr_array(max(o, 1), 950 + count))
    pieces = list(zip(offs, lens))
    B = unmont(buf)
    for x in (Z_SET[4], W4096, R - 1):
        got = ctx.selftest_poly_eval_many(buf, pieces, mont1(x))
        for i, (off, ln) in enumerate(pieces):
            one = ctx.selftest_poly_eval(buf[off:off + ln], mont1(x))
            assert np.array_equal(got[i], one), (count, i, ln)
            assert unmont(got[i])[0] == _horner(B[off:off + ln], x), (count, i, ln)


# ------------------------------------------------------------------------------------------------ transform from a shorter source
@pytest.mark.parametrize("log_n", [1, 2, 3, 5, 10, 11, 12, 13, 16, 17, 20])
def test_ntt_from_a_shorter_source(ctx, orc, log_n):
    """dv_ntt_from with len in {0, 1, n/2 + 1, n - 1, n}: the oracle's transform of the zero-padded input; the source
    unchanged"""
    from pyref.prng import fr_array
    n = 1 << log_n
    full = orc.fr_to_mont(fr_array(n, 1000 + log_n))
    threads = orc.lib.oracle_max_threads()
    for ln in sorted({0, 1, n // 2 + 1, n - 1, n}):
        src = np.ascontiguousarray(full[:ln])
        padded = np.zeros((n, 4), dtype=np.uint64)
        padded[:ln] = src
        for inverse in (0, 1):
            for coset in (0, 1):
                out, back = ctx.selftest_ntt_from(src, log_n, inverse, coset)
                assert np.array_equal(back, src), "source changed"
                assert np.array_equal(out, orc.ntt(padded, log_n, inverse, coset, threads=threads)), (log_n, ln, inverse, coset)


# ------------------------------------------------------------------------------------------------ scan
@pytest.mark.parametrize("n", [0, 1, 2047, 2048, 2049, 2048 * 2048 + 1])
def test_scan_exclusive_u32(ctx, n):
    rs = np.random.default_rng(n)
    for w in (np.zeros(n, np.uint32), np.full(n, 0xFFFFFFFF, np.uint32), rs.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
              rs.integers(0, 2, n, dtype=np.uint32)):
        out, total = ctx.selftest_scan(w)
        incl = np.cumsum(w, dtype=np.uint32)
        assert np.array_equal(out, np.concatenate([[0], incl[:-1]]).astype(np.uint32) if n else out)
        assert total == (int(incl[-1]) if n else 0)


# ------------------------------------------------------------------------------------------------ bulk sampler
R_WORDS = [(R >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def _accepted(raw):
    """ark_ff UniformRand for Fp256 on a keystream (uint32 words): candidates of 8 words, top 3 bits cleared, kept when < r.
    Returns (accepted candidates as n x 4 uint64, index of each in the candidate stream)."""
    c = raw[: raw.size // 8 * 8].reshape(-1, 8).copy()
    c[:, 7] &= 0xFFFFFFFF >> 3
    lt = np.zeros(c.shape[0], dtype=bool)
    undecided = np.ones(c.shape[0], dtype=bool)
    for i in range(7, -1, -1):
        d = undecided & (c[:, i] != R_WORDS[i])
        lt[d] = c[d, i] < R_WORDS[i]
        undecided &= ~d
    idx = np.nonzero(lt)[0]
    return np.ascontiguousarray(c[idx]).view(np.uint64).reshape(-1, 4), idx


def _handles(M, kind, seed):
    """(handle under test, twin that yields the same keystream, function returning the words the handle consumed)"""
    if kind == "builtin":
        h, t = M.rng_from_seed(seed), M.rng_from_seed(seed)
        return h, t, h.word_pos
    if kind == "adopted":
        h, t = M.rng_from_chacha(seed, 3, 12), M.rng_from_chacha(seed, 3, 12)
        return h, t, h.word_pos
    caller = M.rng_from_seed(seed)
    h = M.rng_behind_callback(caller)
    return h, M.rng_from_seed(seed), caller.word_pos


def _sample_case(ctx, M, kind, need, skip, seed):
    h, twin, pos = _handles(M, kind, seed)
    if skip:
        h.fill_bytes(4 * skip)
        twin.fill_bytes(4 * skip)
    start = twin.word_pos()
    got = ctx.selftest_sample_fr(h, need)
    if need == 0:
        assert pos() == start
        return
    raw = np.frombuffer(twin.fill_bytes(32 * int(need / 0.5) + 4096), dtype=np.uint32)
    acc, idx = _accepted(raw)
    assert acc.shape[0] >= need
    assert np.array_equal(got, acc[:need]), (kind, need, skip)
    assert pos() == start + 8 * (int(idx[need - 1]) + 1), (kind, need, skip)


@pytest.mark.parametrize("kind", ["builtin", "adopted", "callback"])
def test_bulk_sampler_small_draws_at_every_block_offset(ctx, kind):
    """need in {0, 1, 2, 1000} starting 0 .. 15 words into a ChaCha block (candidates straddle two blocks)"""
    from simpleworks_amd import marlin as M
    for skip in range(16):
        for need in (0, 1, 2, 1000):
            _sample_case(ctx, M, kind, need, skip, bytes([skip + 1, 7, len(kind)] + [0] * 29))


@pytest.mark.parametrize("kind", ["builtin", "adopted", "callback"])
@pytest.mark.parametrize("need,skip", [(160_000, 0), (160_000, 5), (1_600_000, 11)])
def test_bulk_sampler_long_draws(ctx, kind, need, skip):
    """a draw just over one 2^18-candidate chunk, and one (~2.8 M candidates) that wraps the 4-slot host ring of a
    caller-owned generator and reuses its in-flight totals"""
    from simpleworks_amd import marlin as M
    _sample_case(ctx, M, kind, need, skip, bytes([need % 251, skip, 9] + [0] * 29))


# ------------------------------------------------------------------------------------------------ callback mode at size
@pytest.mark.parametrize("name", ["synthetic_2p16", "synthetic_2p18", "synthetic_2p20"])
def test_callback_rng_golden_proof_bytes_at_size(name):
    """setup + index with the built-in generator, then the proof through a caller-owned generator adopted at the built-in's
    word position: the committed bytes, and the caller's generator ends where the built-in one does after the same proof"""
    from simpleworks_amd import marlin as M, serialization as S, workloads as W
    case = golden("marlin_large.json")[name]
    rng = M.generate_rand()
    srs = M.generate_universal_srs(*case["srs"], rng)
    cs, public = W.synthetic_r1cs(case["num_constraints"], h2i(case["a"]), h2i(case["b"]))
    pk, vk = M.generate_proving_and_verifying_keys(srs, cs)
    srs.free()
    caller = M.rng_from_chacha(M.TEST_RNG_SEED, rng.word_pos(), 12)
    proof = S.serialize_proof(M.generate_proof(cs, pk, M.rng_behind_callback(caller)))
    for source, want in expected_bytes("marlin_large.json", name, "proof"):
        assert proof.hex() == want, "proof vs %s" % source
    assert S.serialize_proof(M.generate_proof(cs, pk, rng)) == proof
    assert caller.word_pos() == rng.word_pos()
    pk.free()

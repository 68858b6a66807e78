"""Whole MSMs over twisted Edwards tables in the 29-bit limb form (csrc/fq29.cuh: msm_te_convert<29-bit rows>, msm_accumulate_te,
msm_accumulate_te_quad and their epilogue into the 28-bit domain) against the CPU oracle, on subgroup bases [tau^i]G.

Sizes: 512 and 513 points (the first sets that get a table, hence the flat schedule), 2^12 + 1, 2^15 + 3 — all of them jobs of at
most 2^20 digits, which msm_accumulate_te_quad accumulates — and 2^18 + 1, the first size past the low-latency variant: the
one-lane msm_accumulate_te with 128-entry segments.  Every scalar vector holds 0, 1, r - 1, scalars whose digits are all at the
largest positive and at the largest negative value of the recoding for every table width from 11 to 22 bits (+2^(c-1) and
-(2^(c-1) - 1): with c = 20, +2^19 and -(2^19 - 1)), and scalars repeated once, twice, 128 and 300 times, so that their buckets
are segments of length 1, 2 and exactly one full segment, and buckets of several segments.  Some bases are the identity, some
of them under the repeated scalars.  A twin pair (a lead and a follower sharing one sort) runs on a set without identities.  Every result
must equal the oracle's as a group element."""
import numpy as np
import pytest

from oracle_lib import Oracle, golden, h2i, ints_to_limbs, R

SIZES = (512, 513, (1 << 12) + 1, (1 << 15) + 3, (1 << 18) + 1)
N_TWIN = (1 << 15) + 3      # at least msm_twin_match's 32768
HOLES = (0, 5, 100, 301, 511)


def extreme_digit_scalars():
    """per table width c: every window at 2^(c-1) (digits +2^(c-1), no carry), and window 0 at 2^(c-1) + 1 with every later one
    at 2^(c-1) (each digit then is negative and carries into the next: -(2^(c-1) - 1) throughout); windows as msm_table_layout
    cuts them (254 bits over ceil(254 / c) windows, the first ones a bit wider), top windows dropped while the value exceeds r"""
    out = []
    for c in range(11, 23):
        nwin = -(-254 // c)
        base, extra = divmod(254, nwin)
        widths = [base + (1 if w < extra else 0) for w in range(nwin)]
        for first_plus in (0, 1):
            use = nwin
            while True:
                s, bit = 0, 0
                for w in range(use):
                    s += ((1 << (widths[w] - 1)) + (first_plus if w == 0 else 0)) << bit
                    bit += widths[w]
                if s < R:
                    break
                use -= 1
            out.append(s)
    return out


def scalars_for(n, seed):
    from pyref.prng import fr_array
    sc = fr_array(n, seed)
    special = [0, 1, R - 1] + extreme_digit_scalars()
    rep = [int(v) for v in np.random.default_rng(seed).integers(1, 1 << 62, size=4)]
    special += [rep[0]] + [rep[1]] * 2 + [rep[2] | (1 << 200)] * 128 + [R - rep[3]] * 300
    assert len(special) <= n
    # the repeated scalars start at row 0, so that the identity bases of HOLES fall under them and under the plain ones alike
    order = special[27:] + special[:27]
    sc[:len(order)] = ints_to_limbs(order, 4)
    return sc


@pytest.fixture(scope="module")
def env():
    import simpleworks_amd as swm
    orc = Oracle()
    tau = h2i(golden("msm.json")["tau"])
    G = orc.points_to_mont([tuple(h2i(v) for v in golden("g1.json")["generator"])])
    bases = orc.srs_bases(max(SIZES), tau, G)
    bases[list(HOLES)] = 0
    bases[max(SIZES) - 2] = 0
    ctx = swm.Context(0)
    yield orc, ctx, bases
    ctx.close()


def affine(orc, ctx, jac):
    xy, inf = ctx.g1_normalize(jac)
    return None if inf else orc.points_from_mont(xy.reshape(1, 12))[0]


def test_scalar_vectors_hold_what_they_claim():
    """No device: the special scalars are reduced, the extreme ones have the digits they are named after under the recoding."""
    ext = extreme_digit_scalars()
    assert len(ext) == 24 and all(0 < s < R for s in ext)
    c, nwin = 20, 13
    base, extra = divmod(254, nwin)
    for s, want in ((ext[2 * (c - 11)], lambda w: 1 << (w - 1)), (ext[2 * (c - 11) + 1], lambda w: -((1 << (w - 1)) - 1))):
        carry, bit, seen = 0, 0, []
        for w in range(nwin):
            wd = base + (1 if w < extra else 0)
            d = ((s >> bit) & ((1 << wd) - 1)) + carry
            carry = 1 if d > (1 << (wd - 1)) else 0
            d -= carry << wd
            if d and not (d == 1 and want(wd) < 0):   # (the last negative digit's carry: a lone 1 in the window above)
                assert d == want(wd), (w, d)
                seen.append(d)
            bit += wd
        assert len(seen) >= nwin - 1
    sc = scalars_for(512, 1)
    assert sc.shape == (512, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_msm_equals_the_oracle(env, n):
    orc, ctx, bases = env
    b = np.ascontiguousarray(bases[:n])
    sc = scalars_for(n, 2900 + n % 97)
    bh = ctx.srs_upload(b)
    try:
        got = affine(orc, ctx, ctx.msm_g1(bh, sc))
    finally:
        bh.free()
    assert got == orc.jac_to_affine_int(orc.msm(b, sc, threads=orc.lib.oracle_max_threads())), n


@pytest.mark.gpu
def test_twin_pair_equals_the_oracle(env):
    """a lead at offset 0 and its follower in the upper half of a set of 2 x 32771 points, one scalar vector: the follower accumulates from the
    lead's sort (twins == 1), both through the 29-bit rows"""
    orc, ctx, bases = env
    lo = max(HOLES) + 1                      # a set with an identity base keeps every job on a sort of its own (msm_twin_match)
    b = np.ascontiguousarray(bases[lo:lo + 2 * N_TWIN])
    assert b.any(axis=1).all()
    sc = scalars_for(N_TWIN, 2999)
    hi = N_TWIN
    bh = ctx.srs_upload(b)
    try:
        jacs, twins = ctx.selftest_msm_jobs([bh], [sc], [(0, 0, 0, N_TWIN, "lead"), (0, hi, 0, N_TWIN, "follow")])
        got = [affine(orc, ctx, j) for j in jacs]
    finally:
        bh.free()
    assert twins == 1
    threads = orc.lib.oracle_max_threads()
    for off, g in zip((0, hi), got):
        assert g == orc.jac_to_affine_int(orc.msm(np.ascontiguousarray(b[off:off + N_TWIN]), sc, threads=threads)), off

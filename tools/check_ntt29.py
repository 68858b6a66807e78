#!/usr/bin/env python3
"""Bit-level emulation of the lazy 29-bit transform arithmetic of simpleworks_amd/csrc/fr29.cuh + ntt.hip (ntt_pass_lazy): every
uint32 limb operation and every 64-bit column sum is checked for wrap-around, the value bounds the host plan assumes are asserted,
and whole small transforms (every pass plan up to 2^12, forward / inverse / coset) are compared with a direct DFT in Python
integers.  Besides random data it feeds the inputs at which the plan's bounds are tight (edge_inputs / tile_patterns: constants,
combs of r - 1 and 0 at every butterfly distance, single elements, root orbits), whole transforms of those against their closed
forms; tests/test_gpu_ntt_edges.py runs the same inputs through the device code.  CPU only, about six minutes of pure Python
(tests/test_ntt29_emulation.py runs a ten-second subset); run: python tools/check_ntt29.py"""
import random, sys

R = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001
M29 = (1 << 29) - 1
R261 = (1 << 261) % R
GEN = 22
ROOT47 = pow(GEN, (R - 1) >> 47, R)


def limbs(v):
    assert 0 <= v < 1 << 264
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def val(l):
    return sum(x << (29 * i) for i, x in enumerate(l))


def spread(k, sub):
    """limbs of k*r with sub * 2^29 borrowed into every limb below the top one"""
    q = limbs(k * R)
    l = [q[0] + sub * (1 << 29)] + [q[i] + sub * (1 << 29) - sub for i in range(1, 8)] + [q[8] - sub]
    assert val(l) == k * R and l[8] > 0
    return l


P29 = limbs(R)
ONE = limbs(R261)
assert P29[0] == 1


def u32(x):
    assert 0 <= x < 1 << 32, "uint32 wrap"
    return x


def mul(a, b, top_bits=23):
    """fr29_mul: a may be lazy (limbs < 2^32), b normalised (limbs < 2^29: a table entry, or the product of two); a b < 2^261 r.
    top_bits: what the caller promises for b's top limb (the transform: a value < 2r; tools/check_poseidon29.py: < 9r)."""
    assert all(0 <= x < 1 << 32 for x in a) and all(0 <= x < 1 << 29 for x in b[:8]) and b[8] < 1 << top_bits
    assert val(a) * val(b) < (1 << 261) * R, "product too large for a result below 2r"
    m, r, acc = [0] * 9, [0] * 9, 0
    for k in range(9):
        for i in range(k + 1):
            acc += a[i] * b[k - i]
        for i in range(k):
            acc += m[i] * P29[k - i]
        assert acc < 1 << 64, "column sum wraps"
        m[k] = (-acc) & M29
        t = acc + M29  # the carry rule of fr29_mul_asm: one 64-bit add, one bit-select, one shift
        assert t < 1 << 64 and (~t) & M29 == m[k] and t >> 29 == (acc + m[k]) >> 29, "asm carry rule"
        acc = (acc + m[k]) >> 29
    for k in range(9, 17):
        for i in range(k - 8, 9):
            acc += a[i] * b[k - i]
        for i in range(k - 8, 9):
            acc += m[i] * P29[k - i]
        assert acc < 1 << 64, "column sum wraps"
        r[k - 9] = acc & M29
        acc >>= 29
    r[8] = acc
    assert val(r) < 2 * R and (val(r) * (1 << 261) - val(a) * val(b)) % R == 0
    return r


def add(a, b):
    return [u32(x + y) for x, y in zip(a, b)]


def sub(a, b, sp):
    return [u32(x + s - y) for x, y, s in zip(a, b, sp)]


def normalize(a):
    r, c = [0] * 9, 0
    for i in range(8):
        t = u32(a[i] + c)
        r[i] = t & M29
        c = t >> 29
    r[8] = u32(a[8] + c)
    return r


def canonical(a, bound):
    """normalised value < bound * r (bound <= 4) -> < r: conditional subtractions of 2r and r"""
    v = val(a)
    assert v < bound * R
    if bound > 2 and v >= 2 * R:
        v -= 2 * R
    if v >= R:
        v -= R
    return limbs(v)


# ---- the host plan of one pass: spreads and y0 reductions per step (mirrors ntt.hip plan_lazy_pass)
def plan(log_r, b0):
    steps, B = [], b0
    if log_r & 1:
        steps.append(("r2", B))
        B = max(2 * B, 2)
    for s in range(log_r // 2):
        last = s == log_r // 2 - 1
        red = 4 * B > 64 or last
        assert B <= 64
        steps.append(("r4", B, red))
        B = 4 if red else 4 * B
    if log_r == 1:
        B = max(B, 2)
    return steps, B


def tile_transform(x, log_r, tw_small, b0):
    """x: list of 2^log_r Fr29 (normalised, value < b0 r).  DIF in place (bit-reversed out), as the kernel's LDS phase."""
    Rn = 1 << log_r
    steps, _ = plan(log_r, b0)
    h = Rn >> 1
    t = list(x)
    for st in steps:
        if st[0] == "r2":
            B = st[1]
            S = spread(2 * B, 1)
            for pos in range(h):
                u, v = t[pos], t[pos + h]
                assert val(u) < B * R and val(v) < B * R
                t[pos] = normalize(add(u, v))
                t[pos + h] = mul(sub(u, v, S), tw_small[pos])
            h >>= 1
        else:
            _, B, red = st
            S1, S2, S4 = spread(2 * B, 1), spread(4 * B, 2), spread(4, 1)
            hh, s1 = h >> 1, (Rn >> 1) // h
            s2 = 2 * s1
            for qq in range(Rn >> 2):
                p, blk = qq & (hh - 1), qq // hh
                i0 = blk * 2 * h + p
                i1, i2, i3 = i0 + hh, i0 + h, i0 + h + hh
                x0, x1, x2, x3 = t[i0], t[i1], t[i2], t[i3]
                for e in (x0, x1, x2, x3):
                    assert val(e) < B * R and all(l < 1 << 29 for l in e[:8])
                a0 = add(x0, x2)
                a2 = mul(sub(x0, x2, S1), tw_small[p * s1])
                a1 = add(x1, x3)
                a3 = mul(sub(x1, x3, S1), tw_small[(p + hh) * s1])
                w = tw_small[p * s2]
                y0 = add(a0, a1)
                y0 = mul(y0, ONE) if red else normalize(y0)
                y1 = mul(sub(a0, a1, S2), w)
                y2 = normalize(add(a2, a3))
                y3 = mul(sub(a2, a3, S4), w)
                t[i0], t[i1], t[i2], t[i3] = y0, y1, y2, y3
            h >>= 2
    return t


def bitrev(x, bits):
    return int(bin(x)[2:].zfill(bits)[::-1], 2) if bits else 0


def root(log_n, inverse):
    w = pow(ROOT47, 1 << (47 - log_n), R)
    return pow(w, R - 2, R) if inverse else w


def pass_radices(log_n, maxr=10):
    """log_r of every pass (ntt_run_multi: as few passes as maxr allows, the larger radices first)"""
    npass = 1 if log_n <= maxr else (log_n + maxr - 1) // maxr
    radices, rem = [], log_n
    for p in range(npass):
        r = (rem + (npass - p) - 1) // (npass - p)
        radices.append(r)
        rem -= r
    return radices


def ntt_lazy(x, log_n, inverse, coset, maxr=10):
    """whole transform with the kernel's pass plan (Stockham index maps of ntt_pass), lazy arithmetic, natural in / out"""
    n = 1 << log_n
    radices = pass_radices(log_n, maxr)
    npass = len(radices)
    w = root(log_n, inverse)
    g = pow(GEN, R - 2, R) if inverse else GEN
    to29 = lambda v: limbs(v % R * R261 % R)          # twiddles: x 2^261 (Montgomery form of the lazy domain)
    src = [limbs(v) for v in x]                       # data stays in whatever domain it came in (the factor is invariant)
    log_ns = 0
    for p, log_r in enumerate(radices):
        Rn, stride = 1 << log_r, n >> log_r
        ns_mask, tw_shift = (1 << log_ns) - 1, log_n - log_ns - log_r
        coset_in = coset and not inverse and p == 0
        last = p == npass - 1
        b0 = 4 if p > 0 else 1
        tw_small = [to29(pow(root(log_r, inverse), e, R)) for e in range(max(Rn >> 1, 1))]
        dst = [None] * n
        b_in = 2 if (p > 0 or coset_in) else 1
        _, b_out = plan(log_r, b_in)
        for j in range(stride):
            tile = []
            for t in range(Rn):
                idx = j + t * stride
                xx = src[idx]
                assert val(xx) < b0 * R
                if coset_in:
                    xx = mul(xx, to29(pow(g, idx, R)))
                if log_ns:
                    k = j & ns_mask
                    xx = mul(xx, to29(pow(w, (k * t) << tw_shift, R)))      # always (w^0 = one): a uniform bound after the load
                tile.append(xx)
            tile = tile_transform(tile, log_r, tw_small, b_in)
            k = j & ns_mask
            for u in range(Rn):
                o = ((j - k) << log_r) + k + (u << log_ns)
                y = tile[bitrev(u, log_r)]
                assert val(y) < b_out * R <= 4 * R
                if last and inverse:
                    s = pow(n, R - 2, R)
                    if coset:
                        s = s * pow(g, o, R) % R
                    y = canonical(mul(y, to29(s)), 2)
                elif last:
                    y = canonical(normalize(y), b_out)
                dst[o] = y
        src = dst
        log_ns += log_r
    return [val(v) for v in src]


def dft(x, log_n, inverse, coset):
    n = 1 << log_n
    w = root(log_n, inverse)
    if coset and not inverse:
        x = [v * pow(GEN, i, R) % R for i, v in enumerate(x)]
    out = [sum(x[i] * pow(w, i * k, R) for i in range(n)) % R for k in range(n)]
    if inverse:
        ni = pow(n, R - 2, R)
        out = [v * ni % R for v in out]
        if coset:
            gi = pow(GEN, R - 2, R)
            out = [v * pow(gi, i, R) % R for i, v in enumerate(out)]
    return out


# ---- inputs at the edges of the plan's bounds.  An input is a description, materialised here as Python integers and in
# tests/test_gpu_ntt_edges.py as numpy limbs; the values are MEMORY integers (the transform is linear and the lazy kernel keeps the
# factor the data came with, so r - 1 in memory is the extreme whatever it stands for):
#   ("const", c)          every element c
#   ("comb", p, hi)       r - 1 where bit p of the index is 0 and 0 elsewhere (hi = 1: the largest differences at the butterfly level
#                         that pairs indices 2^p apart), or the complement (hi = 0: the most negative differences)
#   ("single", i)         r - 1 at index i, 0 elsewhere
#   ("fill", i, rev)      r - 1 everywhere except a 0 at index i (rev = 0), or the reverse (which is a single)
#   ("orbit", s)          x_i = (r - 1) w^(s i): the forward transform is n (r - 1) at index -s mod n and exactly 0 elsewhere
TOP = R - 1


def edge_inputs(log_n, radix0=None, reduced=False):
    """The input descriptions for a transform of 2^log_n elements whose first pass has radix 2^radix0.  reduced: the combs only at
    the levels next to the pass boundary and at both ends (what the sizes above 2^13 run on the device)."""
    n = 1 << log_n
    radix0 = pass_radices(log_n)[0] if radix0 is None else radix0
    stride = n >> radix0
    ps = sorted({0, radix0 - 1, radix0, log_n - 1} & set(range(log_n))) if reduced else range(log_n)
    out = [("const", TOP), ("const", 1), ("const", 0)]
    out += [("comb", p, hi) for p in ps for hi in (1, 0)]
    if not reduced:
        out += [("single", i) for i in sorted({0, 1, n // 2 - 1, n // 2, n - 1, stride - 1, stride, stride + 1} & set(range(n)))]
        out += [("fill", i, rev) for i in sorted({0, n - 1}) for rev in (0, 1)]
    out += [("orbit", s) for s in sorted({1 % n, n // 2, n - 1})]
    return out


def materialize(d, log_n):
    n = 1 << log_n
    if d[0] == "const":
        return [d[1]] * n
    if d[0] == "comb":
        return [TOP if ((i >> d[1]) & 1) != d[2] else 0 for i in range(n)]
    if d[0] == "single":
        return [TOP if i == d[1] else 0 for i in range(n)]
    if d[0] == "fill":
        return [(TOP if i == d[1] else 0) if d[2] else (0 if i == d[1] else TOP) for i in range(n)]
    assert d[0] == "orbit"
    w, x, out = pow(root(log_n, False), d[1], R), TOP, []
    for i in range(n):
        out.append(x)
        x = x * w % R
    return out


_powers = {}


def root_powers(log_n):
    if log_n not in _powers:
        w, x, t = root(log_n, False), 1, []
        for i in range(1 << log_n):
            t.append(x)
            x = x * w % R
        _powers[log_n] = t
    return _powers[log_n]


def closed_form(d, log_n, inverse, coset):
    """The transform of input d in Python integers WITHOUT a transform: the polynomial sum x_i z^i of every family has a closed
    form, evaluated at z_k = 22^coset w^k (forward) or w^-k (inverse, then 1/n and 22^-k)."""
    n, W = 1 << log_n, root_powers(log_n)
    mask = n - 1
    sgn = -1 if inverse else 1
    g = GEN if (coset and not inverse) else 1          # z_k = g w^(sgn k)
    gn = pow(g, n, R)                                   # z_k^n
    gpow = [pow(g, 1 << b, R) for b in range(log_n)]

    def geom(ys):                                       # sum_{i < n} y^i for every y of ys (y^n = gn), one inversion for all
        den = [(y - 1) % R or 1 for y in ys]
        pre, acc = [], 1
        for v in den:
            pre.append(acc)
            acc = acc * v % R
        inv, out = pow(acc, -1, R), [0] * len(ys)
        for k in range(len(ys) - 1, -1, -1):
            out[k] = n % R if ys[k] == 1 else (gn - 1) * (inv * pre[k] % R) % R
            inv = inv * den[k] % R
        return out

    def z_pow(k, e):                                    # z_k^e
        return pow(g, e, R) * W[(sgn * k * e) & mask] % R

    def poly(d):
        if d[0] == "const":
            return [d[1] * v % R for v in geom([g * W[(sgn * k) & mask] % R for k in range(n)])]
        if d[0] == "single":
            return [TOP * z_pow(k, d[1]) % R for k in range(n)]
        if d[0] == "fill":
            one = poly(("single", d[1]))
            return one if d[2] else [(a - b) % R for a, b in zip(poly(("const", TOP)), one)]
        if d[0] == "orbit":
            return [TOP * v % R for v in geom([g * W[(d[1] + sgn * k) & mask] % R for k in range(n)])]
        assert d[0] == "comb"                           # prod over b != p of (1 + z^(2^b)), times z^(2^p) for the complement
        out = []
        for k in range(n):
            acc = TOP if d[2] else TOP * gpow[d[1]] % R * W[((sgn * k) << d[1]) & mask] % R
            for b in range(log_n):
                if b != d[1]:
                    acc = acc * (1 + gpow[b] * W[((sgn * k) << b) & mask]) % R
            out.append(acc)
        return out

    out = poly(d)
    if inverse:
        ni, gi, s = pow(n, -1, R), pow(GEN, -1, R) if coset else 1, 1
        for k in range(n):
            out[k] = out[k] * ni % R * s % R
            s = s * gi % R
    return out


def tile_patterns(log_r, b0):
    """Whole tiles at the input bound b0 r of a pass: all at the top, all zero, and top / 0 alternating at every butterfly distance"""
    Rn, top = 1 << log_r, b0 * R - 1
    yield [top] * Rn
    yield [0] * Rn
    for p in range(log_r):
        for hi in (1, 0):
            yield [top if ((i >> p) & 1) != hi else 0 for i in range(Rn)]


def check_tiles(max_log_r):
    """every pattern through one tile of every size up to 2^max_log_r and both input bounds: only the assertions speak"""
    count = 0
    for log_r in range(1, max_log_r + 1):
        tw = [limbs(pow(root(log_r, False), e, R) * R261 % R) for e in range(max((1 << log_r) >> 1, 1))]
        for b0 in (1, 2):
            for xs in tile_patterns(log_r, b0):
                tile_transform([limbs(v) for v in xs], log_r, tw, b0)
                count += 1
    return count


def check_edge_transforms(plans, variants=((False, False), (False, True), (True, False), (True, True)), reduced=False):
    """whole transforms of the edge inputs with the kernel's plan against the closed forms (and so the closed forms, which the
    device test uses, against the emulated arithmetic)"""
    count = 0
    for log_n, maxr in plans:
        for d in edge_inputs(log_n, pass_radices(log_n, maxr)[0], reduced):
            x = materialize(d, log_n)
            for inverse, coset in variants:
                assert ntt_lazy(x, log_n, inverse, coset, maxr) == closed_form(d, log_n, inverse, coset), (d, log_n, maxr, inverse, coset)
                count += 1
    return count


PLANS = ((1, 10), (2, 10), (3, 10), (5, 10), (6, 10), (7, 3), (8, 4), (9, 3), (6, 2), (10, 10))


def main():
    random.seed(11)
    # worst-case limbs through one multiplication: lazy operand with every lower limb at 2.5 * 2^30 and the value at the 446 r edge
    big = [min((5 << 29) - 1, (1 << 32) - 1)] * 8 + [0]
    big[8] = ((1 << 261) - 1 - val(big)) >> 232
    mul(big, limbs(R - 1))
    for log_r in range(1, 13):                       # every tile size (11, 12: SWM_NTT_MAXR), random data at the bound of the plan
        for b0 in (1, 2):
            tw = [limbs(pow(root(log_r, False), e, R) * R261 % R) for e in range(max((1 << log_r) >> 1, 1))]
            xs = [limbs(random.randrange(b0 * R)) for _ in range(1 << log_r)]
            xs[0] = limbs(b0 * R - 1)
            tile_transform(xs, log_r, tw, b0)
    checked = 0
    for log_n, maxr in PLANS:
        x = [random.randrange(R) for _ in range(1 << log_n)]
        for inverse in (False, True):
            for coset in (False, True):
                assert ntt_lazy(x, log_n, inverse, coset, maxr) == dft(x, log_n, inverse, coset), (log_n, maxr, inverse, coset)
                checked += 1
    for log_n in (1, 2, 3, 5, 6):                    # the closed forms themselves against the direct DFT (quadratic: small sizes)
        for d in edge_inputs(log_n):
            for inverse in (False, True):
                for coset in (False, True):
                    assert closed_form(d, log_n, inverse, coset) == dft(materialize(d, log_n), log_n, inverse, coset), (d, log_n)
    tiles = check_tiles(12)
    edges = check_edge_transforms(PLANS)
    print("fr29 emulation OK: %d transforms equal the direct DFT, %d extremal tiles and %d transforms of extremal inputs (equal to "
          "their closed forms); no uint32 / uint64 wrap, all plan bounds hold" % (checked, tiles, edges))


if __name__ == "__main__":
    main()

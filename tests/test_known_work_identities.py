"""The field identities the prover relies on where it does not compute a value it already has (csrc/marlin_prove.hip: round1_polys,
round3_polys, round3_a_minus_bf), on Python integers and the model's own index (oracle/pyref), no GPU:

* round 1: interpolation over H is linear and deg x < |X| <= |H|, so interp_H(z) - x = interp_H(z - x on H): x is never
  evaluated on H, and z on the X-subgroup positions of H is the instance itself;
* round 3: f is a / b on K by construction, so a - b f vanishes on every fourth point of the 4|K| domain;
* round 3: the form of a - b f with 16 products is the one with 18."""
import random

import pytest

import differential_model as D
from pyref import marlin as M
from pyref.bls12_377 import R
from pyref.poly import Domain, batch_inverse


def _assignment(kind, n, rnd):
    return [0] * n if kind == "zero" else [R - 1] * n if kind == "r-1" else [rnd.randrange(R) for _ in range(n)]


@pytest.mark.parametrize("kind", ["zero", "r-1", "random"])
@pytest.mark.parametrize("H", [8, 64])
@pytest.mark.parametrize("X_of", ["1", "2", "H/2"])
def test_interpolation_minus_x_is_interpolation_of_the_difference(H, X_of, kind):
    X = {"1": 1, "2": 2, "H/2": H // 2}[X_of]
    rnd = random.Random(H * 1000 + X)
    dh, dx = Domain(H), Domain(X)
    ratio = H // X
    inst = [1] + _assignment(kind, X - 1, rnd)   # the formatted input: the constant one in front
    wit = _assignment(kind, H - X, rnd)
    x_poly = dx.ifft(inst)
    x_evals = dh.fft(x_poly)
    # the X-subgroup positions of H hold the instance: what round 2 reads there instead of x's evaluations
    assert [x_evals[k] for k in range(0, H, ratio)] == inst
    z_on_H = [inst[k // ratio] if k % ratio == 0 else wit[k - k // ratio - 1] for k in range(H)]
    model = dh.ifft([0 if k % ratio == 0 else (z_on_H[k] - x_evals[k]) % R for k in range(H)])   # pyref.marlin.prove, round 1
    ours = dh.ifft(z_on_H)
    for i in range(X):
        ours[i] = (ours[i] - x_poly[i]) % R
    assert ours == model


def _index_arith(params):
    """The model's arithmetisation of a system of differential_model.emit (pyref.marlin.index without the commitments)."""
    cs = M.ConstraintSystem()
    D.emit(cs, params)
    ics = M.pad_and_square(cs)
    a, b, c = ics.to_matrices()
    nnz = max(sum(len(r) for r in m) for m in (a, b, c))
    M.balance_matrices(a, b)
    dh, dk, dx = Domain(ics.num_constraints), Domain(nnz), Domain(len(ics.instance))
    db = Domain(3 * dk.size - 3)
    return {n: M._arithmetize(m, dk, dh, dx, db) for n, m in (("a", a), ("b", b), ("c", c))}, dh, dk, db


def _outside(dh, rnd):
    while True:
        v = rnd.randrange(R)
        if dh.vanishing(v):
            return v


@pytest.mark.parametrize("K,params", [(16, dict(seed=301, inputs=2, free=2, rows=12, a=[1, 1], b=[1, 1])),
                                      (32, dict(seed=302, inputs=3, free=4, rows=24, a=[1, 1], b=[1, 1]))])
def test_a_minus_bf_vanishes_on_K(K, params):
    ar, dh, dk, db = _index_arith(params)
    assert dk.size == K and db.size == 4 * K
    rnd = random.Random(K)
    alpha, beta = _outside(dh, rnd), _outside(dh, rnd)
    etas = {m: rnd.randrange(R) for m in "abc"}
    vhab = dh.vanishing(alpha) * dh.vanishing(beta) % R
    # f on K by the prover's formula (pyref.marlin.prove, round 3), then on the 4|K| domain
    inv = {m: batch_inverse([(beta - ar[m]["row_K"][i]) * (alpha - ar[m]["col_K"][i]) % R for i in range(K)]) for m in "abc"}
    f_K = [vhab * (sum(etas[m] * ar[m]["val_K"][i] % R * inv[m][i] for m in "abc") % R) % R for i in range(K)]
    f_B = db.fft(dk.ifft(f_K))
    assert f_B[0::4] == f_K
    den = {m: [(beta * alpha - ar[m]["row_B"][i] * alpha - beta * ar[m]["col_B"][i] + ar[m]["row_col_B"][i]) % R
               for i in range(4 * K)] for m in "abc"}
    diff = []
    for i in range(4 * K):
        t = (etas["a"] * ar["a"]["val_B"][i] % R * den["b"][i] % R * den["c"][i]
             + etas["b"] * ar["b"]["val_B"][i] % R * den["a"][i] % R * den["c"][i]
             + etas["c"] * ar["c"]["val_B"][i] % R * den["a"][i] % R * den["b"][i]) % R
        diff.append((vhab * t - den["a"][i] * den["b"][i] % R * den["c"][i] % R * f_B[i]) % R)
    assert all(diff[4 * j] == 0 for j in range(K))          # every kappa in K
    assert any(diff[i] for i in range(4 * K) if i % 4)      # (and a - b f is not the zero polynomial)


def _form18(row, col, rc, val, alpha, beta, eta, vhab, f):
    d = [(beta * alpha - row[m] * alpha - beta * col[m] + rc[m]) % R for m in range(3)]
    t = (eta[0] * val[0] % R * (d[1] * d[2] % R) + eta[1] * val[1] % R * d[0] % R * d[2] + eta[2] * val[2] % R * d[0] % R * d[1]) % R
    return (vhab * t - d[0] * (d[1] * d[2] % R) % R * f) % R


def _form16(row, col, rc, val, alpha, beta, eta, vhab, f):
    d = [(beta * alpha - row[m] * alpha - beta * col[m] + rc[m]) % R for m in range(3)]
    u = [vhab * eta[m] % R * val[m] % R for m in range(3)]   # (vhab eta_M: formed once on the host)
    dbc = d[1] * d[2] % R
    a = (u[0] * dbc + d[0] * ((u[1] * d[2] + u[2] * d[1]) % R)) % R
    return (a - d[0] * dbc % R * f) % R


def test_sixteen_product_form_is_the_eighteen_product_form():
    rnd = random.Random(16)
    draws = [lambda: 0, lambda: R - 1, lambda: rnd.randrange(R)]
    cases = [[c() for _ in range(18)] for c in draws[:2]]
    cases += [[rnd.choice(draws)() for _ in range(18)] for _ in range(200)]
    cases += [[rnd.randrange(R) for _ in range(18)] for _ in range(200)]
    for v in cases:
        args = (v[0:3], v[3:6], v[6:9], v[9:12], v[12], v[13], v[14:17], v[17], rnd.choice(draws)())
        assert _form16(*args) == _form18(*args)

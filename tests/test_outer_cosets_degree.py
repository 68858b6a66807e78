"""The degree bound behind round 2 on three cosets of H (marlin_prove.hip, SWM_OUTER_COSETS): q_1 - mask, interpolated from the 4|H|
product domain the way the model does it, has no coefficient at index >= 3|H|, so its values on the cosets 0, 1, 2 of H determine
it.  CPU only: round 1 and round 2 of the Python model (oracle/pyref/marlin.py prove) with random challenges and blinding values
in place of the commitments and the transcript, on circuits of 2^8 ... 2^12 constraints, |X| = 4 and |X| = 8."""
import random

import pytest

from pyref import marlin as PM
from pyref.bls12_377 import R
from pyref.poly import Domain, poly_add, poly_divide_by_vanishing, poly_mul, poly_mul_by_vanishing, poly_trim


def _q1_minus_mask(cs, rnd):
    """prove()'s round-2 polynomial before the mask is added, from the 4|H| domain; (q_1 - mask, |H|, |X|, mask length)"""
    pcs = PM.pad_and_square(cs)
    a, b, c = pcs.to_matrices()
    PM.balance_matrices(a, b)
    formatted_input, witness = list(pcs.instance), list(pcs.witness)
    z = formatted_input + witness
    z_a = [sum(v * z[col] for v, col in row) % R for row in a]
    z_b = [sum(v * z[col] for v, col in row) % R for row in b]
    dh, dx = Domain(pcs.num_constraints), Domain(len(formatted_input))
    H = dh.size
    x_poly = poly_trim(dx.ifft(formatted_input))
    x_evals = dh.fft(x_poly)
    ratio = H // dx.size
    w_extended = witness + [0] * (H - dx.size - len(witness))
    w_evals = [0 if k % ratio == 0 else (w_extended[k - k // ratio - 1] - x_evals[k]) % R for k in range(H)]
    w_poly = poly_add(dh.ifft(w_evals), poly_mul_by_vanishing([rnd.randrange(R)], dh))
    w_poly, rem = poly_divide_by_vanishing(w_poly, dx)
    assert not rem
    z_a_poly = poly_add(dh.ifft(z_a), poly_mul_by_vanishing([rnd.randrange(R)], dh))
    z_b_poly = poly_add(dh.ifft(z_b), poly_mul_by_vanishing([rnd.randrange(R)], dh))
    alpha = rnd.randrange(R)
    eta_a, eta_b, eta_c = (rnd.randrange(R) for _ in range(3))
    summed = [v * eta_c % R for v in poly_mul(z_a_poly, z_b_poly)]
    for i in range(min(len(summed), len(z_a_poly), len(z_b_poly))):
        summed[i] = (summed[i] + eta_a * z_a_poly[i] + eta_b * z_b_poly[i]) % R
    summed = poly_trim(summed)
    r_alpha_evals = dh.batch_eval_unnormalized_bivariate_lagrange_poly_with_diff_inputs(alpha)
    r_alpha_poly = poly_trim(dh.ifft(r_alpha_evals))
    t_evals = [0] * H
    for matrix, eta in ((a, eta_a), (b, eta_b), (c, eta_c)):
        for r, row in enumerate(matrix):
            for coeff, col in row:
                k = dh.reindex_by_subdomain(dx, col)
                t_evals[k] = (t_evals[k] + eta * coeff % R * r_alpha_evals[r]) % R
    t_poly = poly_trim(dh.ifft(t_evals))
    z_poly = poly_mul_by_vanishing(w_poly, dx)
    z_poly = z_poly + [0] * (len(x_poly) - len(z_poly))
    for i, xc in enumerate(x_poly):
        z_poly[i] = (z_poly[i] + xc) % R
    z_poly = poly_trim(z_poly)
    mask_len = 3 * H + 2 * PM.ZK_BOUND - 2
    mul_size = max(mask_len, len(r_alpha_poly) + len(summed), len(t_poly) + len(z_poly))
    dm = Domain(mul_size)
    assert dm.size == 4 * H
    ra, sm, zp, tp = dm.fft(r_alpha_poly), dm.fft(summed), dm.fft(z_poly), dm.fft(t_poly)
    return dm.ifft([(p * q - u * v) % R for p, q, u, v in zip(ra, sm, zp, tp)]), H, dx.size, mask_len


CIRCUITS = [("synthetic_2p8", lambda: PM.synthetic_circuit(1 << 8, 3, 5)),
            ("synthetic_2p10", lambda: PM.synthetic_circuit(1 << 10, 7, 11)),
            ("synthetic_2p12", lambda: PM.synthetic_circuit(1 << 12, 13, 17)),
            ("sparse_x8_2p9", lambda: PM.random_sparse_circuit(9, num_inputs=6, free_witnesses=20, num_constraints=300)),
            ("sparse_x8_2p11", lambda: PM.random_sparse_circuit(11, num_inputs=5, free_witnesses=100, num_constraints=1500))]


@pytest.mark.parametrize("name,make", CIRCUITS, ids=[c[0] for c in CIRCUITS])
def test_q1_minus_mask_has_degree_below_3h(name, make):
    rest, H, X, mask_len = _q1_minus_mask(make(), random.Random(name))
    assert PM.ZK_BOUND == 1 and mask_len == 3 * H  # the prover's guard: zk bound 1, a mask of 3|H| coefficients
    assert H >= 1 << 8 and X > 1
    assert len(rest) == 4 * H
    assert not any(rest[3 * H:]), "q_1 - mask has a coefficient at index >= 3|H|"
    assert any(rest[2 * H:3 * H])  # (the bound is tight: the top block is in use)

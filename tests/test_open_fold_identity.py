"""Why the opening round may fold a shifted witness into the plain one (marlin_prove.hip, open_combinations): under an SRS of the
circuit's own degree the shifted powers are the top of the powers, so
    MSM(powers, wq) + MSM(powers from off on, k sq) = MSM(powers, wq + X^off k sq),      off = max_degree - degree bound,
the scalars adding in Fr because G1 has order r.  CPU only: the Python model proves the synthetic circuit at 2^8, its pc_open calls
are recorded, and for both query points the merged coefficient vector committed against the model's powers must equal the
model's witness before the hiding term."""
import pytest

from pyref import bls12_377 as bls
from pyref import marlin as PM
from pyref.bls12_377 import R
from pyref.poly import poly_add, poly_div_linear, poly_scale, poly_trim


def test_merged_witness_commits_to_the_models_witness(monkeypatch):
    n = 1 << 8
    calls = []
    pc_open = PM.pc_open

    def recording(ck, polys, point, xi, rands):
        calls.append((ck, polys, point, xi))
        return pc_open(ck, polys, point, xi, rands)

    monkeypatch.setattr(PM, "pc_open", recording)
    rng = PM.generate_rand()
    srs = PM.generate_universal_srs(n, n, n, rng)
    cs = PM.synthetic_circuit(n, 3, 5)
    pk, vk = PM.generate_proving_and_verifying_keys(srs, cs)
    PM.generate_proof(cs, pk, rng)
    assert len(calls) == 2  # beta, gamma
    grew = []
    for ck, polys, point, xi in calls:
        # the shifted powers are a sub-range of the powers: what the fold needs
        base = ck.max_degree - ck.enforced_degree_bounds[-1]
        assert base + len(ck.shifted_powers) == len(ck.powers) and list(ck.shifted_powers) == list(ck.powers[base:])
        p, merged_shift, model_shifted = [], [], None
        ctr = 0
        for label, poly, degree_bound, _hb in polys:
            p = poly_add(p, poly_scale(poly, pow(xi, ctr, R)))
            ctr += 1
            if degree_bound is not None:
                k = pow(xi, ctr, R)
                ctr += 1
                off = ck.max_degree - degree_bound
                sq = poly_scale(poly_div_linear(poly, point), k)   # after the division: X^off (g / (X - z)), not (X^off g) / (X - z)
                merged_shift = poly_add(merged_shift, [0] * off + sq)
                term = PM._msm(PM.ck_shifted_powers(ck, degree_bound), sq)
                model_shifted = term if model_shifted is None else bls.g1_add(model_shifted, term)
        assert model_shifted is not None  # g_1 at beta, g_2 at gamma
        wq = poly_div_linear(p, point)
        merged = poly_trim(poly_add(wq, merged_shift))
        assert len(merged) <= len(ck.powers)
        grew.append(len(merged) > len(poly_trim(wq)))
        two_jobs = bls.g1_add(PM._msm(ck.powers, wq), model_shifted)
        assert PM._msm(ck.powers, merged) == two_jobs
        # ... and that IS the model's witness without its hiding term
        w_model, _ = PM._open_with_witness(ck.powers, ck.powers_of_gamma_g, point, [], wq, None)
        assert two_jobs == bls.g1_add(w_model, model_shifted)
    # beta: the mask makes the plain quotient 3n - 1 long and the shifted range lies inside it; gamma: the merged vector is longer
    assert grew == [False, True]

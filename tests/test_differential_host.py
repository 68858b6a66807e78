"""CPU tests of the differential cases (tests/differential_model.py, tests/golden/differential.json): the fixture is the one
the case table generates, the product's host-side builder and the Python model lay out the same matrices for every case, and
the model still reproduces the recorded bytes (so a change of the model cannot leave a stale fixture behind)."""
import pytest

import differential_model as D
from oracle_lib import golden, h2i
from pyref import marlin as PM


@pytest.fixture(scope="module")
def fixture():
    return golden("differential.json")["cases"]


def test_fixture_is_the_case_table(fixture):
    assert [c["name"] for c in fixture] == [name for name, _ in D.CASES]
    assert [c["params"] for c in fixture] == [params for _, params in D.CASES]
    assert len(D.CASES) >= 30
    assert [c["name"] for c in fixture if not c["public_input"]] == D.NO_PUBLIC_INPUT
    for c in fixture:
        assert c["num_non_zero"] >= 2 and c["num_constraints"] == c["num_variables"]


@pytest.mark.parametrize("name", [name for name, _ in D.CASES])
def test_product_builder_and_model_lay_out_the_same_matrices(fixture, name):
    from simpleworks_amd import marlin as M
    case = {c["name"]: c for c in fixture}[name]
    model, product = PM.ConstraintSystem(), M.ConstraintSystem()
    public = D.emit(model, case["params"])
    assert D.emit(product, case["params"]) == public == [h2i(x) for x in case["public_input"]]
    assert product.instance == model.instance and product.witness == model.witness
    assert product.num_constraints == model.num_constraints
    for rows, want in zip(product.rows, model.to_matrices()):
        rowptr, col, val = product._csr(rows)
        assert list(rowptr) == [0] + [sum(len(r) for r in want[:i + 1]) for i in range(len(want))]
        assert list(col) == [c for r in want for _, c in r]
        assert val.tolist() == M._to_mont_limbs([v for r in want for v, _ in r]).tolist()
    # the raw form the GPU test feeds import_csr: the same terms, unmerged, in the builder's order
    for (rowptr, col, val), terms in zip(D.raw_csr(product, M._to_mont_limbs), (model.a, model.b, model.c)):
        assert list(rowptr) == [0] + [sum(len(r) for r in terms[:i + 1]) for i in range(len(terms))]
        assert list(col) == [model._col(var) for r in terms for _, var in r]
        assert val.tolist() == M._to_mont_limbs([c for r in terms for c, _ in r]).tolist()
    sizes = (model.num_constraints, len(model.instance) + len(model.witness),
             max(sum(len(r) for r in m) for m in model.to_matrices()))
    assert list(sizes) == case["srs"]
    assert model.is_satisfied()
    bad = model.copy()
    bad.witness[case["flip"]] = (bad.witness[case["flip"]] + 1) % PM.R
    assert not bad.is_satisfied()


def test_model_reproduces_the_two_cheapest_cases(fixture):
    """The drift guard: the model run again on the two smallest committer keys gives the recorded bytes."""
    for case in sorted(fixture, key=lambda c: c["max_degree"])[:2]:
        cs = PM.ConstraintSystem()
        D.emit(cs, case["params"])
        rng = PM.generate_rand()
        srs = PM.generate_universal_srs(*case["srs"], rng)
        assert srs.max_degree == case["max_degree"]
        pk, vk = PM.generate_proving_and_verifying_keys(srs, cs)
        assert (vk["num_constraints"], vk["num_variables"], vk["num_non_zero"]) == (
            case["num_constraints"], case["num_variables"], case["num_non_zero"])
        assert PM.serialize_verifying_key(vk).hex() == case["vk"]
        assert PM.serialize_proof(PM.generate_proof(cs, pk, rng)).hex() == case["proof"]


def test_model_refuses_an_index_with_fewer_than_two_non_zeros():
    """|K| = 1 has no degree bound |K| - 2: the model raises its MarlinError, as the product does, not an IndexError."""
    one_term = PM.ConstraintSystem()
    w = one_term.new_witness_variable(5)
    one_term.enforce_constraint([(1, w)], [], [])
    empty = PM.ConstraintSystem()
    empty.new_witness_variable(5)
    empty.enforce_constraint([], [], [])
    empty.enforce_constraint([], [], [])
    srs = PM.UniversalSRS([None] * 16, [None] * 4, None, None)  # index refuses before it reads a power
    for cs in (one_term, empty):
        with pytest.raises(PM.MarlinError, match=r"\|K\|"):
            PM.index(srs, cs)

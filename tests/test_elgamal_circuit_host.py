"""CPU tests of the ElGamal encryption circuit: its specification, workloads.build_elgamal_encryption, evaluated row by row in
Python integers on the fixture tuples of tests/golden/elgamal.json (valid and edge), on randomness at and above the group order
and on a wrong claimed ciphertext, and its SHAPE as the library states it without a GPU (swm_elgamal_circuit_shape,
csrc/host/elgamal_shape.h): the GPU witness synthesis (csrc/elgamal_witness.hip) lays its output out by these counts."""
import ctypes
import os
import subprocess

import pytest

import elgamal_model as E
from oracle_lib import golden
from simpleworks_amd import marlin as M, workloads as W
from simpleworks_amd._lib import load_library

R = W.R_MODULUS
L = W.ED_SUBGROUP_ORDER
SHAPE = (7, 5371, 5375)
OUT_ROWS = [5371, 5372, 5373, 5374]


@pytest.fixture(scope="module")
def G():
    return golden("elgamal.json")


@pytest.fixture(scope="module")
def generator(G):
    return E.point_from_bytes(bytes.fromhex(G["generator"]))


def _failing_rows(cs):
    """The row evaluator: every row a z * b z == c z in Python integers; returns the indices of the rows that fail."""
    z = {("i", k): v for k, v in enumerate(cs.instance)}
    z.update({("w", k): v for k, v in enumerate(cs.witness)})

    def ev(lc):
        return sum(c * z[v] for c, v in lc) % R
    return [i for i, (a, b, c) in enumerate(zip(*cs.rows)) if ev(a) * ev(b) % R != ev(c)]


def _point(hexstr):
    p = E.point_from_bytes(bytes.fromhex(hexstr))
    assert p is not None
    return p


def _coords(*hexes):
    out = []
    for h in hexes:
        b = bytes.fromhex(h)
        out += [int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little")]
    return out


def _subgroup_key(G):
    return _point(G["valid"][0]["public_key"])


def test_shape_builder_layout_library_and_native_program(G, generator, tmp_path):
    """Builder = elgamal_circuit_layout() = swm_elgamal_circuit_shape = (7, 5371, 5375); the densest matrix fits |K| = 2^13; the
    stand-alone program (tests/native/elgamal_shape_check.cpp), built with -fsanitize=address,undefined, holds the header to the
    layout's numbers."""
    v = G["valid"][0]
    cs, _ = W.elgamal_encryption_circuit(generator, _point(v["public_key"]), _point(v["message"]), bytes.fromhex(v["randomness"]))
    lay = W.elgamal_circuit_layout()
    assert (len(cs.instance), len(cs.witness), cs.num_constraints) == SHAPE
    assert (lay["num_instance"], lay["num_witness"], lay["num_constraints"]) == SHAPE
    assert M.elgamal_circuit_shape() == SHAPE
    assert lay["out"] == OUT_ROWS[0]
    nnz = [int(m[0][-1]) for m in cs.pack().mats]
    assert max(nnz) <= 8192, nnz
    null = ctypes.POINTER(ctypes.c_size_t)()
    n = ctypes.c_size_t(0)
    assert load_library().swm_elgamal_circuit_shape(null, ctypes.byref(n), ctypes.byref(n)) == -1

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "elgamal_shape_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(root, "simpleworks_amd", "csrc"), os.path.join(root, "tests", "native", "elgamal_shape_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and ("asan" in out.stderr.lower() or "ubsan" in out.stderr.lower()) and "error:" not in out.stderr:
        pytest.skip("this g++ has no ASan / UBSan runtime")
    assert out.returncode == 0, out.stderr[-4000:]
    names = ["key", "msg", "rnd", "fix", "dbl", "sel", "add", "sum", "out", "num_instance", "num_witness", "num_constraints"]
    run = subprocess.run([exe] + [str(lay[k]) for k in names], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split() == ["ok"] + [str(x) for x in SHAPE]
    wrong = [str(lay[k] + (k == "sel")) for k in names]
    run = subprocess.run([exe] + wrong, capture_output=True, text=True, timeout=300)
    assert run.returncode == 1 and "sel" in run.stderr


@pytest.mark.parametrize("index", [0, 1, 2])
def test_valid_fixtures_are_satisfied(G, generator, index):
    v = G["valid"][index]
    cs, public = W.elgamal_encryption_circuit(generator, _point(v["public_key"]), _point(v["message"]), bytes.fromhex(v["randomness"]))
    assert _failing_rows(cs) == []
    assert public == _coords(v["public_key"], v["c1"], v["c2"]) == cs.instance[1:]
    assert public == W.elgamal_public_inputs(bytes.fromhex(v["public_key"]), bytes.fromhex(v["c1"] + v["c2"]))


def test_edge_fixtures_are_satisfied(G, generator):
    """All 43: r = 0, the identity, keys and messages of order 2 and 4 or outside the prime subgroup, c2 = identity."""
    assert len(G["edge"]) == 43
    for e in G["edge"]:
        cs, public = W.elgamal_encryption_circuit(generator, _point(e["point"]), _point(e["message"]), bytes.fromhex(e["scalar"]))
        assert _failing_rows(cs) == [], e["note"]
        assert public == _coords(e["point"], e["c1"], e["c2"]), e["note"]


@pytest.mark.parametrize("r", [L, L + 5, (1 << 256) - 1])
def test_randomness_at_and_above_the_group_order(G, generator, r):
    """r enters unreduced: bits 251 .. 255 are rows like the others.  On a key of the prime subgroup the ciphertext is the
    model's with r mod l."""
    v = G["valid"][1]
    pk, m = _subgroup_key(G), _point(v["message"])
    assert W.ed_mul(pk, L) == (0, 1)
    cs, public = W.elgamal_encryption_circuit(generator, pk, m, r)
    assert _failing_rows(cs) == []
    lay = W.elgamal_circuit_layout()
    assert [cs.witness[lay["rnd"] + i] for i in range(256)] == [(r >> i) & 1 for i in range(256)]
    c1, c2 = E.encrypt(generator, pk, m, r % L)
    assert public[2:] == [c1[0], c1[1], c2[0], c2[1]]
    as_bytes, _ = W.elgamal_encryption_circuit(generator, pk, m, r.to_bytes(32, "little"))
    assert as_bytes.witness == cs.witness


def test_a_wrong_claim_fails_the_out_rows_only(G, generator):
    v, other = G["valid"][0], G["valid"][1]
    pk, m, r = _point(v["public_key"]), _point(v["message"]), bytes.fromhex(v["randomness"])
    honest, _ = W.elgamal_encryption_circuit(generator, pk, m, r)
    c1, c2 = _point(v["c1"]), _point(v["c2"])
    for k in range(4):
        claim = [c1[0], c1[1], c2[0], c2[1]]
        claim[k] = (claim[k] + 1) % R
        cs, public = W.elgamal_encryption_circuit(generator, pk, m, r, ((claim[0], claim[1]), (claim[2], claim[3])))
        assert _failing_rows(cs) == [OUT_ROWS[k]]
        assert cs.witness == honest.witness and public[2:] == claim
    cs, _ = W.elgamal_encryption_circuit(generator, pk, m, r, (_point(other["c1"]), _point(other["c2"])))
    assert _failing_rows(cs) == OUT_ROWS


def test_off_curve_inputs_raise(G, generator):
    v = G["valid"][0]
    pk, m = _point(v["public_key"]), _point(v["message"])
    for args in ((generator, pk, (m[0], m[1] ^ 1)), (generator, (pk[0] ^ 1, pk[1]), m), ((generator[0], generator[1] ^ 1), pk, m)):
        assert not all(W.ed_on_curve(p) for p in args)
        with pytest.raises(ValueError):
            W.elgamal_encryption_circuit(*args, 5)
    for r in (-1, 1 << 256, bytes(31)):
        with pytest.raises(ValueError):
            W.elgamal_encryption_circuit(generator, pk, m, r)


def test_the_synthesizer_class_gives_the_builders_system(G, generator):
    v = G["valid"][2]
    pk, m, r = _point(v["public_key"]), _point(v["message"]), bytes.fromhex(v["randomness"])
    cs, _ = W.elgamal_encryption_circuit(generator, pk, m, r)
    got = M.MarlinInst._synthesize(W.ElGamalEncryption(generator, pk, m, r))
    assert got.instance == cs.instance and got.witness == cs.witness and got.rows == cs.rows

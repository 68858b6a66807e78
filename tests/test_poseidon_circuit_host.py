"""CPU tests of the Poseidon hash circuit: its specification, workloads.build_poseidon_hash, evaluated row by row in Python integers
on the inputs of tests/golden/poseidon.json and on tampered assignments, its public outputs against the fixture's digests (which the
big-integer model tests/poseidon_model.py wrote), and its SHAPE as the library states it without a GPU
(swm_poseidon_circuit_shape, csrc/host/poseidon_shape.h): the GPU witness synthesis (csrc/poseidon_witness.hip) lays its output out
by these counts."""
import ctypes
import os
import shutil
import subprocess

import pytest

import poseidon_model as P
from oracle_lib import golden
from simpleworks_amd import hash as H, marlin as M, workloads as W
from simpleworks_amd._lib import load_library

R = W.R_MODULUS
PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")
LENGTHS = (0, 1, 11, 22, 23, 24, 54, 55, 85, 86, 117, 118, 300)   # 8 + n crosses a chunk at 23|24, 54|55 (also the rate), 85|86, 116|117
ALPHAS = (2, 3, 5, 17, 65535)
ROUND_SHAPES = ((8, 29), (8, 0), (2, 29), (2, 0))


def le(h):
    return int.from_bytes(bytes.fromhex(h), "little")


@pytest.fixture(scope="module")
def G():
    return golden("poseidon.json")


@pytest.fixture(scope="module")
def ref():
    return P.load_params(PARAMS)


@pytest.fixture(scope="module")
def params():
    return H.PoseidonParameters.from_json(PARAMS)


@pytest.fixture(scope="module")
def hello(params):
    cs, public = W.poseidon_hash_circuit(params, data=b"Hello World")
    return cs, public


def _failing_rows(cs, instance=None, witness=None):
    """The row evaluator: every row a z * b z == c z in Python integers; returns the indices of the rows that fail."""
    z = {("i", k): v for k, v in enumerate(cs.instance if instance is None else instance)}
    z.update({("w", k): v for k, v in enumerate(cs.witness if witness is None else witness)})

    def ev(lc):
        return sum(c * z[v] for c, v in lc) % R
    return [i for i, (a, b, c) in enumerate(zip(*cs.rows)) if ev(a) * ev(b) % R != ev(c)]


def _shape(full, partial, alpha, bytes_form, n_in, n_out):
    lib = load_library()
    ni, nw, nc = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = lib.swm_poseidon_circuit_shape(full, partial, alpha, 1 if bytes_form else 0, n_in, n_out, ctypes.byref(ni), ctypes.byref(nw),
                                        ctypes.byref(nc))
    return rc, (ni.value, nw.value, nc.value)


def _counts(cs):
    return len(cs.instance), len(cs.witness), cs.num_constraints


def _layout_counts(lay):
    return lay["num_instance"], lay["num_witness"], lay["num_constraints"]


@pytest.mark.parametrize("length", LENGTHS)
def test_bytes_form_shape_rows_and_digest(G, ref, params, length):
    """The library's three counts are the builder's, every row holds, and the public digest is the fixture's (the model's where the
    fixture has no such length)."""
    have = G["bytes"].get(str(length), [])
    for i in range(1 if length == 0 else 2):
        data = P.poseidon_input(length, i)
        cs, public = W.poseidon_hash_circuit(params, data=data)
        rc, got = _shape(8, 29, 17, True, length, 1)
        assert rc == 0
        assert got == _counts(cs) == M.poseidon_circuit_shape(params, input_len=length)
        lay = W.poseidon_circuit_layout(params, input_len=length)
        assert got == _layout_counts(lay) and lay["bits"] == 0 and lay["sponge"] == 8 * length
        assert lay["permutations"] * lay["sboxes"] * lay["chain"] == len(cs.witness) - 8 * length
        assert _failing_rows(cs) == []
        assert cs.witness[:8 * length] == [(byte >> k) & 1 for byte in data for k in range(8)]
        want = le(have[i]) if i < len(have) else P.hash_bytes(ref, data)
        assert public == cs.instance[1:] == [want]
        assert want == P.hash_bytes(ref, data)


def test_the_counts_the_issue_states(params):
    assert M.poseidon_circuit_shape(params, input_len=0) == (2, 265, 266)
    assert M.poseidon_circuit_shape(params, input_len=11) == (2, 353, 354)
    assert M.poseidon_circuit_shape(params, input_len=55) == (2, 970, 971)
    assert M.poseidon_circuit_shape(params, input_len=65536) == (2, 8 * 65536 + 1058 * 265, 8 * 65536 + 1058 * 265 + 1)
    assert 8 * 65536 + 1058 * 265 == 804658
    lay = W.poseidon_circuit_layout(params, input_len=65536)
    assert (lay["permutations"], lay["sboxes"], lay["chain"]) == (1058, 53, 5)


@pytest.mark.parametrize("n_out", [1, 2, 3, 16])
def test_elements_form_shape_rows_and_outputs(G, ref, params, n_out):
    for n_in in range(6):
        cases = [c for c in G["elements"] if len(c["in"]) == n_in]
        assert cases
        rc, got = _shape(8, 29, 17, False, n_in, n_out)
        lay = W.poseidon_circuit_layout(params, n_in=n_in, n_out=n_out)
        assert rc == 0 and got == _layout_counts(lay) == M.poseidon_circuit_shape(params, n_in=n_in, n_out=n_out)
        assert lay["elements"] == 0 and lay["sponge"] == n_in
        for c in cases if n_out <= 3 else cases[:1]:
            elems = [le(h) for h in c["in"]]
            cs, public = W.poseidon_hash_circuit(params, elements=elems, n_out=n_out)
            assert _counts(cs) == got
            assert cs.witness[:n_in] == elems
            assert _failing_rows(cs) == []
            want = [le(h) for h in c["out"][:n_out]] if n_out <= len(c["out"]) else P.hash_elements(ref, elems, n_out)
            assert public == cs.instance[1:] == want


def test_alpha_and_round_shapes(G, ref):
    """The fixture's adversarial parameter sets: alpha 2 .. 65535, with and without partial rounds, two and eight full rounds; fills
    r - 1, identity and the reference's.  Shapes from the library, rows and outputs from the builder."""
    items = [[le(h) for h in item] for item in G["adversarial_items"]]
    seen = set()
    for case in G["adversarial"]:
        full, partial, alpha = case["full_rounds"], case["partial_rounds"], case["alpha"]
        model = P.adversarial_params(case["fill"], full, partial, alpha, ref)
        p = H.PoseidonParameters(*model)
        seen.add((full, partial, alpha))
        item, want = items[0], case["out"][0]
        cs, public = W.poseidon_hash_circuit(p, elements=item, n_out=3)
        rc, got = _shape(full, partial, alpha, False, len(item), 3)
        assert rc == 0 and got == _counts(cs), (case["fill"], full, partial, alpha)
        m = alpha.bit_length() - 1 + bin(alpha).count("1") - 1
        assert W.poseidon_circuit_layout(p, n_in=len(item), n_out=3)["chain"] == m
        assert public == [le(h) for h in want]
        assert _failing_rows(cs) == []
    assert {(f, pr, a) for f, pr in ROUND_SHAPES for a in ALPHAS} <= seen
    for full, partial in ROUND_SHAPES:
        for alpha in ALPHAS:
            p = H.PoseidonParameters(full, partial, alpha, ref[3], ref[4][:full + partial])
            for kw in ({"input_len": 11}, {"input_len": 55}, {"n_in": 5, "n_out": 16}):
                lay = W.poseidon_circuit_layout(p, **kw)
                bytes_form = "input_len" in kw
                rc, got = _shape(full, partial, alpha, bytes_form, kw.get("input_len", kw.get("n_in")), kw.get("n_out", 1))
                assert rc == 0 and got == _layout_counts(lay), (full, partial, alpha, kw)
    assert W.poseidon_circuit_layout(H.PoseidonParameters(2, 0, 65535, ref[3], ref[4][:2]), n_in=1)["chain"] == 30   # 15 squares, 15 products


def test_shape_refusals(params):
    lib = load_library()
    n = ctypes.c_size_t(0)
    refused = [(8, 29, 17, True, 65537, 1), (8, 29, 17, False, 4097, 1), (8, 29, 17, False, 1, 0), (8, 29, 17, False, 1, 17),
               (8, 29, 17, True, 11, 2), (8, 29, 17, True, 11, 0), (7, 29, 17, True, 11, 1), (0, 29, 17, True, 11, 1),
               (8, 248, 17, True, 11, 1), (8, 29, 1, True, 11, 1), (8, 29, 65536, True, 11, 1), (8, 29, 17, True, 1 << 62, 1),
               (1 << 63, 29, 17, False, 1, 1), (8, (1 << 64) - 8, 17, False, 1, 1)]
    for args in refused:
        assert _shape(*args)[0] == -1, args
    assert lib.swm_last_error(None).decode().startswith("poseidon_circuit_shape")
    assert _shape(8, 29, 17, True, 65536, 1)[0] == 0 and _shape(8, 29, 17, False, 4096, 16)[0] == 0
    assert _shape(8, 247, 65535, False, 4096, 16) == (0, (17, 4096 + 2055 * (24 + 247) * 30, 2055 * (24 + 247) * 30 + 16))
    assert lib.swm_poseidon_circuit_shape(8, 29, 17, 1, 5, 1, None, ctypes.byref(n), ctypes.byref(n)) == -1
    assert lib.swm_poseidon_circuit_shape(8, 29, 17, 1, 5, 1, ctypes.byref(n), None, ctypes.byref(n)) == -1
    assert lib.swm_poseidon_circuit_shape(8, 29, 17, 1, 5, 1, ctypes.byref(n), ctypes.byref(n), None) == -1
    with pytest.raises(M.MarlinError) as e:
        M.poseidon_circuit_shape(params, input_len=65537)
    assert e.value.code == -1
    for kw in ({"input_len": 65537}, {"n_in": 4097}, {"n_in": 1, "n_out": 0}, {"n_in": 1, "n_out": 17}, {"input_len": 3, "n_out": 2}, {}):
        with pytest.raises(ValueError):
            W.poseidon_circuit_layout(params, **kw)
    with pytest.raises(ValueError):
        W.build_poseidon_hash(M.ConstraintSystem(), params, elements=[R])
    with pytest.raises(ValueError):
        W.build_poseidon_hash(M.ConstraintSystem(), params, data=b"x", elements=[1])
    with pytest.raises(ValueError):
        W.build_poseidon_hash(M.ConstraintSystem(), params, data=b"xy", n_out=2)


def test_a_flipped_input_bit_reaches_the_output_row(params, hello):
    """The honest witness of another input against the published digest: the output row fails.  The same bit flipped in place,
    nothing recomputed: the rows that read the first absorbed element fail (x x = x^2 and x^16 x = x^17 of the first S-box)."""
    cs, public = hello
    assert _failing_rows(cs) == []
    other, other_public = W.poseidon_hash_circuit(params, data=b"Hello Wnrld")     # 'o' ^ 1
    assert other.rows == cs.rows and other_public != public
    assert [k for k in range(len(cs.witness)) if k < 88 and other.witness[k] != cs.witness[k]] == [8 * 7]
    bad = _failing_rows(cs, witness=other.witness)
    assert bad and cs.num_constraints - 1 in bad
    witness = list(cs.witness)
    witness[8 * 7] ^= 1
    bad = _failing_rows(cs, witness=witness)
    assert bad == [88, 92]


def test_a_bit_of_two_fails_its_booleanity_row(params, hello):
    cs, _ = hello
    witness = list(cs.witness)
    witness[17] = 2
    bad = _failing_rows(cs, witness=witness)
    assert [i for i in bad if i < 88] == [17]


def test_a_changed_chain_value_fails_its_row_and_the_next(params, hello):
    """x^2 of the first S-box: its own row (x x = x^2) and the row of x^4 = x^2 x^2; then one in a partial round."""
    cs, _ = hello
    lay = W.poseidon_circuit_layout(params, input_len=11)
    for at in (lay["sponge"], lay["sponge"] + (4 * 3 + 7) * lay["chain"] + 2):
        witness = list(cs.witness)
        witness[at] = (witness[at] + 1) % R
        assert _failing_rows(cs, witness=witness) == [at, at + 1]   # row of witness k is row k: bit rows first, then chain rows


def test_another_public_digest_fails_the_output_row_only(params, hello):
    cs, public = hello
    assert _failing_rows(cs, instance=[1, (public[0] + 1) % R]) == [cs.num_constraints - 1]


def test_synthesizer_class(params, hello):
    cs, public = hello
    again = M.MarlinInst._synthesize(W.PoseidonHashCircuit(params, data=b"Hello World"))
    assert again.witness == cs.witness and again.rows == cs.rows and again.instance == [1] + public
    el = M.MarlinInst._synthesize(W.PoseidonHashCircuit(params, elements=[5, 6, 7], n_out=2))
    assert el.witness[:3] == [5, 6, 7] and len(el.instance) == 3


def test_ffi_declares_the_six_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ffi = open(os.path.join(root, "swmarlin-sys", "src", "ffi.rs")).read()
    hdr = open(os.path.join(root, "include", "swmarlin.h")).read()
    for name in ("swm_poseidon_circuit_shape", "swm_poseidon_circuit_create", "swm_poseidon_circuit_destroy", "swm_poseidon_witness",
                 "swm_poseidon_witness_dev", "swm_poseidon_prove"):
        assert "pub fn %s(" % name in ffi and "%s(" % name in hdr
        assert hasattr(load_library(), name)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shape_under_asan_ubsan(tmp_path):
    """csrc/host/poseidon_shape.h — the counts and offsets the kernel writes witnesses by — against a brute-force walk of the sponge
    schedule, in a stand-alone program (tests/native/poseidon_shape_check.cpp) built with -fsanitize=address,undefined."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "poseidon_shape_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(root, "simpleworks_amd", "csrc"), os.path.join(root, "tests", "native", "poseidon_shape_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and ("asan" in out.stderr.lower() or "ubsan" in out.stderr.lower()) and "error:" not in out.stderr:
        pytest.skip("this g++ has no ASan / UBSan runtime")
    assert out.returncode == 0, out.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) >= 401 + 65 * 16 + 20

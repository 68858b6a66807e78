"""CPU tests of the rollup circuit: ONE statement for a block of transfers.  The specification workloads.build_rollup /
build_pedersen_rollup evaluated row by row in Python integers on dependent chains (tests/transfer_model.py,
tests/pedersen_transfer_model.py) — the honest chain, a wrong linking root, a wrong public new_root, two transfers swapped in the
instance, a refused transfer —, workloads.rollup_system (the same matrices by relabelling one transfer system) against the builder
entry for entry, and the SHAPE as the library states it without a GPU (swm_rollup_circuit_shape, swm_pedersen_rollup_circuit_shape,
csrc/host/rollup_shape.h): the GPU driver (csrc/rollup_witness.hip) lays the block out by these counts and offsets."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import pedersen_transfer_model as PTM
import poseidon_model as P
import transfer_model as TM
from simpleworks_amd import hash as H, marlin as M, workloads as W
from simpleworks_amd._lib import load_library

R = W.R_MODULUS
PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")
KEYS = ("message", "signature", "sender_leaf", "sender_path", "recipient_leaf", "recipient_path")
# height 2 holds the ids 0 (50) and 1 (1000): every transfer spends what the one before it credited
CHAIN = [("zero to one", 0, 1, 50, None), ("one back, with the credit", 1, 0, 1030, None), ("zero spends it", 0, 1, 1000, None)]
# the middle one is overdrawn by one (1 holds 1050); the last one is valid against the state the FIRST one left
REFUSED = [CHAIN[0], ("overdrawn in the middle", 1, 0, 1051, "overdraft"), ("one to zero", 1, 0, 5, None)]


@pytest.fixture(scope="module")
def ref():
    return P.load_params(PARAMS)


@pytest.fixture(scope="module")
def params():
    return H.PoseidonParameters.from_json(PARAMS)


@pytest.fixture(scope="module")
def merkle():
    return W.MerkleParams()


def _failing_rows(cs, instance=None, witness=None):
    """The row evaluator: every row a z * b z == c z in Python integers; returns the indices of the rows that fail."""
    z = {("i", k): v for k, v in enumerate(cs.instance if instance is None else instance)}
    z.update({("w", k): v for k, v in enumerate(cs.witness if witness is None else witness)})

    def ev(lc):
        return sum(c * z[v] for c, v in lc) % R
    return [i for i, (a, b, c) in enumerate(zip(*cs.rows)) if ev(a) * ev(b) % R != ev(c)]


def _same_matrices(a, b):
    a, b = a.pack(), b.pack()
    assert a.instance.shape == b.instance.shape and a.witness.shape == b.witness.shape and a.num_constraints == b.num_constraints
    for (rp, col, val), (rp2, col2, val2) in zip(a.mats, b.mats):
        assert np.array_equal(rp, rp2) and np.array_equal(col, col2) and np.array_equal(val, val2)
    return True


@pytest.fixture(scope="module")
def chain(ref, params):
    """The honest chain at height 2, N = 3, built once: (transfers, cs, public, layout)."""
    block = TM.transfers(ref, 2, which=CHAIN)[1]
    assert [t["applied"] for t in block] == [True] * 3 and all(a["public"][1] == b["public"][0] for a, b in zip(block, block[1:]))
    cs, public = W.rollup_circuit(params, 2, block)
    return block, cs, public, W.rollup_circuit_layout(params, 2, 3)


def _shape(full, partial, alpha, height, salted, n):
    ni, nw, nc = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = load_library().swm_rollup_circuit_shape(full, partial, alpha, height, salted, n, ctypes.byref(ni), ctypes.byref(nw), ctypes.byref(nc))
    return rc, (ni.value, nw.value, nc.value)


def _pedersen_shape(height, salted, n):
    ni, nw, nc = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = load_library().swm_pedersen_rollup_circuit_shape(height, salted, n, ctypes.byref(ni), ctypes.byref(nw), ctypes.byref(nc))
    return rc, (ni.value, nw.value, nc.value)


def _counts(cs):
    if hasattr(cs, "rows"):
        return len(cs.instance), len(cs.witness), cs.num_constraints
    return cs.instance.shape[0], cs.witness.shape[0], cs.num_constraints


@pytest.mark.parametrize("height", [2, 4])
def test_shape_calls_equal_the_builders_counts(ref, params, height):
    """build_rollup's own counts for N = 1, 2, 3, 8 (one valid transfer in every section: the counts do not depend on the values)."""
    t = next(t for t in TM.transfers(ref, height)[1] if t["name"] == "zero to one")
    for n in (1, 2, 3, 8):
        cs, public = W.rollup_circuit(params, height, [t] * n)
        got = _counts(cs)
        lay = W.rollup_circuit_layout(params, height, n)
        w, r = M.transfer_circuit_shape(params, height)[1:]
        assert got == (3 + 3 * n, n * (w + 1) - 1, n * r) == (lay["num_instance"], lay["num_witness"], lay["num_constraints"])
        assert _shape(8, 29, 17, height, 0, n) == (0, got) and M.rollup_circuit_shape(params, height, n) == got
        assert len(public) == 2 + 3 * n and cs.instance == [1] + public


def test_shape_calls_at_height_9_equal_the_relabelled_systems_counts(ref, params):
    t = next(t for t in TM.transfers(ref, 9)[1] if t["name"] == "meet at level 0")
    one, _ = W.transfer_circuit(params, 9, *[t[k] for k in KEYS])
    packed = one.pack()
    for n in (1, 2, 3, 8):
        got = _counts(W.rollup_system(packed, n))
        assert _shape(8, 29, 17, 9, 0, n) == (0, got) and M.rollup_circuit_shape(params, 9, n) == got
    assert got == (27, 660631, 668552) and got[0] + got[1] == 660658       # the worked numbers: |H| = 2^20
    assert max(got[1] + 27, got[2]) <= 1 << 20 < 13 * 83569


def test_pedersen_shape_calls(merkle):
    for height in (2, 4, 9):
        for salted in (False, True):
            w, r = M.pedersen_transfer_circuit_shape(height, salted)[1:]
            for n in (1, 2, 3, 8):
                want = (3 + 3 * n, n * (w + 1) - 1, n * r)
                lay = W.pedersen_rollup_circuit_layout(height, n, salted)
                assert _pedersen_shape(height, 1 if salted else 0, n) == (0, want) and M.pedersen_rollup_circuit_shape(height, n, salted) == want
                assert (lay["num_instance"], lay["num_witness"], lay["num_constraints"]) == want
    assert M.pedersen_rollup_circuit_shape(9, 5)[2] <= 1 << 20 < M.pedersen_rollup_circuit_shape(9, 6)[2]      # five fit |H| = 2^20


def test_block_sizes_outside_1_to_64_are_refused(ref, params, merkle, chain):
    block = chain[0]
    one, _ = W.transfer_circuit(params, 2, *[block[0][k] for k in KEYS])
    for n in (0, 65, 1 << 40):
        assert _shape(8, 29, 17, 4, 0, n)[0] == -1 and _pedersen_shape(4, 0, n)[0] == -1
        with pytest.raises(M.MarlinError) as e:
            M.rollup_circuit_shape(params, 4, n)
        assert e.value.code == -1
        with pytest.raises(M.MarlinError):
            M.pedersen_rollup_circuit_shape(4, n)
        with pytest.raises(ValueError):
            W.rollup_system(one, n)
        with pytest.raises(ValueError):
            W.rollup_circuit_layout(params, 4, n)
        with pytest.raises(ValueError):
            W.pedersen_rollup_circuit_layout(4, n)
    assert load_library().swm_last_error(None).decode().startswith("pedersen_rollup_circuit_shape")
    assert _shape(8, 29, 17, 4, 0, 64)[0] == 0 and _pedersen_shape(4, 0, 64)[0] == 0 and _shape(8, 29, 17, 10, 0, 2)[0] == -1
    assert _shape(7, 29, 17, 4, 0, 2)[0] == -1 and _pedersen_shape(1, 0, 2)[0] == -1
    for cs_args in ([], [block[0]] * 65):
        with pytest.raises(ValueError):
            W.rollup_circuit(params, 2, cs_args)
        with pytest.raises(ValueError):
            W.pedersen_rollup_circuit(merkle, 2, cs_args)
    with pytest.raises(ValueError):
        W.rollup_circuit(params, 2, block, roots={3: 0})       # root_3 of three transfers is the public new_root
    lib, n = load_library(), ctypes.c_size_t(0)
    assert lib.swm_rollup_circuit_shape(8, 29, 17, 4, 0, 2, None, ctypes.byref(n), ctypes.byref(n)) == -1
    assert lib.swm_rollup_circuit_shape(8, 29, 17, 4, 0, 2, ctypes.byref(n), ctypes.byref(n), None) == -1
    assert lib.swm_pedersen_rollup_circuit_shape(4, 0, 2, ctypes.byref(n), None, ctypes.byref(n)) == -1


def test_the_relabelled_system_is_the_builders_entry_for_entry(ref, params, chain):
    """rollup_system over ONE transfer system (any transfer's: the matrices depend on the shape alone) against build_rollup's packed
    matrices at height 2 for N = 1, 2, 3."""
    block, cs3, _, _ = chain
    other = TM.transfers(ref, 2)[1][-1]        # not a transfer of the chain
    one, _ = W.transfer_circuit(params, 2, *[other[k] for k in KEYS])
    packed = one.pack()
    assert _same_matrices(W.rollup_system(packed, 3), cs3)
    for n in (1, 2):
        cs, _ = W.rollup_circuit(params, 2, block[:n])
        assert _same_matrices(W.rollup_system(packed, n), cs)
    assert _same_matrices(W.rollup_system(packed, 1), one)


def test_one_transfer_is_the_transfer_circuit_verbatim(ref, params, chain):
    t = chain[0][0]
    cs, public = W.rollup_circuit(params, 2, [t])
    one, one_public = W.transfer_circuit(params, 2, *[t[k] for k in KEYS])
    assert cs.rows == one.rows and cs.witness == one.witness and cs.instance == one.instance and public == one_public == t["public"]


def test_rows_of_the_honest_chain_and_of_what_can_be_wrong_with_it(params, chain):
    block, cs, public, lay = chain
    tlay = lay["transfer"]
    w, r = tlay["num_witness"], tlay["num_constraints"]
    assert public == W.rollup_public_inputs(block[0]["public"][0], block[2]["public"][1], [t["message"] for t in block])
    assert cs.instance == [1] + public and public[2:] == [v for t in block for v in t["public"][2:]]
    assert lay["stride"] == w + 1 and lay["sections"] == [0, w + 1, 2 * w + 2] and lay["roots"] == {1: w, 2: 2 * w + 1}
    assert lay["section_rows"] == [0, r, 2 * r] and lay["new_root_row"][2] == cs.num_constraints - 1 == 3 * r - 1
    # the linking roots are the roots the model's block went through, and every section is the transfer's own witness
    assert [cs.witness[lay["roots"][k]] for k in (1, 2)] == [block[0]["public"][1], block[1]["public"][1]]
    for k, t in enumerate(block):
        one, _ = W.transfer_circuit(params, 2, *[t[key] for key in KEYS])
        assert cs.witness[lay["sections"][k]:lay["sections"][k] + w] == one.witness
    assert _failing_rows(cs) == []
    # a wrong root_1: exactly section 0's last row and section 1's sender root row
    wit = list(cs.witness)
    wit[lay["roots"][1]] = (wit[lay["roots"][1]] + 1) % R
    assert _failing_rows(cs, witness=wit) == [lay["new_root_row"][0], lay["sender_root_row"][1]]
    assert lay["new_root_row"][0] == r - 1 and lay["sender_root_row"][1] == r + tlay["sender_root_row"]
    # a wrong public new_root: the last row only; a wrong public old_root: section 0's sender root row only
    inst = list(cs.instance)
    inst[2] = (inst[2] + 1) % R
    assert _failing_rows(cs, instance=inst) == [3 * r - 1]
    inst = list(cs.instance)
    inst[1] = (inst[1] + 1) % R
    assert _failing_rows(cs, instance=inst) == [lay["sender_root_row"][0]]
    # transfers 0 and 1 swapped in the instance: tie rows only, of those two sections
    inst = list(cs.instance)
    inst[3:6], inst[6:9] = inst[6:9], inst[3:6]
    failing = _failing_rows(cs, instance=inst)
    ties = {lay["tie_rows"][k] + j for k in (0, 1) for j in range(3)}
    assert failing and set(failing) <= ties and {lay["tie_rows"][0] + 2, lay["tie_rows"][1] + 2} <= set(failing)      # the amounts differ


def test_a_refused_middle_transfer_fails_rows_of_its_own_section_only(ref, params):
    block = TM.transfers(ref, 2, which=REFUSED)[1]
    assert [t["applied"] for t in block] == [True, False, True] and block[1]["flag"] == 15 - 2
    lay = W.rollup_circuit_layout(params, 2, 3)
    r = lay["transfer"]["num_constraints"]
    # the roots the library's pass publishes: a refused transfer leaves the root where it was
    cs, public = W.rollup_circuit(params, 2, block, roots={2: block[1]["public"][1]})
    assert block[1]["public"][0] == block[1]["public"][1] == cs.witness[lay["roots"][1]] == cs.witness[lay["roots"][2]]
    failing = _failing_rows(cs)
    assert lay["pack_row"][1] in failing and all(r <= i < 2 * r for i in failing)
    assert set(failing) == {lay["pack_row"][1], lay["new_root_row"][1]}
    # with the root it walks to instead, the section fails its overdraft row alone and the NEXT section's root row breaks the chain
    cs, _ = W.rollup_circuit(params, 2, block)
    assert _failing_rows(cs) == [lay["pack_row"][1], lay["sender_root_row"][2]]


def test_the_pedersen_chain(merkle):
    """The same chain checks over the Pedersen tree at height 2, N = 2."""
    block = PTM.transfers(merkle, 2, which=CHAIN[:2])[1]
    assert [t["applied"] for t in block] == [True, True]
    cs, public = W.pedersen_rollup_circuit(merkle, 2, block)
    lay = W.pedersen_rollup_circuit_layout(2, 2)
    w, r = M.pedersen_transfer_circuit_shape(2)[1:]
    assert _counts(cs) == (9, 2 * w + 1, 2 * r) == M.pedersen_rollup_circuit_shape(2, 2)
    assert public == W.rollup_public_inputs(block[0]["public"][0], block[1]["public"][1], [t["message"] for t in block])
    assert cs.witness[lay["roots"][1]] == block[0]["public"][1] and lay["roots"] == {1: w}
    one, _ = PTM.build(merkle, 2, block[1])
    assert cs.witness[w + 1:] == one.witness
    assert _same_matrices(W.rollup_system(one, 2), cs)
    assert _failing_rows(cs) == []
    wit = list(cs.witness)
    wit[w] = (wit[w] + 1) % R
    assert _failing_rows(cs, witness=wit) == [lay["new_root_row"][0], lay["sender_root_row"][1]] == [r - 1, r + lay["transfer"]["sender_root_row"]]
    inst = list(cs.instance)
    inst[2] = (inst[2] + 1) % R
    assert _failing_rows(cs, instance=inst) == [2 * r - 1]
    inst = list(cs.instance)
    inst[3:6], inst[6:9] = inst[6:9], inst[3:6]
    failing = _failing_rows(cs, instance=inst)
    assert failing and set(failing) <= {lay["tie_rows"][k] + j for k in (0, 1) for j in range(3)}
    # a refused first transfer (overdrawn by one) fails rows of section 0 only
    bad = PTM.transfers(merkle, 2, which=[("overdrawn", 0, 1, 51, "overdraft"), ("one to zero", 1, 0, 5, None)])[1]
    assert [t["applied"] for t in bad] == [False, True]
    cs, _ = W.pedersen_rollup_circuit(merkle, 2, bad, roots={1: bad[0]["public"][1]})
    assert set(_failing_rows(cs)) == {lay["pack_row"][0], lay["new_root_row"][0]}
    # N = 1 is the Pedersen transfer circuit verbatim
    cs1, _ = W.pedersen_rollup_circuit(merkle, 2, block[:1])
    one, _ = PTM.build(merkle, 2, block[0])
    assert cs1.rows == one.rows and cs1.witness == one.witness and cs1.instance == one.instance


def test_ffi_and_header_declare_the_new_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ffi = open(os.path.join(root, "swmarlin-sys", "src", "ffi.rs")).read()
    hdr = open(os.path.join(root, "include", "swmarlin.h")).read()
    for name in ("swm_rollup_circuit_shape", "swm_pedersen_rollup_circuit_shape", "swm_rollup_witness_at", "swm_pedersen_rollup_witness_at",
                 "swm_rollup_prove_at", "swm_pedersen_rollup_prove_at"):
        assert "pub fn %s(" % name in ffi and "int %s(" % name in hdr
        assert hasattr(load_library(), name)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shape_under_asan_ubsan(tmp_path):
    """csrc/host/rollup_shape.h — the counts and offsets the driver lays a block out by — over both trees' transfer shapes, a cover of
    the witnesses, rows and instance by sections and roots, the limits on N and the overflow checks, in a stand-alone program
    (tests/native/rollup_shape_check.cpp) built with -fsanitize=address,undefined."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "rollup_shape_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(root, "simpleworks_amd", "csrc"), os.path.join(root, "tests", "native", "rollup_shape_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and ("asan" in out.stderr.lower() or "ubsan" in out.stderr.lower()) and "error:" not in out.stderr:
        pytest.skip("this g++ has no ASan / UBSan runtime")
    assert out.returncode == 0, out.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) >= 2 * 2 * 8 * 8 + 16

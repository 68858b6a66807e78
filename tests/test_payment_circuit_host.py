"""CPU tests of the payment circuit: the model of a small ledger and its payments (tests/payment_model.py) against its fixture,
the circuit's specification workloads.build_payment evaluated row by row in Python integers on every payment of the fixture —
honest ones, an overdraft, a flipped signature, a recipient without an account, tampered public inputs — and its SHAPE as the
library states it without a GPU (swm_payment_circuit_shape, csrc/host/payment_shape.h): the GPU witness synthesis
(csrc/payment_witness.hip) lays its output out by these counts and offsets."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import payment_model as PM
import poseidon_model as P
import poseidon_tree_model as T
import schnorr_model as S
from oracle_lib import golden
from simpleworks_amd import hash as H, marlin as M, workloads as W
from simpleworks_amd._lib import load_library

R = W.R_MODULUS
PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")
SALT = bytes(range(32))
C = 265     # chain values per permutation of the reference's parameters: (3 * 8 + 29) * 5


def le(h):
    return int.from_bytes(bytes.fromhex(h), "little")


@pytest.fixture(scope="module")
def G():
    return golden("payment.json")


@pytest.fixture(scope="module")
def ref():
    return P.load_params(PARAMS)


@pytest.fixture(scope="module")
def params():
    return H.PoseidonParameters.from_json(PARAMS)


def _failing_rows(cs, instance=None, witness=None):
    """The row evaluator: every row a z * b z == c z in Python integers; returns the indices of the rows that fail."""
    z = {("i", k): v for k, v in enumerate(cs.instance if instance is None else instance)}
    z.update({("w", k): v for k, v in enumerate(cs.witness if witness is None else witness)})

    def ev(lc):
        return sum(c * z[v] for c, v in lc) % R
    return [i for i, (a, b, c) in enumerate(zip(*cs.rows)) if ev(a) * ev(b) % R != ev(c)]


def _build(params, height, g, salt=None):
    return W.payment_circuit(params, height, bytes.fromhex(g["message"]), bytes.fromhex(g["signature"]), bytes.fromhex(g["sender_leaf"]),
                             [le(h) for h in g["sender_path"]], bytes.fromhex(g["recipient_leaf"]), [le(h) for h in g["recipient_path"]],
                             salt=salt)


@pytest.fixture(scope="module")
def systems(G, params):
    """name -> (the builder's system, its public inputs, the rows that fail), each built and evaluated once."""
    seen = {}

    def get(name):
        if name not in seen:
            g = next(g for g in G["payments"] if g["name"] == name)
            cs, public = _build(params, G["height"], g)
            seen[name] = (cs, public, _failing_rows(cs))
        return seen[name]
    return get


def test_model_against_fixture(G, ref):
    leaves, levels = PM.ledger(ref, G["height"])
    assert {str(i): leaf.hex() for i, leaf in leaves.items()} == G["accounts"] and levels[-1][0] == le(G["root"])
    assert levels[0][0] == 0 and levels[0][PM.BLANK_ID] == 0       # blank leaves: digest zero
    payments = PM.payments(ref, G["height"])
    assert [p["name"] for p in payments] == [g["name"] for g in G["payments"]] == [p[0] for p in PM.PAYMENTS]
    for p, g in zip(payments, G["payments"]):
        for k in ("message", "signature", "sender_leaf", "recipient_leaf"):
            assert p[k].hex() == g[k], (p["name"], k)
        assert p["sender_path"] == [le(h) for h in g["sender_path"]] and p["recipient_path"] == [le(h) for h in g["recipient_path"]]
        assert p["public"] == [le(g["public"][0])] + g["public"][1:] and p["flag"] == g["flag"] and p["wrong"] == g["wrong"]
        # the flag byte is the two native checks; both paths lead to the root unless the recipient's leaf is blank
        msg, sender_leaf = p["message"], p["sender_leaf"]
        assert bool(g["flag"] & 1) == S.verify(S.GENERATOR, None, sender_leaf[:64], msg, p["signature"]) == (p["wrong"] != "signature")
        assert bool(g["flag"] & 2) == (int.from_bytes(msg[2:], "little") <= int.from_bytes(sender_leaf[64:], "little")) == (p["wrong"] != "overdraft")
        assert T.verify(ref, levels[-1][0], sender_leaf, msg[0], p["sender_path"])
        assert T.verify(ref, levels[-1][0], p["recipient_leaf"], msg[1], p["recipient_path"]) == (p["wrong"] != "recipient")
    amounts = {g["name"]: g["public"][3] for g in G["payments"]}
    assert amounts["amount zero"] == 0 and amounts["whole balance"] == PM.BALANCES[2] and amounts["overdraft by 1"] == PM.BALANCES[2] + 1
    assert PM.BALANCES[3] == (1 << 64) - 1


@pytest.mark.parametrize("name", [p[0] for p in PM.PAYMENTS])
def test_rows_of_every_payment(G, params, systems, name):
    """Honest payments: no failing row.  An overdraft: exactly the packing row.  A flipped signature: comparison rows of the Schnorr
    block only.  A recipient without an account: the recipient's root row only."""
    g = next(g for g in G["payments"] if g["name"] == name)
    cs, public, failing = systems(name)
    lay = W.payment_circuit_layout(params, G["height"])
    assert public == [le(g["public"][0])] + g["public"][1:] and cs.instance == [1] + public
    assert (len(cs.instance), len(cs.witness), cs.num_constraints) == (lay["num_instance"], lay["num_witness"], lay["num_constraints"])
    s_rows = lay["schnorr"]["num_constraints"]
    if g["wrong"] is None:
        assert failing == []
    elif g["wrong"] == "overdraft":
        assert failing == [lay["pack_row"]]
    elif g["wrong"] == "signature":
        assert failing and set(failing) <= set(range(s_rows - 8, s_rows))
    else:
        assert failing == [lay["recipient_root_row"]] == [cs.num_constraints - 1]
    # the witness groups sit where the layout says
    w = cs.witness
    balance, amount = int.from_bytes(bytes.fromhex(g["sender_leaf"])[64:], "little"), g["public"][3]
    assert w[lay["balance"]:lay["diff"]] == [(balance >> i) & 1 for i in range(64)]
    assert w[lay["diff"]:lay["sender"]] == [(((balance - amount) % (1 << 64)) >> i) & 1 for i in range(64)]
    leaf_bits = lambda leaf: [(byte >> i) & 1 for byte in leaf for i in range(8)]
    assert w[lay["recipient_bits"]:lay["recipient"]] == leaf_bits(bytes.fromhex(g["recipient_leaf"]))
    dec = lay["schnorr"]["dec"]
    assert w[dec:dec + 512] + w[lay["balance"]:lay["diff"]] == leaf_bits(bytes.fromhex(g["sender_leaf"]))
    mb, levels = lay["membership"], lay["levels"]
    for base, idx, path in ((lay["sender"], g["public"][1], g["sender_path"]), (lay["recipient"], g["public"][2], g["recipient_path"])):
        assert w[base + mb["bits"]:base + mb["bits"] + levels] == [(idx >> l) & 1 for l in range(levels)]
        assert w[base + mb["siblings"]:base + mb["siblings"] + levels] == [le(h) for h in path]


def test_the_membership_blocks_are_the_membership_circuits(G, params, systems):
    """Witness section for witness section: what build_poseidon_membership allocates for the same leaf, index and path."""
    g = G["payments"][0]
    cs, _, _ = systems(g["name"])
    lay = W.payment_circuit_layout(params, G["height"])
    for base, leaf, idx, path in ((lay["sender"], g["sender_leaf"], g["public"][1], g["sender_path"]),
                                  (lay["recipient"], g["recipient_leaf"], g["public"][2], g["recipient_path"])):
        alone, _ = W.poseidon_membership_circuit(params, G["height"], bytes.fromhex(leaf), idx, [le(h) for h in path])
        assert cs.witness[base:base + lay["membership_witnesses"]] == alone.witness
    sv, _ = W.schnorr_verification_circuit(S.GENERATOR, None, S.point_from_bytes(bytes.fromhex(g["sender_leaf"])[:64]),
                                           bytes.fromhex(g["message"]), bytes.fromhex(g["signature"]))
    assert cs.witness[:lay["balance"]] == sv.witness and [r[:sv.num_constraints] for r in cs.rows] == list(sv.rows)


def test_tampered_public_inputs_fail_the_row_that_names_them(G, params, systems):
    cs, public, failing = systems("valid")
    lay = W.payment_circuit_layout(params, G["height"])
    assert failing == []
    for k, want in ((0, [lay["sender_root_row"], lay["recipient_root_row"]]), (1, [lay["tie_rows"]]), (2, [lay["tie_rows"] + 1]),
                    (3, [lay["tie_rows"] + 2])):
        inst = [1] + public
        inst[1 + k] = (inst[1 + k] + 1) % R
        assert _failing_rows(cs, instance=inst) == want, k
    # the same through the builder's own override
    wrong, wrong_public = _build_with_root(params, G, (public[0] + 1) % R)
    assert wrong_public[0] == (public[0] + 1) % R and _failing_rows(wrong) == [lay["sender_root_row"], lay["recipient_root_row"]]
    # a balance bit that is not the leaf's: the packing row and the sender's leaf sponge
    w = list(cs.witness)
    w[lay["balance"] + 40] ^= 1
    bad = _failing_rows(cs, witness=w)
    assert bad[0] == lay["pack_row"] and bad[1] >= lay["sender_rows"] + 8 and bad[-1] < lay["recipient_bit_rows"]
    # an index bit that is not the id's: its tie row first
    w = list(cs.witness)
    w[lay["recipient"]] ^= 1
    assert _failing_rows(cs, witness=w)[0] == lay["recipient_rows"]


def _build_with_root(params, G, root):
    g = G["payments"][0]
    return W.payment_circuit(params, G["height"], bytes.fromhex(g["message"]), bytes.fromhex(g["signature"]), bytes.fromhex(g["sender_leaf"]),
                             [le(h) for h in g["sender_path"]], bytes.fromhex(g["recipient_leaf"]), [le(h) for h in g["recipient_path"]],
                             root=root)


def _shape(full, partial, alpha, height, salted):
    ni, nw, nc = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = load_library().swm_payment_circuit_shape(full, partial, alpha, height, salted, ctypes.byref(ni), ctypes.byref(nw), ctypes.byref(nc))
    return rc, (ni.value, nw.value, nc.value)


@pytest.mark.parametrize("salt", [None, SALT])
@pytest.mark.parametrize("height", [2, 4, 9])
def test_counts_builder_layout_library_and_formulas_agree(ref, params, height, salt):
    p = PM.payments(ref, height, salt, which=PM.PAYMENTS[-2:-1])[0]       # "to oneself": fits every height
    cs, public = W.payment_circuit(params, height, p["message"], p["signature"], p["sender_leaf"], p["sender_path"], p["recipient_leaf"],
                                   p["recipient_path"], salt=salt)
    assert public == p["public"] and _failing_rows(cs) == []
    got = (len(cs.instance), len(cs.witness), cs.num_constraints)
    lay = W.payment_circuit_layout(params, height, salt is not None)
    assert got == (lay["num_instance"], lay["num_witness"], lay["num_constraints"])
    assert _shape(8, 29, 17, height, 1 if salt else 0) == (0, got) and M.payment_circuit_shape(params, height, salt is not None) == got
    s, s_rows, levels = M.schnorr_circuit_shape(10, salt is not None)[1:] + (height - 1,)
    assert got == (5, s + 704 + 2 * (3 * levels + (2 + levels) * C), s_rows + 708 + 2 * (8 + 2 * C + levels * (2 + C) + 1))
    if height == 9 and salt is None:
        assert got == (5, 77197, 78186)      # the worked numbers
        assert [int(m[0][-1]) for m in cs.pack().mats] == [196786, 143524, 108363]


def test_the_matrices_of_two_payments_are_identical(systems):
    """One key serves all: the packed matrices depend on the shape alone."""
    a, b = systems("valid")[0].pack(), systems("balance 2^64 - 1")[0].pack()
    assert not np.array_equal(a.witness, b.witness)
    for ma, mb in zip(a.mats, b.mats):
        assert all(np.array_equal(x, y) for x, y in zip(ma, mb))


def test_synthesizer_class_and_public_inputs(G, params, systems):
    g = G["payments"][0]
    cs, public, _ = systems("valid")
    assert W.payment_public_inputs(public[0], bytes.fromhex(g["message"])) == public
    again = M.MarlinInst._synthesize(W.PaymentValidation(S.GENERATOR, None, params, G["height"], public[0], bytes.fromhex(g["message"]),
                                                         bytes.fromhex(g["signature"]), bytes.fromhex(g["sender_leaf"]),
                                                         [le(h) for h in g["sender_path"]], bytes.fromhex(g["recipient_leaf"]),
                                                         [le(h) for h in g["recipient_path"]]))
    assert again.witness == cs.witness and again.rows == cs.rows and again.instance == [1] + public


def test_builder_refusals(G, params):
    g = G["payments"][0]
    args = [bytes.fromhex(g["message"]), bytes.fromhex(g["signature"]), bytes.fromhex(g["sender_leaf"]), [le(h) for h in g["sender_path"]],
            bytes.fromhex(g["recipient_leaf"]), [le(h) for h in g["recipient_path"]]]
    for height in (1, 10):
        with pytest.raises(ValueError):
            W.payment_circuit_layout(params, height)
    for k, bad in ((0, args[0][:9]), (2, args[2][:71]), (4, args[4] + b"\0"), (3, args[3][:2]), (0, bytes([1, 8]) + args[0][2:]),
                   (2, R.to_bytes(32, "little") + args[2][32:]), (2, bytes([args[2][0] ^ 1]) + args[2][1:])):
        changed = list(args)
        changed[k] = bad
        with pytest.raises(ValueError):
            W.payment_circuit(params, 4, *changed)
    with pytest.raises(ValueError):
        W.payment_public_inputs(0, b"short")


def test_shape_call_without_a_gpu_and_its_refusals(params):
    lib = load_library()
    n = ctypes.c_size_t(0)
    for args in ((8, 29, 17, 1, 0), (8, 29, 17, 10, 0), (8, 29, 17, 31, 1), (7, 29, 17, 4, 0), (0, 29, 17, 4, 0), (8, 248, 17, 4, 0),
                 (8, 29, 1, 4, 0), (8, 29, 65536, 4, 0), (8, 29, 17, 1 << 62, 0), (1 << 63, 29, 17, 4, 0), (8, (1 << 64) - 8, 17, 4, 1)):
        assert _shape(*args)[0] == -1, args
    assert lib.swm_last_error(None).decode().startswith("payment_circuit_shape")
    assert _shape(8, 29, 17, 9, 1)[0] == 0 and _shape(8, 29, 17, 2, 0)[0] == 0
    assert lib.swm_payment_circuit_shape(8, 29, 17, 4, 0, None, ctypes.byref(n), ctypes.byref(n)) == -1
    assert lib.swm_payment_circuit_shape(8, 29, 17, 4, 0, ctypes.byref(n), None, ctypes.byref(n)) == -1
    assert lib.swm_payment_circuit_shape(8, 29, 17, 4, 0, ctypes.byref(n), ctypes.byref(n), None) == -1
    with pytest.raises(M.MarlinError) as e:
        M.payment_circuit_shape(params, 10)
    assert e.value.code == -1


def test_ffi_declares_the_new_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ffi = open(os.path.join(root, "swmarlin-sys", "src", "ffi.rs")).read()
    hdr = open(os.path.join(root, "include", "swmarlin.h")).read()
    names = ("swm_payment_circuit_shape", "swm_payment_circuit_create", "swm_payment_circuit_destroy", "swm_payment_witness",
             "swm_payment_witness_at", "swm_payment_witness_dev", "swm_payment_prove_at", "swm_payment_prove_many_at")
    for name in names:
        assert "pub fn %s(" % name in ffi and "%s(" % name in hdr
        assert hasattr(load_library(), name)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shape_under_asan_ubsan(tmp_path):
    """csrc/host/payment_shape.h — the counts and offsets the kernels write witnesses by — against the two shapes it is composed of,
    the formulas, and a cover of [0, num_witness) by its groups, in a stand-alone program (tests/native/payment_shape_check.cpp) built
    with -fsanitize=address,undefined."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "payment_shape_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(root, "simpleworks_amd", "csrc"), os.path.join(root, "tests", "native", "payment_shape_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and ("asan" in out.stderr.lower() or "ubsan" in out.stderr.lower()) and "error:" not in out.stderr:
        pytest.skip("this g++ has no ASan / UBSan runtime")
    assert out.returncode == 0, out.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) >= 8 * 2 * 5 * 6 + 18

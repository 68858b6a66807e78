"""CPU tests of the Schnorr verification circuit: its specification, workloads.build_schnorr_verification, evaluated row by row in
Python integers on fixture signatures and on tampered ones, its values against hashlib and the big-integer model
(tests/schnorr_model.py), and its SHAPE as the library states it without a GPU (swm_schnorr_circuit_shape,
csrc/host/schnorr_shape.h): the GPU witness synthesis (csrc/schnorr_witness.hip) lays its output out by these counts."""
import ctypes
import hashlib
import os
import shutil
import subprocess

import pytest

import schnorr_model as S
from oracle_lib import golden
from simpleworks_amd import marlin as M, workloads as W
from simpleworks_amd._lib import load_library

R = W.R_MODULUS
LENGTHS = (0, 1, 24, 63, 64, 65)   # the hash input (128 + len, or 160 + len) on, just before and just after a block boundary
CMP_ROWS = 8


@pytest.fixture(scope="module")
def G():
    return golden("schnorr.json")


def _signature(G, msg_len, salted):
    """(salt, public key, message, signature) of that length: the fixture's where it has one, the model's at the ledger's 24."""
    salt = bytes.fromhex(G["salt"]) if salted else None
    for v in G["valid"]:
        if v["salted"] == salted and len(v["message"]) == 2 * msg_len:
            return salt, S.point_from_bytes(bytes.fromhex(v["public_key"])), bytes.fromhex(v["message"]), bytes.fromhex(v["signature"])
    secret = int.from_bytes(hashlib.sha256(b"circuit secret %d" % msg_len).digest(), "little") % S.L
    nonce = int.from_bytes(hashlib.sha256(b"circuit nonce %d" % msg_len).digest(), "little") % S.L
    msg = hashlib.shake_128(b"circuit message").digest(msg_len)
    pk = S.keygen(S.GENERATOR, secret)
    sig = S.sign(S.GENERATOR, salt, secret, pk, nonce, msg)
    assert S.verify(S.GENERATOR, salt, S.point_bytes(pk), msg, sig)
    return salt, pk, msg, sig


@pytest.fixture(scope="module")
def systems(G):
    """(msg_len, salted) -> (inputs, the builder's ConstraintSystem); built once."""
    made = {}

    def get(msg_len, salted):
        if (msg_len, salted) not in made:
            salt, pk, msg, sig = _signature(G, msg_len, salted)
            cs, public = W.schnorr_verification_circuit(W.ED_GENERATOR, salt, pk, msg, sig)
            assert public == []
            made[msg_len, salted] = ((salt, pk, msg, sig), cs)
        return made[msg_len, salted]
    return get


def _failing_rows(cs):
    """The row evaluator: every row a z * b z == c z in Python integers; returns the indices of the rows that fail."""
    z = {("i", k): v for k, v in enumerate(cs.instance)}
    z.update({("w", k): v for k, v in enumerate(cs.witness)})

    def ev(lc):
        return sum(c * z[v] for c, v in lc) % R
    return [i for i, (a, b, c) in enumerate(zip(*cs.rows)) if ev(a) * ev(b) % R != ev(c)]


def _shape(msg_len, salted):
    lib = load_library()
    ni, nw, nc = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = lib.swm_schnorr_circuit_shape(msg_len, 1 if salted else 0, ctypes.byref(ni), ctypes.byref(nw), ctypes.byref(nc))
    return rc, (ni.value, nw.value, nc.value)


def _digest(cs, msg_len, salted):
    lay = W.schnorr_circuit_layout(msg_len, salted)
    bits = [cs.witness[lay["digest"] + 64 * (i // 32) + i % 32] for i in range(256)]
    assert set(bits) <= {0, 1}
    return sum(b << i for i, b in enumerate(bits)).to_bytes(32, "little")


def _commitment(cs, msg_len, salted):
    lay = W.schnorr_circuit_layout(msg_len, salted)
    return cs.witness[lay["sum"] + 5], cs.witness[lay["sum"] + 6]


@pytest.mark.parametrize("salted", [False, True])
@pytest.mark.parametrize("msg_len", LENGTHS)
def test_shape_and_fixture_signatures(systems, msg_len, salted):
    """The library's three counts are the builder's, and every row of the builder's system holds for a valid signature."""
    (salt, pk, msg, sig), cs = systems(msg_len, salted)
    rc, got = _shape(msg_len, salted)
    assert rc == 0
    assert got == (len(cs.instance), len(cs.witness), cs.num_constraints) == M.schnorr_circuit_shape(msg_len, salted)
    lay = W.schnorr_circuit_layout(msg_len, salted)
    assert got == (lay["num_instance"], lay["num_witness"], lay["num_constraints"])
    assert lay["blocks"] == (len(S.hash_input(salt, pk, (0, 1), msg)) + 63) // 64
    assert _failing_rows(cs) == []
    # the builder's values: the digest is hashlib's over the model's hash input, the commitment the model's
    commitment = S.commitment(S.GENERATOR, pk, int.from_bytes(sig[:32], "little"), sig[32:])
    assert _commitment(cs, msg_len, salted) == commitment
    assert _digest(cs, msg_len, salted) == hashlib.blake2s(S.hash_input(salt, pk, commitment, msg)).digest() == sig[32:]


@pytest.mark.parametrize("how", ["a bit of e", "a bit of s", "a message byte", "another signer's key"])
def test_tampered_inputs_fail_comparison_rows_only(G, systems, how):
    (salt, pk, msg, sig), good = systems(24, False)
    if how == "a bit of e":
        sig = sig[:50] + bytes([sig[50] ^ 0x04]) + sig[51:]
    elif how == "a bit of s":
        sig = sig[:7] + bytes([sig[7] ^ 0x80]) + sig[8:]
    elif how == "a message byte":
        msg = msg[:23] + bytes([msg[23] ^ 0xFF])
    else:
        pk = S.point_from_bytes(bytes.fromhex(G["valid"][5]["public_key"]))
    cs, _ = W.schnorr_verification_circuit(W.ED_GENERATOR, salt, pk, msg, sig)
    assert (len(cs.witness), cs.num_constraints) == (len(good.witness), good.num_constraints)
    bad = _failing_rows(cs)
    assert bad and min(bad) >= cs.num_constraints - CMP_ROWS
    # the digest is still the honest hash of what the circuit computed
    rx, ry = _commitment(cs, 24, False)
    assert _digest(cs, 24, False) == hashlib.blake2s(S.hash_input(salt, pk, (rx, ry), msg)).digest()


def test_key_outside_the_subgroup_follows_the_integer_challenge(G):
    """The system is well formed for an on-curve key outside the prime subgroup, and R' is s G + e Y with the INTEGER e: not the
    native scheme's (e mod l) Y.  The comparison outcome is whatever that rule gives."""
    def differs(c):   # Y = G + T with T of order 4: e Y and (e mod l) Y differ iff e and e mod l differ mod 4
        e = int.from_bytes(bytes.fromhex(c["challenge"]), "little")
        return e % 4 != e % S.L % 4
    cases = [c for c in G["commitments"] if c["note"].startswith("key = G + a point of order 4")]
    case = next((c for c in cases if differs(c)), cases[-1])
    pk = S.point_from_bytes(bytes.fromhex(case["public_key"]))
    assert W.ed_mul(pk, S.L) != (0, 1)
    sig = bytes.fromhex(case["response"]) + bytes.fromhex(case["challenge"])
    s, e = int.from_bytes(sig[:32], "little"), int.from_bytes(sig[32:], "little")
    cs, _ = W.schnorr_verification_circuit(W.ED_GENERATOR, None, pk, b"", sig)
    want = W.ed_add(W.ed_mul(W.ED_GENERATOR, s), W.ed_mul(pk, e))
    assert _commitment(cs, 0, False) == want
    native = S.point_from_bytes(bytes.fromhex(case["commitment"]))
    assert (want != native) == differs(case)
    digest = hashlib.blake2s(S.hash_input(None, pk, want, b"")).digest()
    assert _digest(cs, 0, False) == digest
    bad = _failing_rows(cs)
    assert (bad == []) == (digest == sig[32:])
    assert all(i >= cs.num_constraints - CMP_ROWS for i in bad)


def test_synthesizer_class_and_builder_argument_errors(G, systems):
    (salt, pk, msg, sig), cs = systems(0, False)
    again = M.MarlinInst._synthesize(W.SimpleSchnorrSignatureVerification(W.ED_GENERATOR, salt, pk, msg, sig))
    assert again.witness == cs.witness and again.rows == cs.rows
    off_curve = (pk[0], pk[1] ^ 1)
    for args in ((W.ED_GENERATOR, None, off_curve, msg, sig), (W.ED_GENERATOR, None, pk, msg, sig[:63]),
                 (W.ED_GENERATOR, b"short", pk, msg, sig), (off_curve, None, pk, msg, sig),
                 (W.ED_GENERATOR, None, pk, bytes(65537), sig)):
        with pytest.raises(ValueError):
            W.build_schnorr_verification(M.ConstraintSystem(), *args)


def test_shape_argument_errors():
    lib = load_library()
    for msg_len in (65537, 1 << 40):
        for salted in (False, True):
            assert _shape(msg_len, salted)[0] == -1, msg_len
    assert lib.swm_last_error(None).decode().startswith("schnorr_circuit_shape")
    n = ctypes.c_size_t(0)
    assert lib.swm_schnorr_circuit_shape(5, 0, None, ctypes.byref(n), ctypes.byref(n)) == -1
    assert lib.swm_schnorr_circuit_shape(5, 0, ctypes.byref(n), None, ctypes.byref(n)) == -1
    assert lib.swm_schnorr_circuit_shape(5, 0, ctypes.byref(n), ctypes.byref(n), None) == -1
    assert _shape(65536, True) == (0, (1, 6649 + 8 * 65536 + 21472 * 1027, 6672 + 8 * 65536 + 21792 * 1027))
    with pytest.raises(M.MarlinError) as e:
        M.schnorr_circuit_shape(65537)
    assert e.value.code == -1
    # SchnorrCircuit.shape() is this call on the wrapper's own (msg_len, salt): no GPU handle is needed to ask
    from simpleworks_amd.schnorr import SchnorrCircuit
    sc = SchnorrCircuit.__new__(SchnorrCircuit)
    sc.h, sc.msg_len, sc.params = None, 24, type("P", (), {"salt": None})()
    assert sc.shape() == (1, 71257, 72240)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shape_and_schedule_under_asan_ubsan(tmp_path):
    """csrc/host/schnorr_shape.h — the offset arithmetic and the Blake2s schedule the kernel writes witnesses by — in a stand-alone
    program (tests/native/schnorr_shape_check.cpp) built with -fsanitize=address,undefined."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "schnorr_shape_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(root, "simpleworks_amd", "csrc"), os.path.join(root, "tests", "native", "schnorr_shape_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and ("asan" in out.stderr.lower() or "ubsan" in out.stderr.lower()) and "error:" not in out.stderr:
        pytest.skip("this g++ has no ASan / UBSan runtime")
    assert out.returncode == 0, out.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) >= 32 and int(run.stdout.split()[2]) >= 100

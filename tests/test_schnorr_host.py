"""CPU tests of the Schnorr scheme's test infrastructure and binding: the big-integer model (tests/schnorr_model.py) against the
committed fixture (tests/golden/schnorr.json), the byte layout of the hash input, the scalar draw, and the seven symbols of the C ABI
(include/swmarlin.h, libswmarlin.so, simpleworks_amd/_lib.py).  Reference: src/schnorr_signature/schnorr.rs."""
import hashlib
import os
import re

import pytest

import schnorr_model as S
from oracle_lib import golden
from pyref.pedersen import ED_SUBGROUP_ORDER as L
from pyref.pedersen import ed_mul, ed_on_curve
from pyref import rng as pyrng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["swm_schnorr_create", "swm_schnorr_destroy", "swm_schnorr_keygen", "swm_schnorr_sign", "swm_schnorr_verify",
           "swm_schnorr_commitments"]


@pytest.fixture(scope="module")
def g():
    return golden("schnorr.json")


def test_fixture_shape(g):
    assert len(g["valid"]) == 64 and len(g["commitments"]) >= 40
    assert g["generator"] == S.point_bytes(S.GENERATOR).hex() and int(g["group_order"], 16) == L
    assert {len(v["message"]) // 2 for v in g["valid"]} == set(g["lengths"]) == {0, 1, 11, 63, 64, 65, 200}
    assert {v["salted"] for v in g["valid"]} == {True, False}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "schnorr.json")) < 200 * 1024


def test_generator_is_on_the_curve_and_of_prime_order():
    assert ed_on_curve(S.GENERATOR) and S.GENERATOR != S.IDENTITY and ed_mul(S.GENERATOR, L) == S.IDENTITY


def test_model_signs_the_fixture_inputs_to_the_fixture_bytes(g):
    salt = bytes.fromhex(g["salt"])
    for i, v in enumerate(g["valid"]):
        x, k = int.from_bytes(bytes.fromhex(v["secret"]), "little"), int.from_bytes(bytes.fromhex(v["nonce"]), "little")
        pk = S.keygen(S.GENERATOR, x)
        assert S.point_bytes(pk).hex() == v["public_key"], i
        sig = S.sign(S.GENERATOR, salt if v["salted"] else None, x, pk, k, bytes.fromhex(v["message"]))
        assert sig.hex() == v["signature"], i


def test_model_verifies_and_rejects(g):
    salt = bytes.fromhex(g["salt"])
    for i in (0, 1, 27, 62):
        v = g["valid"][i]
        pk, msg, sig = bytes.fromhex(v["public_key"]), bytes.fromhex(v["message"]), bytes.fromhex(v["signature"])
        s = salt if v["salted"] else None
        assert S.verify(S.GENERATOR, s, pk, msg, sig), i
        assert not S.verify(S.GENERATOR, None if v["salted"] else salt, pk, msg, sig), i
        assert not S.verify(S.GENERATOR, s, pk, msg + b"\x00", sig), i
        assert not S.verify(S.GENERATOR, s, pk, msg, bytes([sig[0] ^ 1]) + sig[1:]), i
        assert not S.verify(S.GENERATOR, s, bytes([pk[0] ^ 1]) + pk[1:], msg, sig), i
    v = g["valid"][0]
    big = (int.from_bytes(bytes.fromhex(v["signature"])[:32], "little") + L).to_bytes(32, "little")   # the same response, not canonical
    assert not S.verify(S.GENERATOR, None, bytes.fromhex(v["public_key"]), bytes.fromhex(v["message"]), big + bytes.fromhex(v["signature"])[32:])


def test_model_commitments_equal_the_fixture(g):
    for c in g["commitments"][::3] + g["commitments"][-2:]:
        pk = S.point_from_bytes(bytes.fromhex(c["public_key"]))
        got = S.commitment(S.GENERATOR, pk, int.from_bytes(bytes.fromhex(c["response"]), "little"), bytes.fromhex(c["challenge"]))
        assert S.point_bytes(got).hex() == c["commitment"], c["note"]
    assert g["commitments"][-1]["commitment"] == S.point_bytes(S.IDENTITY).hex()


def test_hash_input_layout():
    """schnorr.rs:98-104: [salt] || pk.x || pk.y || R.x || R.y || message, coordinates as 32 little-endian bytes."""
    pk, r = (3, 0x0102030405), (7, 1 << 250)
    msg, salt = b"hello world", bytes(range(32))
    by_hand = (b"\x03" + bytes(31)) + (b"\x05\x04\x03\x02\x01" + bytes(27)) + (b"\x07" + bytes(31)) + (bytes(31) + b"\x04") + msg
    assert S.hash_input(None, pk, r, msg) == by_hand and len(by_hand) == 128 + 11
    assert S.hash_input(salt, pk, r, msg) == salt + by_hand
    assert S.challenge(None, pk, r, msg) == hashlib.blake2s(by_hand, digest_size=32).digest()
    assert S.challenge(salt, pk, r, b"") == hashlib.blake2s(salt + by_hand[:128]).digest()


def test_scalar_draw_rule():
    """32 bytes of the stream, top five bits cleared, retried while >= l, read as a Montgomery representation [U]."""
    a, b = pyrng.test_rng(), pyrng.test_rng()
    for _ in range(8):
        while True:
            raw = sum(b.next_u64() << (64 * i) for i in range(4)) & ((1 << 251) - 1)
            if raw < L:
                break
        v = S.draw_scalar(a)
        assert v < L and v * (1 << 256) % L == raw


def test_mirror_draws_equal_the_model():
    """simpleworks_amd.schnorr.rand_scalar on the library's test_rng against the model's draw on the Python generator."""
    from simpleworks_amd import marlin as M
    from simpleworks_amd import schnorr as SCH
    assert SCH.GROUP_ORDER == L and SCH.GENERATOR == S.GENERATOR
    lib_rng, py_rng = M.generate_rand(), pyrng.test_rng()
    assert [SCH.rand_scalar(lib_rng) for _ in range(40)] == [S.draw_scalar(py_rng) for _ in range(40)]


def test_seven_symbols_declared_exported_and_bound():
    """typedef struct swm_schnorr and the six functions: in the header, in the library, in the binding's ABI table and as Context methods."""
    import simpleworks_amd._lib as B
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "swmarlin.h")).read(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+swm_schnorr\s+swm_schnorr\s*;", header)
    lib = B.load_library()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared in swmarlin.h" % name
        assert hasattr(lib, name), "%s is not exported" % name
        assert name in B.ABI, "%s is not bound" % name
        assert hasattr(B.Context, name[len("swm_"):]), "Context lacks %s" % name[len("swm_"):]
    ffi = open(os.path.join(ROOT, "swmarlin-sys", "src", "ffi.rs")).read()
    assert "pub struct swm_schnorr" in ffi
    for name in SYMBOLS:
        assert re.search(r"pub fn %s\s*\(" % name, ffi), "%s is not declared in swmarlin-sys" % name

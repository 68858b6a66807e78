"""CPU tests of the ElGamal scheme's test infrastructure and binding: the big-integer model (tests/elgamal_model.py) against the
committed fixture (tests/golden/elgamal.json), the fixture against its generator, the draws of the mirror, and the symbols of the
C ABI (include/swmarlin.h, libswmarlin.so, simpleworks_amd/_lib.py).  Reference: tests/encrypt.rs:11-28."""
import importlib.util
import json
import os
import re

import pytest

import elgamal_model as E
from oracle_lib import golden
from pyref import rng as pyrng
from pyref.pedersen import ED_SUBGROUP_ORDER as L
from pyref.pedersen import ed_mul, ed_on_curve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "elgamal.json")
SYMBOLS = ["swm_elgamal_create", "swm_elgamal_destroy", "swm_elgamal_keygen", "swm_elgamal_key_create", "swm_elgamal_key_destroy",
           "swm_elgamal_encrypt", "swm_elgamal_encrypt_to", "swm_elgamal_decrypt"]


@pytest.fixture(scope="module")
def g():
    return golden("elgamal.json")


def _pt(h):
    p = E.point_from_bytes(bytes.fromhex(h))
    assert p is not None
    return p


def _sc(h):
    return int.from_bytes(bytes.fromhex(h), "little")


def test_fixture_shape(g):
    assert len(g["valid"]) == 64 and len(g["edge"]) >= 40 and int(g["group_order"], 16) == L
    assert all(c["note"] for c in g["edge"]) and len({c["note"] for c in g["edge"]}) == len(g["edge"])
    assert os.path.getsize(FIXTURE) < 200 * 1024
    G = _pt(g["generator"])
    assert ed_on_curve(G) and G != E.IDENTITY and ed_mul(G, L) == E.IDENTITY
    scalars = {_sc(c["scalar"]) for c in g["edge"]}
    assert {0, 1, 2, L - 1, L - 2, 0xF, int("0" + "1" * 63, 16)} <= scalars and all(k < L for k in scalars)
    points = {c["point"] for c in g["edge"]} & {c["message"] for c in g["edge"]}        # what both the key and the message take
    identity = E.point_bytes(E.IDENTITY).hex()
    assert identity in points
    assert any(ed_mul(_pt(p), 2) == E.IDENTITY and _pt(p) != E.IDENTITY for p in points)
    assert any(ed_mul(_pt(p), 4) == E.IDENTITY and ed_mul(_pt(p), 2) != E.IDENTITY for p in points)
    assert any(ed_mul(_pt(p), L) != E.IDENTITY and ed_mul(_pt(p), 4) != E.IDENTITY for p in points)
    assert any(c["c2"] == identity and c["message"] != identity for c in g["edge"])
    assert any(c["point"] == g["generator"] for c in g["edge"])


def test_the_first_tuple_is_the_draw_order_of_encrypt_rs(g):
    """generator, sk, message, r: four draws from a fresh test_rng."""
    rng = pyrng.test_rng()
    G = E.setup(rng)
    pk, sk = E.keygen(G, rng)
    m, r = E.rand_plaintext(rng), E.rand_randomness(rng)
    v = g["valid"][0]
    assert (E.point_bytes(G).hex(), sk, E.point_bytes(pk).hex(), E.point_bytes(m).hex(), r) == \
        (g["generator"], _sc(v["secret"]), v["public_key"], v["message"], _sc(v["randomness"]))
    assert E.ciphertext_bytes(E.encrypt(G, pk, m, r)).hex() == v["c1"] + v["c2"]


def test_model_decrypts_what_it_encrypted(g):
    G = _pt(g["generator"])
    for i, v in enumerate(g["valid"]):
        assert E.decrypt(_sc(v["secret"]), (_pt(v["c1"]), _pt(v["c2"]))) == _pt(v["message"]), i
    sk0 = _sc(g["valid"][0]["secret"])
    for i in (1, 31, 63):                                            # what went to tuple 0's key opens under tuple 0's secret
        v = g["valid"][i]
        assert E.decrypt(sk0, (_pt(v["c1"]), _pt(v["c2_to_key0"]))) == _pt(v["message"]), i
        assert E.ciphertext_bytes(E.encrypt(G, _pt(v["public_key"]), _pt(v["message"]), _sc(v["randomness"]))).hex() == v["c1"] + v["c2"]
    for c in g["edge"]:
        # (point, c2) is the ciphertext of `message` under the secret `scalar` when `point` plays c1: c2 - k point = message
        k, p, m = _sc(c["scalar"]), _pt(c["point"]), _pt(c["message"])
        assert E.decrypt(k, (p, _pt(c["c2"]))) == m, c["note"]
        assert E.point_bytes(E.decrypt(k, (p, m))).hex() == c["plaintext"], c["note"]


def test_committed_fixture_equals_a_fresh_run_of_its_generator():
    spec = importlib.util.spec_from_file_location("gen_golden_elgamal", os.path.join(ROOT, "tests", "golden", "gen_golden_elgamal.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert json.dumps(gen.build(), indent=1) == open(FIXTURE).read()


def test_mirror_draws_equal_the_model():
    """simpleworks_amd.elgamal's draws on the library's test_rng against the model's on the Python generator, in encrypt.rs's order
    and beyond it."""
    from simpleworks_amd import marlin as M
    from simpleworks_amd import elgamal as EG
    assert EG.GROUP_ORDER == L
    lib_rng, py_rng = M.generate_rand(), pyrng.test_rng()
    for _ in range(3):
        assert EG.rand_plaintext(lib_rng) == E.rand_plaintext(py_rng)          # setup's draw is this one
        assert EG.rand_scalar(lib_rng) == E.draw_scalar(py_rng)                # keygen's
        assert EG.rand_plaintext(lib_rng) == E.rand_plaintext(py_rng)
        assert EG.rand_randomness(lib_rng) == E.rand_randomness(py_rng)


def test_symbols_declared_exported_and_bound():
    """The two handle types and the eight functions: in the header, in the library, in the binding's ABI table and as Context
    methods; the mirror module is exported from the package."""
    import simpleworks_amd
    import simpleworks_amd._lib as B
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "swmarlin.h")).read(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+swm_elgamal\s+swm_elgamal\s*;", header)
    assert re.search(r"typedef\s+struct\s+swm_elgamal_key\s+swm_elgamal_key\s*;", header)
    lib = B.load_library()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared in swmarlin.h" % name
        assert hasattr(lib, name), "%s is not exported" % name
        assert name in B.ABI, "%s is not bound" % name
        assert hasattr(B.Context, name[len("swm_"):]), "Context lacks %s" % name[len("swm_"):]
    for name in ("Parameters", "ResidentKey", "SecretKey", "setup", "keygen", "rand_randomness", "rand_plaintext", "encrypt", "decrypt",
                 "keygen_many", "encrypt_many", "decrypt_many"):
        assert hasattr(simpleworks_amd.elgamal, name), name

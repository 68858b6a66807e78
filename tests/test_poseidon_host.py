"""CPU tests of the Poseidon sponge's host side: the byte-to-element rule as the library states it without a GPU
(swm_poseidon_pack_bytes, csrc/host/host_abi.inc) against the model tests/poseidon_model.py, the parameter loader, the committed
fixture against the model, and the model itself against an identity that does not share its structure."""
import ctypes
import os

import numpy as np
import pytest

import poseidon_model as P
from oracle_lib import golden
from pyref.bls12_377 import R
from simpleworks_amd import hash as H
from simpleworks_amd._lib import load_library

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARAMS = os.path.join(GOLDEN, "poseidon_params.json")
INVALID_ARG = -1
# 8 + length crosses a 31-byte chunk boundary at 23 -> 24 and 54 -> 55 (the element count crosses the rate there) and at 85 -> 86
LENGTHS = [0, 1, 22, 23, 24, 54, 55, 85, 86, 1000]


def _pack(data, cap):
    """-> (return code, n_elems, the cap x 32 output bytes, pre-filled with 0xAA)"""
    lib = load_library()
    out = np.full((max(cap, 1), 32), 0xAA, dtype=np.uint8)
    n = ctypes.c_size_t(12345)
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    rc = lib.swm_poseidon_pack_bytes(src.ctypes.data if len(data) else None, len(data), out.ctypes.data, cap, ctypes.byref(n))
    return rc, n.value, out


@pytest.mark.parametrize("length", LENGTHS)
def test_pack_bytes_equals_the_model(length):
    data = P.poseidon_input(length, 1) if length else b""
    want = P.pack_bytes(data)
    assert len(want) == (8 + length + 30) // 31 and all(v < 1 << 248 for v in want)
    rc, n, out = _pack(data, len(want) + 1)
    assert rc == 0 and n == len(want)
    assert [int.from_bytes(out[i].tobytes(), "little") for i in range(n)] == want
    assert (out[n] == 0xAA).all(), "wrote past the last element"
    assert H.poseidon_pack_bytes(data) == want


def test_pack_bytes_all_ones_fills_every_chunk_byte():
    data = b"\xff" * 54          # 62 bytes with the prefix: exactly two full chunks
    rc, n, out = _pack(data, 2)
    assert rc == 0 and n == 2
    assert [int.from_bytes(out[i].tobytes(), "little") for i in range(2)] == P.pack_bytes(data)
    assert out[1, 31] == 0 and (out[1, :31] == 0xFF).all()


@pytest.mark.parametrize("length", [0, 23, 24, 1000])
def test_pack_bytes_refuses_a_small_buffer_and_reports_the_count(length):
    need = (8 + length + 30) // 31
    rc, n, out = _pack(b"\x01" * length, need - 1)
    assert rc == INVALID_ARG and n == need
    assert (out == 0xAA).all(), "a refused call wrote elements"
    lib = load_library()
    n = ctypes.c_size_t(0)
    assert lib.swm_poseidon_pack_bytes(None, 0, None, 0, ctypes.byref(n)) == INVALID_ARG and n.value == 1   # the size query
    assert lib.swm_poseidon_pack_bytes(None, 0, None, 0, None) == INVALID_ARG
    assert lib.swm_poseidon_pack_bytes(None, 5, out.ctypes.data, 1, ctypes.byref(n)) == INVALID_ARG


def test_loader_reduces_the_oversize_strings():
    import json
    with open(PARAMS) as f:
        raw = json.load(f)
    strings = [s for row in raw["mds"] + raw["ark"] for s in row]
    assert len(strings) == 9 + 111 and sum(int(s) >= R for s in strings) == 86
    p = H.PoseidonParameters.from_json(PARAMS)
    assert (p.full_rounds, p.partial_rounds, p.alpha) == (8, 29, 17)
    flat = [v for row in p.mds + p.ark for v in row]
    assert flat == [int(s) % R for s in strings] and all(0 <= v < R for v in flat)
    model = P.load_params(PARAMS)
    assert model == (8, 29, 17, p.mds, p.ark)
    with pytest.raises(ValueError):
        H.PoseidonParameters(8, 29, 17, p.mds, p.ark[:36])
    with pytest.raises(ValueError):
        H.PoseidonParameters(8, 29, 17, p.mds[:2], p.ark)


@pytest.mark.parametrize("full,partial,alpha", [(8, 29, 17), (2, 0, 2), (2, 5, 3), (8, 0, 65535)])
def test_model_against_a_power_identity(full, partial, alpha):
    """With mds = identity and ark = 0 the entries never mix and state[0] meets the S-box in every round: one absorbed x squeezes
    to x^(alpha^(F + P)), which Python's pow states without a sponge, a round loop or a matrix."""
    params = P.adversarial_params("identity", full, partial, alpha, None)
    for x in (0, 1, 2, R - 1, P.fr("power identity")):
        assert P.hash_elements(params, [x], 1) == [pow(x, alpha ** (full + partial), R)]
    # state[1] meets it in the full rounds only
    x, y = P.fr("power identity left"), P.fr("power identity right")
    assert P.hash_elements(params, [x, y], 2) == [pow(x, alpha ** (full + partial), R), pow(y, alpha ** full, R)]


def test_model_sponge_bookkeeping():
    """Absorbing nothing does nothing; squeezing is prefix-consistent; a third output comes from a second permutation."""
    ref = P.load_params(PARAMS)
    zero = P.permute(ref, [0, 0, 0])
    assert P.hash_elements(ref, [], 3) == zero[:2] + P.permute(ref, zero)[:1]
    item = [P.fr("bookkeeping %d" % k) for k in range(3)]
    three = P.hash_elements(ref, item, 3)
    assert P.hash_elements(ref, item, 1) == three[:1] and P.hash_elements(ref, item, 2) == three[:2]
    s = P.permute(ref, [item[0], item[1], 0])
    s[0] = (s[0] + item[2]) % R
    assert three[:2] == P.permute(ref, s)[:2]
    assert P.hash_bytes(ref, b"") == P.hash_elements(ref, [0], 1)[0]        # the length prefix alone: one zero element


def test_fixture_is_what_the_model_gives():
    """A sample of tests/golden/poseidon.json recomputed (the generator writes all of it from the same model)."""
    G = golden("poseidon.json")
    ref = P.load_params(PARAMS)
    le = lambda h: int.from_bytes(bytes.fromhex(h), "little")
    assert set(G["lengths"]) >= {0, 11, 22, 23, 24, 54, 55, 85, 86, 300}
    for ln in G["lengths"]:
        digests = G["bytes"][str(ln)]
        assert len(digests) == (1 if ln == 0 else G["per_length"])
        for i in (0, len(digests) - 1):
            assert le(digests[i]) == P.hash_bytes(ref, P.poseidon_input(ln, i)), (ln, i)
    assert P.poseidon_input(11, 0) == b"Hello World"
    for case in G["elements"][::5]:
        assert [le(h) for h in case["out"]] == P.hash_elements(ref, [le(h) for h in case["in"]], 3)
    assert le(G["compress"][-1]) == P.hash_elements(ref, P.poseidon_pair(len(G["compress"]) - 1), 1)[0]
    items = [[le(h) for h in item] for item in G["adversarial_items"]]
    for case in G["adversarial"][::7]:
        params = P.adversarial_params(case["fill"], case["full_rounds"], case["partial_rounds"], case["alpha"], ref)
        assert [[le(h) for h in o] for o in case["out"]] == [P.hash_elements(params, item, 3) for item in items]

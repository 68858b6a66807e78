"""CPU tests of the uncompressed forms of the VERIFYING key (swm_vk_serialize_ex / swm_vk_deserialize_ex, host only): the
serialize_uncompressed layout against bytes written by an independent serializer from the Python model's keys
(tests/golden/key_forms.json, gen_golden_key_forms.py), and what the checked (deserialize_uncompressed) and the unchecked
(deserialize_unchecked) readers refuse.

Layout of an uncompressed vk: 4 x u64 | u64 12 | 12 x (G1 96 B + tag 0) | g | gamma_g | h 192 B | beta_h 192 B | 1 | u64 k |
k x (u64, G1) | 2 x u64.  The first G1 (index_comms[0].comm) is at byte 40, h at 40 + 12 * 97 + 192 = 1396."""
import ctypes
import hashlib

import pytest

from oracle_lib import golden

import simpleworks_amd._lib as L
from simpleworks_amd import marlin as M
from simpleworks_amd import serialization as S

Q = 0x1ae3a4617c510eac63b05c06ca1493b1a22d9f300f5138f1ef3622fba094800170b5d44300000008508c00000000001
NAMES = ["manual_constraints", "synthetic_8", "random_sparse"]
G1_AT, H_AT = 40, 40 + 12 * 97 + 192
CHECKED, UNCHECKED = S.KEY_UNCOMPRESSED, S.KEY_UNCOMPRESSED | S.KEY_UNCHECKED
ERR_INVALID_ARG, ERR_SERIALIZATION = -1, -7


@pytest.fixture(scope="module")
def lib():
    return L.load_library()


@pytest.fixture(scope="module")
def forms():
    return golden("key_forms.json")


def _load(lib, data, flags):
    """(return code, handle or None) of swm_vk_deserialize_ex"""
    buf = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
    h = ctypes.c_void_p()
    rc = lib.swm_vk_deserialize_ex(buf, len(data), flags, ctypes.byref(h))
    return rc, (M.VerifyingKey(h) if rc == 0 else None)


def _put(data, at, value, width=48):
    out = bytearray(data)
    out[at:at + width] = value.to_bytes(width, "little")
    return bytes(out)


@pytest.mark.parametrize("name", NAMES)
def test_vk_round_trips_between_the_forms(forms, name):
    case = forms[name]
    comp, unc = bytes.fromhex(case["vk_compressed"]), bytes.fromhex(case["vk_bytes"])
    assert len(unc) == case["vk"]["len"] and hashlib.sha256(unc).hexdigest() == case["vk"]["sha256"]
    vk = S.deserialize_verifying_key(comp)
    got = S.serialize_verifying_key(vk, uncompressed=True)
    assert got[:64].hex() == case["vk"]["head"]
    assert got == unc
    for unchecked in (False, True):
        back = S.deserialize_verifying_key(unc, uncompressed=True, unchecked=unchecked)
        assert S.serialize_verifying_key(back) == comp
        assert S.serialize_verifying_key(back, uncompressed=True) == unc
    # the two forms are not each other's: a reader of one refuses the other
    for data, kw in ((comp, {"uncompressed": True}), (comp, {"uncompressed": True, "unchecked": True}), (unc, {})):
        with pytest.raises(M.MarlinError) as e:
            S.deserialize_verifying_key(data, **kw)
        assert e.value.code == ERR_SERIALIZATION


def test_flags_zero_is_the_existing_codec(lib, forms):
    comp = bytes.fromhex(forms["random_sparse"]["vk_compressed"])
    vk = S.deserialize_verifying_key(comp)
    n0, n1 = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.swm_vk_serialize(vk.h, None, 0, ctypes.byref(n0)) == 0
    assert lib.swm_vk_serialize_ex(vk.h, 0, None, 0, ctypes.byref(n1)) == 0  # out == NULL: the length
    assert n0.value == n1.value == len(comp)
    a, b = (ctypes.c_uint8 * n0.value)(), (ctypes.c_uint8 * n0.value)()
    assert lib.swm_vk_serialize(vk.h, a, n0.value, ctypes.byref(n0)) == 0
    assert lib.swm_vk_serialize_ex(vk.h, 0, b, n1.value, ctypes.byref(n1)) == 0
    assert bytes(a) == bytes(b) == comp
    assert lib.swm_vk_serialize_ex(vk.h, S.KEY_UNCOMPRESSED, b, n1.value, ctypes.byref(n1)) == ERR_INVALID_ARG  # buffer too small
    rc, vk0 = _load(lib, comp, 0)
    assert rc == 0 and S.serialize_verifying_key(vk0) == comp


def test_bad_flag_combinations(lib, forms):
    case = forms["synthetic_8"]
    comp, unc = bytes.fromhex(case["vk_compressed"]), bytes.fromhex(case["vk_bytes"])
    vk = S.deserialize_verifying_key(comp)
    n = ctypes.c_size_t(0)
    for flags in (S.KEY_UNCHECKED, UNCHECKED, 4, 4 | S.KEY_UNCOMPRESSED, 0x80000000):  # UNCHECKED is a reader's flag
        assert lib.swm_vk_serialize_ex(vk.h, flags, None, 0, ctypes.byref(n)) == ERR_INVALID_ARG, flags
    for flags in (S.KEY_UNCHECKED, 4, 4 | S.KEY_UNCOMPRESSED, 7, 0x80000000):  # UNCHECKED only together with UNCOMPRESSED
        for data in (comp, unc):
            assert _load(lib, data, flags)[0] == ERR_INVALID_ARG, flags


@pytest.mark.parametrize("flags", [CHECKED, UNCHECKED], ids=["checked", "unchecked"])
def test_malformed_bytes_are_refused_in_both_modes(lib, forms, flags):
    unc = bytes.fromhex(forms["manual_constraints"]["vk_bytes"])
    assert _load(lib, unc, flags)[0] == 0
    bad = {
        "truncated": unc[:-1],
        "truncated inside a point": unc[:G1_AT + 50],
        "empty": b"",
        "trailing byte": unc + b"\x00",
        # SWFlags: infinity AND the sign bit is no valid combination, G1 (last byte of y) and G2 (last byte of y.c1)
        "G1 flags 0xC0": unc[:G1_AT + 95] + bytes([unc[G1_AT + 95] | 0xC0]) + unc[G1_AT + 96:],
        "G2 flags 0xC0": unc[:H_AT + 191] + bytes([unc[H_AT + 191] | 0xC0]) + unc[H_AT + 192:],
        # Fp::deserialize refuses a non-canonical coordinate in every mode
        "G1 x = q": _put(unc, G1_AT, Q),
        "G1 y = q": _put(unc, G1_AT + 48, Q),
        "G2 x.c1 = q": _put(unc, H_AT + 48, Q),
        "G2 y.c0 = q + 1": _put(unc, H_AT + 96, Q + 1),
        # ... also under the infinity flag, whose coordinates are read and then ignored
        "G1 infinity with x = q": _put(_put(unc, G1_AT, Q), G1_AT + 48, 1 | (0x40 << 376)),
    }
    for what, data in bad.items():
        assert _load(lib, data, flags)[0] == ERR_SERIALIZATION, what


def test_points_off_the_curve_and_off_the_subgroup(lib, forms):
    """deserialize_uncompressed evaluates the curve equation and [r]P = O; deserialize_unchecked takes the coordinates as they are."""
    unc = bytes.fromhex(forms["manual_constraints"]["vk_bytes"])
    y = int.from_bytes(unc[G1_AT + 48:G1_AT + 96], "little")
    yc0 = int.from_bytes(unc[H_AT + 96:H_AT + 144], "little")
    assert y + 1 < Q and yc0 + 1 < Q and not unc[G1_AT + 95] & 0xC0 and not unc[H_AT + 191] & 0xC0
    # a point of the curve outside the prime-order subgroup (the cofactor of BLS12-377 G1 is ~2^125: almost every curve point)
    from pyref import bls12_377 as bls
    x = 5
    while True:
        ys = bls.fq_sqrt((x * x * x + 1) % Q)
        if ys is not None and bls.g1_mul_fast((x, ys), bls.R) is not None:
            break
        x += 1
    cases = {"G1 off the curve": _put(unc, G1_AT + 48, y + 1), "G2 off the curve": _put(unc, H_AT + 96, yc0 + 1),
             "G1 off the subgroup": _put(_put(unc, G1_AT, x), G1_AT + 48, ys)}
    for what, data in cases.items():
        assert _load(lib, data, CHECKED)[0] == ERR_SERIALIZATION, what
        rc, vk = _load(lib, data, UNCHECKED)
        assert rc == 0, what
        assert S.serialize_verifying_key(vk, uncompressed=True) == data, what  # taken as it is, written back as it is
    # the identity, as arkworks writes it — (0, 1) with the infinity flag — is a valid point in both modes
    ident = _put(_put(unc, G1_AT, 0), G1_AT + 48, 1 | (0x40 << 376))
    for flags in (CHECKED, UNCHECKED):
        rc, vk = _load(lib, ident, flags)
        assert rc == 0 and S.serialize_verifying_key(vk, uncompressed=True) == ident
    g2_ident = _put(_put(_put(_put(unc, H_AT, 0), H_AT + 48, 0), H_AT + 96, 1), H_AT + 144, 0x40 << 376)
    for flags in (CHECKED, UNCHECKED):
        rc, vk = _load(lib, g2_ident, flags)
        assert rc == 0 and S.serialize_verifying_key(vk, uncompressed=True) == g2_ident

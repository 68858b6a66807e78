"""GPU tests of the uncompressed forms of the PROVING key (swm_pk_serialize_ex / swm_pk_deserialize_ex) and of their point kernels
(g1_encode_uncompressed_kernel, g1_decode_uncompressed_kernel<checked / unchecked>, through swm_selftest_g1_codec):
  1. the kernels against Python integers, one lane to several workgroups with a ragged tail, the identity, and one malformed point
     of every kind the decoders tell apart;
  2. the serialize_uncompressed bytes of three small keys against an independent serializer over the Python model's keys
     (tests/golden/key_forms.json);
  3. uncompressed bytes load — checked and unchecked — into keys that re-serialize and prove like the original;
  4. what the two readers refuse."""
import ctypes
import hashlib

import numpy as np
import pytest

from oracle_lib import Q, golden, h2i

pytestmark = pytest.mark.gpu

CHECKED, UNCHECKED = 1, 3  # SWM_KEY_UNCOMPRESSED, | SWM_KEY_UNCHECKED
ERR_INVALID_ARG, ERR_SERIALIZATION = -1, -7
MONT = 1 << 384  # the Montgomery radix of Fq in memory: 12 words of 32 bits


@pytest.fixture(scope="module")
def M():
    from simpleworks_amd import marlin
    return marlin


@pytest.fixture(scope="module")
def S():
    from simpleworks_amd import serialization
    return serialization


@pytest.fixture(scope="module")
def W():
    from simpleworks_amd import workloads
    return workloads


@pytest.fixture(scope="module")
def off_subgroup():
    """a point of the curve outside the prime-order subgroup, found as tests/test_gpu_marlin.py finds one"""
    from pyref import bls12_377 as bls
    x = 5
    while True:
        y = bls.fq_sqrt((x * x * x + 1) % Q)
        if y is not None and bls.g1_mul_fast((x, y), bls.R) is not None:
            return x, y
        x += 1


# ------------------------------------------------------------------------------------------------ 1. kernels
@pytest.fixture(scope="module")
def multiples():
    """[1]G .. [1025]G from the model, computed once"""
    from pyref import bls12_377 as bls
    G = tuple(h2i(v) for v in golden("g1.json")["generator"])
    out, P = [], None
    for _ in range(1025):
        P = bls.g1_add(P, G)
        out.append(P)
    return out


def _limbs(points):
    """affine Montgomery limbs as the device holds them: n x 12 uint64, (0, 0) for the identity"""
    raw = b"".join((b"\0" * 96) if P is None else
                   (P[0] * MONT % Q).to_bytes(48, "little") + (P[1] * MONT % Q).to_bytes(48, "little") for P in points)
    return np.frombuffer(raw, dtype=np.uint64).reshape(len(points), 12).copy()


def _enc(P):
    """serialize_uncompressed of one point [U: ark-ec 0.3]"""
    if P is None:
        return (0).to_bytes(48, "little") + (1 | (0x40 << 376)).to_bytes(48, "little")
    return P[0].to_bytes(48, "little") + P[1].to_bytes(48, "little")


def _case(multiples, n):
    pts = list(multiples[:n])
    if n == 257:
        for i in (0, 255, 256):
            pts[i] = None
    return pts


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_codec_kernels_against_python_integers(M, multiples, n):
    ctx = M.default_context()
    pts = _case(multiples, n)
    limbs, want = _limbs(pts), b"".join(_enc(P) for P in pts)
    assert ctx.selftest_g1_codec("encode", limbs, n) == want
    for op in ("decode", "decode_unchecked"):
        got, bad = ctx.selftest_g1_codec(op, want, n)
        assert bad == 0, op
        assert np.array_equal(got, limbs), op


def test_codec_kernels_report_each_kind_of_bad_point(M, multiples, off_subgroup):
    """one crafted element per run, at the last index of the 257 case (lane 0 of the second workgroup)"""
    ctx = M.default_context()
    n = 257
    pts = _case(multiples, n)
    limbs, good = _limbs(pts), b"".join(_enc(P) for P in pts)
    x, y = multiples[300]
    flagged = bytearray(_enc((x, y)))
    flagged[95] |= 0xC0
    crafted = {  # name: (bytes of the last point, bits the checked decoder reports, bits the unchecked one reports, its point)
        "y + 1": (_enc((x, y + 1)), 2, 0, (x, y + 1)),
        "off the subgroup": (_enc(off_subgroup), 4, 0, off_subgroup),
        "x = q": (Q.to_bytes(48, "little") + y.to_bytes(48, "little"), 1, 1, None),
        "y = q": (x.to_bytes(48, "little") + Q.to_bytes(48, "little"), 1, 1, None),
        "flags 0xC0": (bytes(flagged), 1, 1, None),
    }
    assert y + 1 < Q
    for what, (enc, checked_bits, unchecked_bits, as_is) in crafted.items():
        data = good[:-96] + enc
        got, bad = ctx.selftest_g1_codec("decode", data, n)
        assert bad == checked_bits, what
        assert np.array_equal(got[:-1], limbs[:-1]), what  # the other lanes are not disturbed
        assert not got[-1].any(), what                     # a refused point reads as the identity
        got, bad = ctx.selftest_g1_codec("decode_unchecked", data, n)
        assert bad == unchecked_bits, what
        assert np.array_equal(got[:-1], limbs[:-1]), what
        assert np.array_equal(got[-1:], _limbs([as_is])), what  # taken as it is, or refused


# ------------------------------------------------------------------------------------------------ keys
GOLDEN_NAMES = ["manual_constraints", "synthetic_8", "random_sparse"]


@pytest.fixture(scope="module")
def keys(M, S, W):
    """name -> (cs, public inputs, pk, vk, compressed bytes, uncompressed bytes): every key is built and written once per module"""
    made, srss = {}, []

    def get(name):
        if name not in made:
            if name in GOLDEN_NAMES:
                sizes = golden("pk_bytes.json")[name]["srs"]
                cs = {"manual_constraints": lambda: W.manual_constraints_circuit(1, 1), "synthetic_8": lambda: W.synthetic_circuit(8, 3, 5),
                      "random_sparse": lambda: W.random_sparse_circuit(seed=20261002)}[name]()
                public = cs.instance[1:]
            else:  # 2^10 constraints: vectors of several workgroups with a ragged tail (3 * 2^10 + 3 powers, 2^10 - 1 shifted powers)
                n = 1 << 10
                cs, public = W.synthetic_r1cs(n, 3, 5)
                # "tailored": the shifted powers are the top of the powers; "double": an SRS of twice the degree, shifted powers
                # in a range (and an MSM table) of their own
                sizes = (n, n, n) if name == "2p10_tailored" else (2 * n, 2 * n, 2 * n)
            srs = M.generate_universal_srs(*sizes, M.generate_rand())
            pk, vk = M.generate_proving_and_verifying_keys(srs, cs)
            srss.append(srs)
            made[name] = (cs, public, pk, vk, S.serialize_proving_key(pk), S.serialize_proving_key(pk, uncompressed=True))
        return made[name]

    yield get
    for entry in made.values():
        entry[2].free()
    for srs in srss:
        srs.free()


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_uncompressed_proving_key_bytes_match_the_model(S, keys, name):
    cs, public, pk, vk, comp, unc = keys(name)
    want, want0 = golden("key_forms.json")[name], golden("pk_bytes.json")[name]
    assert unc[:64].hex() == want["pk"]["head"]
    assert len(unc) == want["pk"]["len"]
    assert hashlib.sha256(unc).hexdigest() == want["pk"]["sha256"]
    assert S.serialize_verifying_key(vk, uncompressed=True).hex() == want["vk_bytes"]
    assert unc.startswith(bytes.fromhex(want["vk_bytes"]))  # the vk's bytes open the proving key's
    # flags = 0 is swm_pk_serialize
    assert len(comp) == want0["len"] and hashlib.sha256(comp).hexdigest() == want0["sha256"]
    ctx = pk.ctx
    n = ctypes.c_size_t(0)
    assert ctx.lib.swm_pk_serialize(ctx.h, pk.h, None, 0, ctypes.byref(n)) == 0 and n.value == len(comp)
    buf = (ctypes.c_uint8 * n.value)()
    assert ctx.lib.swm_pk_serialize(ctx.h, pk.h, buf, n.value, ctypes.byref(n)) == 0 and bytes(buf) == comp


@pytest.mark.parametrize("name", GOLDEN_NAMES + ["2p10_tailored", "2p10_double"])
def test_uncompressed_bytes_load_into_the_same_key(M, S, keys, name):
    cs, public, pk, vk, comp, unc = keys(name)
    seed = bytes(range(32))
    p0 = M.generate_proof(cs, pk, M.rng_from_seed(seed))
    for unchecked in (False, True):
        pk2 = S.deserialize_proving_key(unc, uncompressed=True, unchecked=unchecked)
        assert pk2.refcount == 1
        assert S.serialize_proving_key(pk2) == comp
        assert S.serialize_proving_key(pk2, uncompressed=True) == unc
        p = M.generate_proof(cs, pk2, M.rng_from_seed(seed))
        assert p.data == p0.data
        assert M.verify_proof(vk, public, p, M.generate_rand())
        other = pk2.attach(pk2.ctx)  # a second holder, as for any key
        assert pk2.refcount == 2
        other.free()
        assert pk2.refcount == 1
        pk2.free()
        assert pk2.h is None
    # the flags = 0 reader through the new entry point is swm_pk_deserialize
    pk3 = S.deserialize_proving_key(comp, uncompressed=False)
    assert S.serialize_proving_key(pk3, uncompressed=True) == unc
    pk3.free()


def _rc(pk_ctx, data, flags):
    """return code of swm_pk_deserialize_ex; a key that loads is freed again"""
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(bytes(data))
    h = ctypes.c_void_p()
    rc = pk_ctx.lib.swm_pk_deserialize_ex(pk_ctx.h, buf, len(data), flags, ctypes.byref(h))
    if rc == 0:
        pk_ctx.lib.swm_pk_destroy(pk_ctx.h, h)
    return rc


def test_refusals(M, S, W, keys, off_subgroup):
    cs, public, pk, vk, comp, unc = keys("synthetic_8")
    ctx = pk.ctx
    assert _rc(ctx, unc, CHECKED) == 0 and _rc(ctx, unc, UNCHECKED) == 0
    for flags in (CHECKED, UNCHECKED):
        assert _rc(ctx, unc[:-5], flags) == ERR_SERIALIZATION
        assert _rc(ctx, unc[:len(unc) // 2], flags) == ERR_SERIALIZATION
        assert _rc(ctx, unc + b"\x00", flags) == ERR_SERIALIZATION
        assert _rc(ctx, comp, flags) == ERR_SERIALIZATION  # the compressed form is not the uncompressed one
    assert _rc(ctx, unc, 0) == ERR_SERIALIZATION
    # flags: unknown bits, UNCHECKED without UNCOMPRESSED, UNCHECKED on a writer
    for flags in (2, 4, 5, 7, 0x80000000):
        assert _rc(ctx, unc, flags) == ERR_INVALID_ARG, flags
    n = ctypes.c_size_t(0)
    for flags in (2, 3, 4, 5, 0x80000000):
        assert ctx.lib.swm_pk_serialize_ex(ctx.h, pk.h, flags, None, 0, ctypes.byref(n)) == ERR_INVALID_ARG, flags
    with pytest.raises(M.MarlinError) as e:
        S.deserialize_proving_key(comp, unchecked=True)
    assert e.value.code == ERR_INVALID_ARG
    # the committer key ends the bytes: ... powers | 1 | shifted | u64 3 | gamma (3) | 1 | bounds | max_degree
    pos = unc.rfind((3).to_bytes(8, "little"), 0, len(unc) - 3 * 96)
    assert pos > 0
    last = slice(pos - 96, pos)  # the last shifted power (not one the verifying key repeats: that is shifted[0] here)
    x, y = off_subgroup
    bad = bytearray(unc)
    bad[last] = x.to_bytes(48, "little") + y.to_bytes(48, "little")
    assert _rc(ctx, bad, CHECKED) == ERR_SERIALIZATION
    assert _rc(ctx, bad, UNCHECKED) == 0  # the caller's assertion is taken; load only, nothing is proved with it
    bad[last] = x.to_bytes(48, "little") + ((y + 1) % Q).to_bytes(48, "little")  # not even on the curve
    assert _rc(ctx, bad, CHECKED) == ERR_SERIALIZATION
    assert _rc(ctx, bad, UNCHECKED) == 0
    for coord in (0, 48):  # a coordinate >= q is no field element in any mode
        bad = bytearray(unc)
        bad[pos - 96 + coord:pos - 48 + coord] = Q.to_bytes(48, "little")
        assert _rc(ctx, bad, CHECKED) == ERR_SERIALIZATION
        assert _rc(ctx, bad, UNCHECKED) == ERR_SERIALIZATION
    bad = bytearray(unc)
    bad[pos - 1] |= 0xC0
    assert _rc(ctx, bad, CHECKED) == ERR_SERIALIZATION and _rc(ctx, bad, UNCHECKED) == ERR_SERIALIZATION
    # the verifying-key half of a key built for another SRS in front of this committer key: the halves disagree
    srs2 = M.generate_universal_srs(8, 8, 8, M.rng_from_seed(bytes([9] * 32)))
    pk2, vk2 = M.generate_proving_and_verifying_keys(srs2, cs)
    vkb, vkb2 = S.serialize_verifying_key(vk, uncompressed=True), S.serialize_verifying_key(vk2, uncompressed=True)
    assert len(vkb) == len(vkb2) and vkb != vkb2 and unc.startswith(vkb)
    mixed = vkb2 + unc[len(vkb):]
    assert _rc(ctx, mixed, CHECKED) == ERR_SERIALIZATION and _rc(ctx, mixed, UNCHECKED) == ERR_SERIALIZATION
    pk2.free()
    srs2.free()

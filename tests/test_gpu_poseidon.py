"""The Poseidon sponge on the GPU (csrc/poseidon.hip through the C ABI and simpleworks_amd/hash.py) against the committed fixture
tests/golden/poseidon.json, which tests/golden/gen_golden_poseidon.py writes from the big-integer model tests/poseidon_model.py.
Reference: src/hash/mod.rs:30-43 with the parameters of src/hash/helpers.rs (tests/golden/poseidon_params.json).
  * bytes: lengths on both sides of every chunk and rate boundary, batches around the wave (= workgroup) size and with a ragged
    last workgroup; every digest at its position;
  * elements: every absorb / squeeze shape up to a permutation inside the squeeze, host and device forms;
  * the lazy arithmetic's bounds: parameter sets of r - 1 throughout and of the identity matrix, inputs of r - 1, alpha from 2 to
    65535, no partial rounds, two full rounds — bit-exact against the model, the identity case against pow as well;
  * what the library must refuse, and how;
  * the mirror."""
import ctypes
import os

import numpy as np
import pytest

import poseidon_model as P
from oracle_lib import golden
from pyref.bls12_377 import R

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")
LENGTHS = [0, 11, 22, 23, 24, 54, 55, 85, 86, 300]
BATCHES = [1, 63, 64, 65, 257]


def le(h):
    return int.from_bytes(bytes.fromhex(h), "little")


def rows(values):
    """ints -> uint8 [len, 32]"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(len(values), 32).copy()


def ints(a):
    return [int.from_bytes(r.tobytes(), "little") for r in np.asarray(a).reshape(-1, 32)]


@pytest.fixture(scope="module")
def G():
    return golden("poseidon.json")


@pytest.fixture(scope="module")
def HASH():
    from simpleworks_amd import hash
    return hash


@pytest.fixture(scope="module")
def ref_params(HASH):
    return HASH.PoseidonParameters.from_json(PARAMS)


@pytest.fixture(scope="module")
def sponge(HASH, ref_params):
    s = HASH.PoseidonSponge(ref_params)
    yield s
    s.free()


@pytest.fixture(scope="module")
def expected(G):
    """Per length the digests of inputs 0 .. 256: the first 65 from the fixture, the rest from the model (computed once)."""
    ref = P.load_params(PARAMS)
    out = {}
    for ln in LENGTHS:
        have = [le(h) for h in G["bytes"][str(ln)]]
        out[ln] = [have[i] if i < len(have) else (have[0] if ln == 0 else P.hash_bytes(ref, P.poseidon_input(ln, i)))
                   for i in range(max(BATCHES))]
    return out


@pytest.mark.parametrize("batch", BATCHES)
def test_bytes_equal_the_fixture(sponge, expected, batch):
    for ln in LENGTHS:
        msgs = [P.poseidon_input(ln, i) for i in range(batch)]
        a = np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(batch, ln)
        got = ints(sponge.hash_many(a))
        assert got == expected[ln][:batch], ln
        if ln:   # (the empty input has one digest)
            assert len(set(msgs)) == batch and len(set(got)) == batch, ln


def test_hello_world_and_the_mirror(HASH, G, ref_params, sponge):
    want = le(G["bytes"]["11"][0])
    assert HASH.poseidon2_hash(b"Hello World", ref_params) == want
    assert ints(sponge.hash_many(np.frombuffer(b"Hello World", dtype=np.uint8).reshape(1, 11))) == [want]
    # bytes and elements meet: the packed elements of an input hash to its digest
    assert ints(sponge.hash_elements_many([HASH.poseidon_pack_bytes(b"Hello World")])) == [want]
    s = HASH.PoseidonSponge(ref_params)
    s.free()
    s.free()
    assert s.h is None


@pytest.mark.parametrize("n_out", [1, 2, 3])
def test_elements_equal_the_fixture(sponge, G, n_out):
    """n_in = 0 .. 5 over {0, 1, r - 1, random}; n_out = 3 permutes inside the squeeze.  Host and device forms agree."""
    ctx = sponge.ctx
    for n_in in range(6):
        cases = [c for c in G["elements"] if len(c["in"]) == n_in]
        assert cases
        count = len(cases)
        elems = rows([le(h) for c in cases for h in c["in"]]).reshape(count, n_in, 32)
        want = [le(h) for c in cases for h in c["out"][:n_out]]
        assert ints(sponge.hash_elements_many(elems, n_out)) == want, n_in
        d_in = ctx.alloc(max(elems.nbytes, 32)).upload(elems) if n_in else None
        d_out, d_st = ctx.alloc(count * n_out * 32), ctx.alloc(4 * count)
        d_st.upload(np.full(count, 7, dtype=np.uint32))
        ctx.poseidon_hash_fr_dev(sponge.h, d_in, n_in, count, n_out, d_out, d_st)
        ctx.synchronize()
        assert ints(d_out.download((count, n_out, 32), np.uint8)) == want, n_in
        assert not d_st.download((count,), np.uint32).any()
        for b in (d_in, d_out, d_st):
            if b:
                b.free()


def test_two_to_one_compressions_across_workgroups(sponge, G):
    """130 pairs: two full workgroups and a ragged third, every digest at its position; the device form without a status buffer."""
    want = [le(h) for h in G["compress"]]
    pairs = [P.poseidon_pair(i) for i in range(len(want))]
    assert ints(sponge.hash_elements_many(pairs)) == want
    assert ints(sponge.hash_elements_many(pairs[:65])) == want[:65]
    ctx = sponge.ctx
    elems = rows([v for p in pairs for v in p])
    d_in, d_out = ctx.alloc(elems.nbytes).upload(elems), ctx.alloc(32 * len(want))
    ctx.poseidon_hash_fr_dev(sponge.h, d_in, 2, len(want), 1, d_out, None)
    ctx.synchronize()
    assert ints(d_out.download((len(want), 32), np.uint8)) == want
    d_in.free()
    d_out.free()


def test_bytes_device_form(sponge, expected):
    ctx = sponge.ctx
    ln, batch = 55, 65
    a = np.frombuffer(b"".join(P.poseidon_input(ln, i) for i in range(batch)), dtype=np.uint8)
    d_in, d_out = ctx.alloc(a.nbytes).upload(a), ctx.alloc(32 * batch)
    ctx.poseidon_hash_bytes_dev(sponge.h, d_in, ln, batch, d_out)
    ctx.synchronize()
    assert ints(d_out.download((batch, 32), np.uint8)) == expected[ln][:batch]
    d_out.upload(np.zeros(32, dtype=np.uint8))
    ctx.poseidon_hash_bytes_dev(sponge.h, None, 0, 1, d_out)      # no input bytes: the pointer may be NULL
    ctx.synchronize()
    assert ints(d_out.download((1, 32), np.uint8)) == expected[0][:1]
    d_in.free()
    d_out.free()


def test_bounds_of_the_lazy_arithmetic(HASH, G):
    """Every parameter set of the fixture's adversarial list (fill r - 1 / identity / reference, alpha 2 .. 65535, with and without
    partial rounds, two and eight full rounds) over items of r - 1 and random values, three outputs each, bit-exact against the
    model; the identity sets against pow as well."""
    ref = P.load_params(PARAMS)
    items = [[le(h) for h in item] for item in G["adversarial_items"]]
    assert [R - 1, R - 1] in items and [R - 1] * 5 in items
    seen = set()
    for case in G["adversarial"]:
        full, partial, alpha, mds, ark = P.adversarial_params(case["fill"], case["full_rounds"], case["partial_rounds"], case["alpha"], ref)
        seen.add((case["fill"], full, partial, alpha))
        s = HASH.PoseidonSponge(HASH.PoseidonParameters(full, partial, alpha, mds, ark))
        try:
            for item, want in zip(items, case["out"]):
                assert ints(s.hash_elements_many([item], 3)) == [le(h) for h in want], (case["fill"], full, partial, alpha, len(item))
            if case["fill"] == "identity":
                x = R - 1
                assert ints(s.hash_elements_many([[x]], 1)) == [pow(x, alpha ** (full + partial), R)]
                x, y = P.fr("gpu power identity left"), P.fr("gpu power identity right")
                assert ints(s.hash_elements_many([[x, y]], 2)) == [pow(x, alpha ** (full + partial), R), pow(y, alpha ** full, R)]
        finally:
            s.free()
    for fill in ("r-1", "identity"):
        for alpha in (2, 3, 5, 17, 65535):
            assert {(fill, 8, 0, alpha), (fill, 2, 29, alpha), (fill, 2, 0, alpha), (fill, 8, 29, alpha)} <= seen


def test_host_form_refuses_a_non_canonical_element(sponge):
    ctx = sponge.ctx
    for bad in (R, (1 << 256) - 1):
        for n_in, pos in ((1, 0), (2, 1), (5, 4)):
            item = [P.fr("refusal %d" % k) for k in range(n_in)]
            elems = np.stack([rows(item), rows(item[:pos] + [bad] + item[pos + 1:]), rows(item)])
            out = np.full((3, 2, 32), 0x5A, dtype=np.uint8)
            with pytest.raises(Exception) as e:
                ctx.poseidon_hash_fr(sponge.h, elems, 2, out)
            assert e.value.code == INVALID_ARG
            assert (out == 0x5A).all(), "a refused call wrote to the output"


def test_device_form_reports_a_non_canonical_element_per_item(sponge):
    ctx = sponge.ctx
    ref = P.load_params(PARAMS)
    count, n_in, n_out = 70, 3, 3
    items = [[P.fr("status %d %d" % (i, k)) for k in range(n_in)] for i in range(count)]
    bad = {5: (0, R), 63: (2, (1 << 256) - 1), 64: (1, R), 69: (2, R + 1)}
    sent = [list(it) for it in items]
    for i, (pos, v) in bad.items():
        sent[i][pos] = v
    elems = rows([v for it in sent for v in it])
    d_in, d_out, d_st = ctx.alloc(elems.nbytes).upload(elems), ctx.alloc(count * n_out * 32), ctx.alloc(4 * count)
    d_out.upload(np.full(count * n_out * 32, 0x5A, dtype=np.uint8))
    d_st.upload(np.full(count, 7, dtype=np.uint32))
    ctx.poseidon_hash_fr_dev(sponge.h, d_in, n_in, count, n_out, d_out, d_st)
    ctx.synchronize()
    got = d_out.download((count, n_out, 32), np.uint8)
    status = d_st.download((count,), np.uint32)
    assert [int(s) for s in status] == [1 if i in bad else 0 for i in range(count)]
    for i in range(count):
        assert ints(got[i]) == ([0] * n_out if i in bad else P.hash_elements(ref, items[i], n_out)), i
    for b in (d_in, d_out, d_st):
        b.free()


def test_create_refuses_bad_parameters(HASH, ref_params):
    ctx = HASH.default_context()
    p = ref_params
    mds = b"".join(v.to_bytes(32, "little") for row in p.mds for v in row)
    ark = b"".join(v.to_bytes(32, "little") for row in p.ark for v in row)
    big = ark * 8

    def refused(full, partial, alpha, m=mds, a=None):
        a = big[:96 * (full + partial)] if a is None else a
        with pytest.raises(Exception) as e:
            ctx.poseidon_destroy(ctx.poseidon_create(full, partial, alpha, m, a))
        assert e.value.code == INVALID_ARG, (full, partial, alpha)

    refused(7, 29, 17)          # odd
    refused(0, 29, 17)          # < 2
    refused(1, 29, 17)
    refused(8, 248, 17)         # 256 rounds
    refused(200, 56, 17)
    refused(8, 29, 1)           # alpha < 2
    refused(8, 29, 0)
    refused(8, 29, 65536)       # alpha > 65535
    rbytes = R.to_bytes(32, "little")
    for i in (0, 8):            # a matrix entry equal to r, then one of 2^256 - 1
        refused(8, 29, 17, m=mds[:32 * i] + rbytes + mds[32 * i + 32:])
        refused(8, 29, 17, m=mds[:32 * i] + b"\xff" * 32 + mds[32 * i + 32:])
    for i in (0, 110):          # the same in the first and in the last round key
        refused(8, 29, 17, a=ark[:32 * i] + rbytes + ark[32 * i + 32:])
    h = ctx.poseidon_create(8, 247, 65535, mds, big[:96 * 255])      # the largest legal shape is accepted
    ctx.poseidon_destroy(h)


def test_shapes_the_hash_calls_refuse_and_count_zero(sponge):
    ctx = sponge.ctx
    lib = ctx.lib
    out = np.full((1, 17, 32), 0x5A, dtype=np.uint8)
    one = rows([1]).reshape(1, 1, 32)
    for n_out in (0, 17):
        assert lib.swm_poseidon_hash_fr(ctx.h, sponge.h, one.ctypes.data, 1, 1, n_out, out.ctypes.data) == INVALID_ARG
    assert lib.swm_poseidon_hash_fr(ctx.h, sponge.h, one.ctypes.data, 4097, 1, 1, out.ctypes.data) == INVALID_ARG
    assert lib.swm_poseidon_hash_bytes(ctx.h, sponge.h, one.ctypes.data, 65537, 1, out.ctypes.data) == INVALID_ARG
    assert lib.swm_poseidon_hash_fr(ctx.h, sponge.h, None, 1, 1, 1, out.ctypes.data) == INVALID_ARG
    assert lib.swm_poseidon_hash_fr(ctx.h, None, one.ctypes.data, 1, 1, 1, out.ctypes.data) == INVALID_ARG
    # count = 0: SWM_OK, nothing launched, nothing written, buffers may be NULL
    assert lib.swm_poseidon_hash_fr(ctx.h, sponge.h, None, 2, 0, 1, None) == 0
    assert lib.swm_poseidon_hash_fr_dev(ctx.h, sponge.h, None, 2, 0, 1, None, None) == 0
    assert lib.swm_poseidon_hash_bytes(ctx.h, sponge.h, None, 11, 0, None) == 0
    assert lib.swm_poseidon_hash_bytes_dev(ctx.h, sponge.h, None, 11, 0, None) == 0
    assert (out == 0x5A).all()
    assert sponge.hash_many(np.zeros((0, 11), dtype=np.uint8)).shape == (0, 32)
    # the context still works after the refusals
    assert ints(sponge.hash_elements_many([[1]])) == [P.hash_elements(P.load_params(PARAMS), [1], 1)[0]]

"""Native Schnorr signatures on the GPU (csrc/schnorr.hip through the C ABI and simpleworks_amd/schnorr.py) against the committed
fixture tests/golden/schnorr.json, which tests/golden/gen_golden_schnorr.py writes from the big-integer model tests/schnorr_model.py.
Reference: src/schnorr_signature/schnorr.rs:57-160, examples/schnorr-signature/main.rs:79-100.
  * keygen and sign byte-identical to the fixture at batch sizes around the wave and block size, message lengths around the hash's
    block boundaries, with and without salt;
  * verify accepts every fixture signature and rejects every one-bit change; results land at the right positions in batches that
    span many blocks and end in a ragged one;
  * swm_schnorr_commitments equals the model bit for bit on the edge cases of the scalar and curve arithmetic;
  * what the library must refuse, and how;
  * the mirror's round trip with the reference's own example messages."""
import numpy as np
import pytest

import schnorr_model as S
from oracle_lib import golden
from pyref import rng as pyrng
from pyref.pedersen import ED_SUBGROUP_ORDER as L

pytestmark = pytest.mark.gpu

INVALID_ARG = -1


def _rows(items, key):
    raw = [bytes.fromhex(it[key]) for it in items]
    return np.frombuffer(b"".join(raw), dtype=np.uint8).reshape(len(raw), -1).copy()


@pytest.fixture(scope="module")
def G():
    return golden("schnorr.json")


@pytest.fixture(scope="module")
def SCH():
    from simpleworks_amd import schnorr
    return schnorr


@pytest.fixture(scope="module")
def params(SCH, G):
    """(without salt, with the fixture's salt)"""
    plain, salted = SCH.Parameters(), SCH.Parameters(salt=bytes.fromhex(G["salt"]))
    yield plain, salted
    plain.free()
    salted.free()


@pytest.fixture(scope="module")
def valid(G):
    """The 64 signatures as arrays: salted flag, messages (byte strings), secrets, nonces, public keys, signatures."""
    v = G["valid"]
    return {"salted": np.array([it["salted"] for it in v]), "messages": [bytes.fromhex(it["message"]) for it in v],
            "secret": _rows(v, "secret"), "nonce": _rows(v, "nonce"), "public_key": _rows(v, "public_key"),
            "signature": _rows(v, "signature")}


def _flip(a, col, bit=0):
    b = a.copy()
    b[:, col] ^= np.uint8(1 << bit)
    return b


@pytest.mark.parametrize("batch", [1, 2, 63, 64, 65, 257])
def test_keygen_and_sign_equal_the_fixture(params, valid, G, batch):
    """Without salt the hash input is 128 + length bytes (a block boundary at lengths 0 and 64), with salt 160 + length."""
    for salted in (False, True):
        p = params[int(salted)]
        for ln in G["lengths"]:
            group = [i for i in range(64) if valid["salted"][i] == salted and len(valid["messages"][i]) == ln]
            assert group, (salted, ln)
            idx = np.array([group[j % len(group)] for j in range(batch)])
            pk = p.ctx.schnorr_keygen(p.h, valid["secret"][idx])
            assert np.array_equal(pk, valid["public_key"][idx]), (salted, ln)
            msgs = np.frombuffer(b"".join(valid["messages"][i] for i in idx), dtype=np.uint8).reshape(batch, ln)
            sig = p.ctx.schnorr_sign(p.h, valid["secret"][idx], pk, valid["nonce"][idx], msgs)
            assert np.array_equal(sig, valid["signature"][idx]), (salted, ln)


def test_verify_accepts_the_fixture_and_rejects_one_bit_changes(SCH, params, valid):
    salted = valid["salted"]
    pk, sig, msgs = valid["public_key"], valid["signature"], valid["messages"]
    for which in (0, 1):
        mine = salted == bool(which)
        ok = SCH.verify_many(params[which], pk, msgs, sig)
        assert np.array_equal(ok, mine), which       # every signature of this salt setting, none of the other
        sel = np.flatnonzero(mine)
        p, s, m = pk[sel], sig[sel], [msgs[i] for i in sel]
        assert SCH.verify_many(params[which], p, m, s).all()
        changed = [bytes([b[0] ^ 1]) + b[1:] if b else b for b in m]          # (the empty message has no bit to change)
        assert np.array_equal(SCH.verify_many(params[which], p, changed, s), np.array([len(b) == 0 for b in m]))
        changed = [b[:-1] + bytes([b[-1] ^ 0x80]) if b else b for b in m]
        assert np.array_equal(SCH.verify_many(params[which], p, changed, s), np.array([len(b) == 0 for b in m]))
        for col, bit in ((0, 0), (17, 3), (32, 0), (63, 7)):                 # the response, then the challenge
            assert not SCH.verify_many(params[which], p, m, _flip(s, col, bit)).any(), (col, bit)
        for col, bit in ((0, 0), (20, 5), (32, 0), (50, 2)):                 # x, then y
            assert not SCH.verify_many(params[which], _flip(p, col, bit), m, s).any(), (col, bit)


def _tampered_cycle(valid, members, count):
    """`count` signatures cycling through `members`, those at i % 7 == 3 with one challenge bit changed."""
    idx = np.array(members)[np.arange(count) % len(members)]
    sig = valid["signature"][idx]
    bad = np.arange(count) % 7 == 3
    sig[bad, 40] ^= np.uint8(4)
    return idx, sig, bad


@pytest.mark.parametrize("count", [5000, 70000])
def test_positions_in_a_mixed_batch(SCH, params, valid, count):
    """All 64 signatures cycled (seven message lengths, both salt settings): under each parameter set exactly the untampered
    signatures of its own salt setting verify, each at its own index."""
    idx, sig, bad = _tampered_cycle(valid, list(range(64)), count)
    msgs = [valid["messages"][i] for i in idx]
    for which in (0, 1):
        ok = SCH.verify_many(params[which], valid["public_key"][idx], msgs, sig)
        assert np.array_equal(ok, ~bad & (valid["salted"][idx] == bool(which))), which


def test_positions_in_one_launch_of_many_blocks(SCH, params, valid):
    """70 000 signatures of one message length in ONE launch: more blocks than compute units, and a ragged last block."""
    members = [i for i in range(64) if not valid["salted"][i] and len(valid["messages"][i]) == 65]
    idx, sig, bad = _tampered_cycle(valid, members, 70000)
    msgs = np.frombuffer(b"".join(valid["messages"][i] for i in idx), dtype=np.uint8).reshape(70000, 65)
    ok = SCH.verify_many(params[0], valid["public_key"][idx], msgs, sig)
    assert np.array_equal(ok, ~bad)


def test_commitments_equal_the_fixture_on_every_edge_case(params, G):
    cases = G["commitments"]
    assert len(cases) >= 40
    pk = _rows(cases, "public_key")
    sig = np.concatenate([_rows(cases, "response"), _rows(cases, "challenge")], axis=1)
    for p in params:                                   # the salt takes no part in the commitment
        got = p.ctx.schnorr_commitments(p.h, pk, sig)
        for i, c in enumerate(cases):
            assert got[i].tobytes().hex() == c["commitment"], c["note"]
    one = params[0].ctx.schnorr_commitments(params[0].h, pk[-1:], sig[-1:])          # a batch of one: -G, s = 1, e = l + 1
    assert one[0].tobytes() == S.point_bytes(S.IDENTITY)


def _le(v):
    return np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)


def test_refusals(SCH, params, valid):
    from simpleworks_amd import SwmError
    p = params[0]
    ctx = p.ctx
    with pytest.raises(SwmError) as e:                                         # (1, 1) is not on the curve
        SCH.Parameters(generator=(1, 1))
    assert e.value.code == INVALID_ARG
    with pytest.raises(SwmError) as e:                                         # x = r is not a field element
        SCH.Parameters(generator=(0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001, 1))
    assert e.value.code == INVALID_ARG

    sk, k, pk, sig = valid["secret"][:5].copy(), valid["nonce"][:5].copy(), valid["public_key"][:5].copy(), valid["signature"][:5].copy()
    msgs = np.zeros((5, 3), dtype=np.uint8)
    sentinel = np.full((5, 64), 0xA5, dtype=np.uint8)
    for bad_scalar in (L, L + 1, (1 << 256) - 1):
        bad_sk = sk.copy()
        bad_sk[3] = _le(bad_scalar)
        out = sentinel.copy()
        with pytest.raises(SwmError) as e:
            ctx.schnorr_keygen(p.h, bad_sk, out=out)
        assert e.value.code == INVALID_ARG and np.array_equal(out, sentinel)
        with pytest.raises(SwmError) as e:
            ctx.schnorr_sign(p.h, bad_sk, pk, k, msgs, out=out)
        assert e.value.code == INVALID_ARG and np.array_equal(out, sentinel)
        bad_k = k.copy()
        bad_k[0] = _le(bad_scalar)
        with pytest.raises(SwmError) as e:
            ctx.schnorr_sign(p.h, sk, pk, bad_k, msgs, out=out)
        assert e.value.code == INVALID_ARG and np.array_equal(out, sentinel)
    out = sentinel.copy()
    with pytest.raises(SwmError) as e:                                         # a public key off the curve
        ctx.schnorr_sign(p.h, sk, _flip(pk, 0)[:5], k, msgs, out=out)
    assert e.value.code == INVALID_ARG and np.array_equal(out, sentinel)
    ctx.schnorr_sign(p.h, sk, pk, k, msgs, out=out)                            # and the same call with good inputs writes
    assert not np.array_equal(out, sentinel)

    # verify: ok = 0, and the call succeeds.  s + l is the same residue as s, but no field element holds it
    v_pk, v_sig, v_msgs = valid["public_key"][::2][:6].copy(), valid["signature"][::2][:6].copy(), [valid["messages"][i] for i in range(0, 12, 2)]
    assert SCH.verify_many(p, v_pk, v_msgs, v_sig).all()
    big = v_sig.copy()
    big[2, :32] = _le(int.from_bytes(v_sig[2, :32].tobytes(), "little") + L)
    assert list(SCH.verify_many(p, v_pk, v_msgs, big)) == [True, True, False, True, True, True]
    off = v_pk.copy()
    off[4, 32] ^= 1                                                            # y changed: off the curve
    off[5, 32:] = _le(int.from_bytes(v_pk[5, 32:].tobytes(), "little") + 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001)
    assert list(SCH.verify_many(p, off, v_msgs, v_sig)) == [True, True, True, True, False, False]   # y + r: the same point, not canonical

    out = sentinel[:6].copy()
    for bad_pk, bad_sig in ((off, v_sig), (v_pk, big)):
        with pytest.raises(SwmError) as e:
            ctx.schnorr_commitments(p.h, bad_pk, bad_sig, out=out)
        assert e.value.code == INVALID_ARG and np.array_equal(out, sentinel[:6])

    # count = 0
    none32, none64 = np.zeros((0, 32), dtype=np.uint8), np.zeros((0, 64), dtype=np.uint8)
    assert ctx.schnorr_keygen(p.h, none32).shape == (0, 64)
    assert ctx.schnorr_sign(p.h, none32, none64, none32, np.zeros((0, 7), dtype=np.uint8)).shape == (0, 64)
    assert ctx.schnorr_verify(p.h, none64, np.zeros((0, 7), dtype=np.uint8), none64).shape == (0,)
    assert ctx.schnorr_commitments(p.h, none64, none64).shape == (0, 64)


def test_mirror_round_trip(SCH):
    """examples/schnorr-signature/main.rs:79-100: setup, keygen, sign b"hello world"; it verifies, b"goodbye world" does not.  The
    secret key and the nonce are the model's draws from the same stream, and the bytes are the model's."""
    from simpleworks_amd import marlin as M
    rng, py_rng = M.generate_rand(), pyrng.test_rng()
    params = SCH.setup(rng)
    assert params.salt is None and params.generator == S.GENERATOR
    pk, sk = SCH.keygen(params, rng)
    x = S.draw_scalar(py_rng)
    assert sk.secret_key == x and sk.public_key == pk == S.keygen(S.GENERATOR, x)
    sig = SCH.sign(params, sk, b"hello world", rng)
    assert sig.to_bytes() == S.sign(S.GENERATOR, None, x, pk, S.draw_scalar(py_rng), b"hello world")
    assert SCH.verify(params, pk, b"hello world", sig)
    assert not SCH.verify(params, pk, b"goodbye world", sig)
    # the batched forms: draws in order, one per key and one per signature; messages of several lengths in one call
    pks, sks = SCH.keygen_many(params, rng, 5)
    xs = [S.draw_scalar(py_rng) for _ in range(5)]
    assert [int.from_bytes(r.tobytes(), "little") for r in sks] == xs
    msgs = [b"", b"a", b"hello world", b"a", b"x" * 100]
    sigs = SCH.sign_many(params, sks, pks, msgs, rng)
    ks = [S.draw_scalar(py_rng) for _ in range(5)]
    assert sigs[2].tobytes() == S.sign(S.GENERATOR, None, xs[2], SCH.point_from_bytes(pks[2]), ks[2], msgs[2])
    assert SCH.verify_many(params, pks, msgs, sigs).all()
    assert list(SCH.verify_many(params, pks, msgs[1:] + msgs[:1], sigs)) == [False, False, False, False, False]
    params.free()

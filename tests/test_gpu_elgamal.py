"""ElGamal encryption on the GPU (csrc/elgamal.hip through the C ABI and simpleworks_amd/elgamal.py) against the committed fixture
tests/golden/elgamal.json, which tests/golden/gen_golden_elgamal.py writes from the big-integer model tests/elgamal_model.py.
Reference: tests/encrypt.rs:11-28 (ark-crypto-primitives 0.3, encryption/elgamal/mod.rs).
  * keygen, encrypt, encrypt_to and decrypt byte-identical to the fixture at batch sizes around the wave and block size;
  * the resident-key path gives the per-item path's bytes for every item;
  * every edge case of the scalar and curve arithmetic, bit for bit, on all three kernels;
  * decryptions land at the right positions in a batch that spans many blocks and ends in a ragged one, and in one that crosses
    the boundary between two launches of the ladder's kernels;
  * what the library must refuse, and how;
  * the mirror's round trip, draw for draw, with tests/encrypt.rs."""
import numpy as np
import pytest

import elgamal_model as E
from oracle_lib import golden
from pyref import rng as pyrng
from pyref.pedersen import ED_SUBGROUP_ORDER as L

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
R_MODULUS = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001
LADDER_CHUNK = 1 << 18          # csrc/ed_mul.cuh, ED_LADDER_CHUNK: items per launch of elgamal_encrypt / elgamal_decrypt


def _rows(items, *keys):
    raw = [b"".join(bytes.fromhex(it[k]) for k in keys) for it in items]
    return np.frombuffer(b"".join(raw), dtype=np.uint8).reshape(len(raw), -1).copy()


@pytest.fixture(scope="module")
def G():
    return golden("elgamal.json")


@pytest.fixture(scope="module")
def EG():
    from simpleworks_amd import elgamal
    return elgamal


@pytest.fixture(scope="module")
def params(EG, G):
    p = EG.Parameters(E.point_from_bytes(bytes.fromhex(G["generator"])))
    yield p
    p.free()


@pytest.fixture(scope="module")
def valid(G):
    """The 64 tuples as arrays; "ct_to_key0": the ciphertexts of the same (message, randomness) under tuple 0's public key."""
    v = G["valid"]
    return {"secret": _rows(v, "secret"), "public_key": _rows(v, "public_key"), "message": _rows(v, "message"),
            "randomness": _rows(v, "randomness"), "ct": _rows(v, "c1", "c2"), "ct_to_key0": _rows(v, "c1", "c2_to_key0")}


@pytest.fixture(scope="module")
def key0(EG, params, valid):
    k = EG.ResidentKey(E.point_from_bytes(valid["public_key"][0].tobytes()), params.ctx)
    yield k
    k.free()


@pytest.mark.parametrize("batch", [1, 2, 63, 64, 65, 257])
def test_all_four_equal_the_fixture(EG, params, valid, key0, batch):
    idx = np.arange(batch) % 64
    ctx = params.ctx
    assert np.array_equal(ctx.elgamal_keygen(params.h, valid["secret"][idx]), valid["public_key"][idx])
    ct = ctx.elgamal_encrypt(params.h, valid["public_key"][idx], valid["message"][idx], valid["randomness"][idx])
    assert np.array_equal(ct, valid["ct"][idx])
    to = ctx.elgamal_encrypt_to(params.h, key0.h, valid["message"][idx], valid["randomness"][idx])
    assert np.array_equal(to, valid["ct_to_key0"][idx])
    assert np.array_equal(ctx.elgamal_decrypt(valid["secret"][idx], valid["ct"][idx]), valid["message"][idx])
    # tuple 0's secret key opens everything that went to its public key
    assert np.array_equal(EG.decrypt_many(params, valid["secret"][0], valid["ct_to_key0"][idx]), valid["message"][idx])


def test_two_paths_one_answer(EG, params, valid):
    """For every item: encrypt_to under ResidentKey(pk) equals encrypt with that pk, over all 64 messages and scalars."""
    for i in range(64):
        key = EG.ResidentKey(E.point_from_bytes(valid["public_key"][i].tobytes()), params.ctx)
        pks = np.ascontiguousarray(np.broadcast_to(valid["public_key"][i], (64, 64)))
        per_item = EG.encrypt_many(params, pks, valid["message"], valid["randomness"])
        resident = EG.encrypt_many(params, key, valid["message"], valid["randomness"])
        key.free()
        assert np.array_equal(resident, per_item), i
        assert np.array_equal(per_item[i], valid["ct"][i])


def test_every_edge_case_on_all_three_kernels(EG, params, G):
    cases = G["edge"]
    assert len(cases) >= 40
    ctx = params.ctx
    k, p, m = _rows(cases, "scalar"), _rows(cases, "point"), _rows(cases, "message")
    ct, plain = _rows(cases, "c1", "c2"), _rows(cases, "plaintext")
    got = ctx.elgamal_encrypt(params.h, p, m, k)
    for i, c in enumerate(cases):
        assert got[i].tobytes() == ct[i].tobytes(), c["note"]
    got = ctx.elgamal_decrypt(k, np.concatenate([p, m], axis=1))
    for i, c in enumerate(cases):
        assert got[i].tobytes() == plain[i].tobytes(), c["note"]
    keys = {}                                                  # one resident key per distinct point: the same bytes are expected
    for i, c in enumerate(cases):
        keys.setdefault(c["point"], []).append(i)
    assert len(keys) >= 7
    for point, members in keys.items():
        key = EG.ResidentKey(E.point_from_bytes(bytes.fromhex(point)), ctx)
        got = ctx.elgamal_encrypt_to(params.h, key.h, m[members], k[members])
        key.free()
        for j, i in enumerate(members):
            assert got[j].tobytes() == ct[i].tobytes(), cases[i]["note"]
    # a batch of one on each kernel: the last case with c2 = the identity
    i = max(j for j, c in enumerate(cases) if c["c2"] == E.point_bytes(E.IDENTITY).hex())
    assert ctx.elgamal_encrypt(params.h, p[i:i + 1], m[i:i + 1], k[i:i + 1])[0, 64:].tobytes() == E.point_bytes(E.IDENTITY)
    key = EG.ResidentKey(E.point_from_bytes(p[i].tobytes()), ctx)
    assert ctx.elgamal_encrypt_to(params.h, key.h, m[i:i + 1], k[i:i + 1])[0].tobytes() == ct[i].tobytes()
    key.free()
    assert ctx.elgamal_decrypt(k[i:i + 1], np.concatenate([p[i:i + 1], m[i:i + 1]], axis=1))[0].tobytes() == plain[i].tobytes()


@pytest.fixture(scope="module")
def swapped_plain(valid):
    """What decrypt must return for tuple k's (secret, c1) with tuple k + 1's c2: c2' - sk c1 = message + c2' - c2 (two additions
    of the model, no scalar multiplication)."""
    from pyref.pedersen import ed_add
    pts = [[E.point_from_bytes(valid[key][k].tobytes()[off:off + 64]) for k in range(64)] for key, off in (("message", 0), ("ct", 64))]
    rows = [E.point_bytes(ed_add(ed_add(pts[0][k], pts[1][(k + 1) % 64]), E.ed_neg(pts[1][k]))) for k in range(64)]
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(64, 64)


def _swapped_cycle(valid, swapped_plain, count):
    """`count` (secret, ciphertext) pairs cycling through the fixture, every seventh (i % 7 == 3) with the next tuple's c2 ->
    (fixture indices, ciphertexts, the plaintext expected at every index)."""
    idx = np.arange(count) % 64
    ct, expect = valid["ct"][idx], valid["message"][idx]
    swapped = np.arange(count) % 7 == 3
    ct[swapped, 64:] = valid["ct"][(idx[swapped] + 1) % 64, 64:]
    expect[swapped] = swapped_plain[idx[swapped]]
    assert (expect[swapped] != valid["message"][idx[swapped]]).any(axis=1).all()
    return idx, ct, expect


def test_round_trip_and_positions_in_many_blocks(EG, params, valid, key0, swapped_plain):
    """70 000 items in one launch: more blocks than compute units, and a ragged last block."""
    count = 70000
    idx, ct, expect = _swapped_cycle(valid, swapped_plain, count)
    assert np.array_equal(params.ctx.elgamal_decrypt(valid["secret"][idx], ct), expect)
    # and what the GPU encrypts it decrypts, on both encrypt paths
    enc = params.ctx.elgamal_encrypt(params.h, valid["public_key"][idx], valid["message"][idx], valid["randomness"][idx])
    assert np.array_equal(enc, valid["ct"][idx])
    to = EG.encrypt_many(params, key0, valid["message"][idx], valid["randomness"][idx])
    assert np.array_equal(to, valid["ct_to_key0"][idx])
    assert np.array_equal(EG.decrypt_many(params, valid["secret"][0], to), valid["message"][idx])


def test_positions_across_the_launch_boundary(params, valid, swapped_plain):
    """elgamal_encrypt and elgamal_decrypt run in launches of LADDER_CHUNK items: one call of LADDER_CHUNK + 257 crosses the
    boundary; every item on both sides of it is checked."""
    count = LADDER_CHUNK + 257
    idx, ct, expect = _swapped_cycle(valid, swapped_plain, count)
    got = params.ctx.elgamal_decrypt(valid["secret"][idx], ct)
    assert np.array_equal(got[LADDER_CHUNK - 300:LADDER_CHUNK], expect[LADDER_CHUNK - 300:LADDER_CHUNK])   # the end of the first launch
    assert np.array_equal(got[LADDER_CHUNK:], expect[LADDER_CHUNK:])                                       # the whole second launch
    assert np.array_equal(got, expect)
    enc = params.ctx.elgamal_encrypt(params.h, valid["public_key"][idx], valid["message"][idx], valid["randomness"][idx])
    assert np.array_equal(enc, valid["ct"][idx])


def _le(v):
    return np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)


def test_refusals(EG, params, valid, key0):
    from simpleworks_amd import SwmError
    ctx = params.ctx
    for cls in (EG.Parameters, EG.ResidentKey):
        with pytest.raises(SwmError) as e:                                     # (1, 1) is not on the curve
            cls((1, 1))
        assert e.value.code == INVALID_ARG
        with pytest.raises(SwmError) as e:                                     # x = r is not a field element
            cls((R_MODULUS, 1))
        assert e.value.code == INVALID_ARG

    sk, pk, m, r, ct = (valid[k][:5].copy() for k in ("secret", "public_key", "message", "randomness", "ct"))

    def bad(a, col=None, scalar=None, plus_r=None):
        b = a.copy()
        if scalar is not None:
            b[3, :32] = _le(scalar)
        elif plus_r is not None:                                               # the same point, not canonical
            b[3, plus_r:plus_r + 32] = _le(int.from_bytes(a[3, plus_r:plus_r + 32].tobytes(), "little") + R_MODULUS)
        else:
            b[3, col] ^= 1                                                     # off the curve
        return b

    calls = {
        "keygen": (64, lambda out, sk=sk: ctx.elgamal_keygen(params.h, sk, out=out)),
        "encrypt": (128, lambda out, pk=pk, m=m, r=r: ctx.elgamal_encrypt(params.h, pk, m, r, out=out)),
        "encrypt_to": (128, lambda out, m=m, r=r: ctx.elgamal_encrypt_to(params.h, key0.h, m, r, out=out)),
        "decrypt": (64, lambda out, sk=sk, ct=ct: ctx.elgamal_decrypt(sk, ct, out=out)),
    }
    refused = []
    for s in (L, L + 1, (1 << 256) - 1):
        refused += [("keygen", {"sk": bad(sk, scalar=s)}), ("encrypt", {"r": bad(r, scalar=s)}), ("encrypt_to", {"r": bad(r, scalar=s)}),
                    ("decrypt", {"sk": bad(sk, scalar=s)})]
    refused += [("encrypt", {"pk": bad(pk, col=0)}), ("encrypt", {"pk": bad(pk, col=32)}), ("encrypt", {"m": bad(m, col=32)}),
                ("encrypt_to", {"m": bad(m, col=0)}), ("decrypt", {"ct": bad(ct, col=0)}), ("decrypt", {"ct": bad(ct, col=96)}),
                ("encrypt", {"pk": bad(pk, plus_r=32)}), ("encrypt", {"m": bad(m, plus_r=32)}), ("encrypt_to", {"m": bad(m, plus_r=32)}),
                ("decrypt", {"ct": bad(ct, plus_r=32)}), ("decrypt", {"ct": bad(ct, plus_r=96)})]
    for name, change in refused:
        width, call = calls[name]
        sentinel = np.full((5, width), 0xA5, dtype=np.uint8)
        out = sentinel.copy()
        with pytest.raises(SwmError) as e:
            call(out, **change)
        assert e.value.code == INVALID_ARG and np.array_equal(out, sentinel), (name, list(change))
        call(out)                                                              # and the same call with good inputs writes
        assert not (out == 0xA5).all(axis=1).any(), name

    none32, none64, none128 = (np.zeros((0, w), dtype=np.uint8) for w in (32, 64, 128))
    assert ctx.elgamal_keygen(params.h, none32).shape == (0, 64)
    assert ctx.elgamal_encrypt(params.h, none64, none64, none32).shape == (0, 128)
    assert ctx.elgamal_encrypt_to(params.h, key0.h, none64, none32).shape == (0, 128)
    assert ctx.elgamal_decrypt(none32, none128).shape == (0, 64)
    assert EG.encrypt_many(params, key0, none64, none32).shape == (0, 128) and EG.decrypt_many(params, none32, none128).shape == (0, 64)


def test_mirror_of_encrypt_rs(EG):
    """tests/encrypt.rs:13-27: setup, keygen, a random message, random r, encrypt, decrypt.  The generator, sk, message and r are
    the model's draws from the same stream, and the ciphertext bytes are the model's."""
    from simpleworks_amd import marlin as M
    rng, py_rng = M.generate_rand(), pyrng.test_rng()
    params = EG.setup(rng)
    gen = E.setup(py_rng)
    assert params.generator == gen
    pk, sk = EG.keygen(params, rng)
    m_pk, m_sk = E.keygen(gen, py_rng)
    assert (pk, sk.secret_key) == (m_pk, m_sk)
    msg, r = EG.rand_plaintext(rng), EG.rand_randomness(rng)
    assert (msg, r) == (E.rand_plaintext(py_rng), E.rand_randomness(py_rng))
    cipher = EG.encrypt(params, pk, msg, r)
    assert cipher == E.encrypt(gen, pk, msg, r)
    assert EG.decrypt(params, sk, cipher) == msg
    # the batched forms on five items, draws in order
    pks, sks = EG.keygen_many(params, rng, 5)
    xs = [E.draw_scalar(py_rng) for _ in range(5)]
    assert [int.from_bytes(s.tobytes(), "little") for s in sks] == xs
    msgs = [EG.rand_plaintext(rng) for _ in range(5)]
    rs = [EG.rand_randomness(rng) for _ in range(5)]
    assert msgs == [E.rand_plaintext(py_rng) for _ in range(5)] and rs == [E.rand_randomness(py_rng) for _ in range(5)]
    m_arr = np.frombuffer(b"".join(E.point_bytes(p) for p in msgs), dtype=np.uint8).reshape(5, 64)
    r_arr = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in rs), dtype=np.uint8).reshape(5, 32)
    cts = EG.encrypt_many(params, pks, m_arr, r_arr)
    assert cts[2].tobytes() == E.ciphertext_bytes(E.encrypt(gen, EG.point_from_bytes(pks[2]), msgs[2], rs[2]))
    assert np.array_equal(EG.decrypt_many(params, sks, cts), m_arr)
    key = EG.ResidentKey(EG.point_from_bytes(pks[4]), params.ctx)
    to = EG.encrypt_many(params, key, m_arr, r_arr)
    assert np.array_equal(to[4], cts[4])
    assert np.array_equal(EG.decrypt_many(params, EG.SecretKey(xs[4]), to), m_arr)
    key.free()
    params.free()

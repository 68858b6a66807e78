"""The Schnorr verification circuit's witness synthesised on the GPU (csrc/schnorr_witness.hip: swm_schnorr_witness,
swm_schnorr_witness_dev, swm_schnorr_prove) against its specification, workloads.build_schnorr_verification run on the CPU: exact
equality of the whole witness vector in Montgomery limbs, the per-item ok byte, the device form's refusals, and
generate_schnorr_proof against generate_proof on the builder's system, byte for byte.
The builder costs about a second per signature, so every test uses a handful and the module shares what it has built."""
import numpy as np
import pytest

import schnorr_model as S
from oracle_lib import golden

pytestmark = pytest.mark.gpu

R = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001


class _WitnessOnly:
    """The builder's vocabulary, keeping the assignment and dropping the rows."""

    def __init__(self):
        self.witness = []

    @staticmethod
    def one():
        return ("i", 0)

    def new_input_variable(self, value):
        raise AssertionError("the circuit has no public input")

    def new_witness_variable(self, value):
        self.witness.append(int(value) % R)
        return ("w", len(self.witness) - 1)

    def enforce_constraint(self, a, b, c):
        pass


@pytest.fixture(scope="module")
def M():
    from simpleworks_amd import marlin
    return marlin


@pytest.fixture(scope="module")
def W():
    from simpleworks_amd import workloads
    return workloads


@pytest.fixture(scope="module")
def SCH():
    from simpleworks_amd import schnorr
    return schnorr


@pytest.fixture(scope="module")
def G():
    return golden("schnorr.json")


@pytest.fixture(scope="module")
def params(SCH, G):
    """(without salt, with the fixture's salt)"""
    plain, salted = SCH.Parameters(), SCH.Parameters(salt=bytes.fromhex(G["salt"]))
    yield plain, salted
    plain.free()
    salted.free()


@pytest.fixture(scope="module")
def circuits(SCH, params):
    made = {}

    def get(msg_len, salted=False):
        if (msg_len, salted) not in made:
            made[msg_len, salted] = SCH.SchnorrCircuit(params[int(salted)], msg_len)
        return made[msg_len, salted]
    yield get
    for c in made.values():
        c.free()


@pytest.fixture(scope="module")
def oracle(M, W, G):
    """(salted, key bytes, message, signature) -> the builder's witness as Montgomery limbs; built once per input."""
    salt = bytes.fromhex(G["salt"])
    seen = {}

    def get(salted, key, msg, sig):
        k = (bool(salted), bytes(key), bytes(msg), bytes(sig))
        if k not in seen:
            cs = _WitnessOnly()
            pk = (int.from_bytes(k[1][:32], "little"), int.from_bytes(k[1][32:], "little"))
            W.build_schnorr_verification(cs, W.ED_GENERATOR, salt if salted else None, pk, k[2], k[3])
            seen[k] = M._to_mont_limbs(cs.witness)
        return seen[k]
    return get


def _valid(G, i):
    v = G["valid"][i]
    return v["salted"], bytes.fromhex(v["public_key"]), bytes.fromhex(v["message"]), bytes.fromhex(v["signature"])


def _check_batch(oracle, circuit, salted, items, want_ok):
    """items: (key, message, signature); the whole witness of each equals the builder's, ok is per item."""
    keys = np.frombuffer(b"".join(it[0] for it in items), dtype=np.uint8).reshape(-1, 64)
    sigs = np.frombuffer(b"".join(it[2] for it in items), dtype=np.uint8).reshape(-1, 64)
    witness, ok = circuit.witness_many(keys, [it[1] for it in items], sigs)
    assert witness.shape == (len(items), circuit.shape()[1], 4)
    for i, (key, msg, sig) in enumerate(items):
        want = oracle(salted, key, msg, sig)
        assert want.shape == witness[i].shape, i
        bad = np.nonzero((witness[i] != want).any(axis=1))[0]
        assert bad.size == 0, "item %d: %d witnesses differ, the first at %d" % (i, bad.size, bad[0])
    assert ok.tolist() == list(want_ok)
    return witness


@pytest.mark.parametrize("index,msg_len,salted", [(0, 0, False), (3, 1, True), (10, 65, False)])
def test_fixture_signatures_at_the_block_boundaries(G, oracle, circuits, index, msg_len, salted):
    """Unsalted, empty message: the hash input is exactly two full blocks — the finalisation flag falls on a full block, there is
    no padding and the counter is 128.  Salted, one byte: three blocks, the last 33 bytes long.  Unsalted, 65 bytes: 193 bytes, one
    past a boundary."""
    s, key, msg, sig = _valid(G, index)
    assert s == salted and len(msg) == msg_len
    _check_batch(oracle, circuits(msg_len, salted), salted, [(key, msg, sig)], [True])


def test_extremal_scalars_and_keys_in_one_launch(G, oracle, circuits):
    """None of these is a valid signature: ok = 0 everywhere, and every witness is still the builder's.  s = 0 keeps every
    fixed-base prefix at the identity; e = 0 keeps every accumulator there; the keys of order 1, 2 and 4 and the key outside the
    prime subgroup take the complete law through its degenerate points."""
    _, key, msg, sig = _valid(G, 0)
    s, e = sig[:32], sig[32:]
    notes = {c["note"].split(",")[0]: bytes.fromhex(c["public_key"]) for c in G["commitments"]}
    identity = (0).to_bytes(32, "little") + (1).to_bytes(32, "little")
    order2 = (0).to_bytes(32, "little") + (R - 1).to_bytes(32, "little")
    assert notes["key = identity"] == identity and notes["key = order 2"] == order2
    items = [(key, msg, bytes(32) + e), (key, msg, b"\xff" * 32 + e), (key, msg, s + bytes(32)), (key, msg, s + b"\xff" * 32),
             (identity, msg, sig), (order2, msg, sig), (notes["key = order 4"], msg, sig), (notes["key = G + a point of order 4"], msg, sig)]
    _check_batch(oracle, circuits(0), False, items, [False] * 8)


def test_batches_mix_valid_and_tampered(G, oracle, circuits):
    """ok is per item: a batch of 1, and a batch of 5 with the valid ones at both ends."""
    _, key, msg, sig = _valid(G, 0)
    _, key2, msg2, sig2 = _valid(G, 14)
    assert msg2 == b"" and key2 != key
    flip_e = sig[:40] + bytes([sig[40] ^ 0x10]) + sig[41:]
    flip_s = bytes([sig[0] ^ 1]) + sig[1:]
    c = circuits(0)
    _check_batch(oracle, c, False, [(key, msg, sig)], [True])
    _check_batch(oracle, c, False, [(key, msg, sig), (key, msg, flip_e), (key2, msg, sig), (key, msg, flip_s), (key2, msg2, sig2)],
                 [True, False, False, False, True])
    w0, ok0 = c.witness_many(np.zeros((0, 64), np.uint8), [], np.zeros((0, 64), np.uint8))   # nothing to launch
    assert w0.shape[0] == 0 and ok0.size == 0


@pytest.mark.parametrize("count,chunk", [(7, 3), (3, 1)])
def test_batch_across_a_chunk_seam(G, oracle, circuits, count, chunk):
    """The host form with its stage cap moved (swm_selftest_witness_stage): 7 items at a cap of 3 items' witness bytes + 5 go in
    chunks of 3, 3 and 1, 3 items at a cap one byte short of an item one by one.  The empty message; valid and tampered items on
    both sides of each seam, every witness the builder's and ok per item."""
    _, key, msg, sig = _valid(G, 0)
    _, key2, msg2, sig2 = _valid(G, 14)
    flip_e = sig[:40] + bytes([sig[40] ^ 0x10]) + sig[41:]
    flip_s = bytes([sig[0] ^ 1]) + sig[1:]
    items = [(key, msg, sig), (key, msg, flip_e), (key2, msg, sig), (key, msg, flip_s), (key2, msg2, sig2), _valid(G, 28)[1:],
             _valid(G, 42)[1:]][:count]
    assert not _valid(G, 28)[0] and not _valid(G, 42)[0] and _valid(G, 28)[2] == _valid(G, 42)[2] == b""
    c = circuits(0)
    item = 32 * c.shape()[1]
    with c.ctx.selftest_witness_stage(3 * item + 5 if chunk == 3 else item - 1):
        _check_batch(oracle, c, False, items, [True, False, False, False, True, True, True][:count])


def test_device_form_with_an_off_curve_key_in_the_middle(G, oracle, circuits):
    from simpleworks_amd._lib import DeviceBuffer, SwmError
    c = circuits(0)
    ctx, nw = c.ctx, c.shape()[1]
    _, key, msg, sig = _valid(G, 0)
    _, key2, _, sig2 = _valid(G, 14)
    off_curve = key[:32] + (int.from_bytes(key[32:], "little") ^ 1).to_bytes(32, "little")
    assert S.point_from_bytes(off_curve) is None
    not_canonical = R.to_bytes(32, "little") + key[32:]
    for bad in (off_curve, not_canonical):
        keys = np.frombuffer(key + bad + key2, dtype=np.uint8)
        sigs = np.frombuffer(sig + sig + sig2, dtype=np.uint8)
        bufs = [DeviceBuffer(ctx, 256).upload(keys), DeviceBuffer(ctx, 256).upload(sigs), DeviceBuffer(ctx, 3 * nw * 32), DeviceBuffer(ctx, 256),
                DeviceBuffer(ctx, 256)]
        ctx.schnorr_witness_dev(c.h, bufs[0], None, bufs[1], 3, bufs[2], bufs[3], bufs[4])
        w, ok, status = bufs[2].download((3, nw, 4)), bufs[3].download((3,), np.uint8), bufs[4].download((3,), np.uint32)
        for b in bufs:
            b.free()
        assert status.tolist() == [0, 1, 0] and ok.tolist() == [1, 0, 1]
        assert not w[1].any()
        assert np.array_equal(w[0], oracle(False, key, b"", sig)) and np.array_equal(w[2], oracle(False, key2, b"", sig2))
        # the host form refuses the whole call
        with pytest.raises(SwmError) as e:
            c.witness_many(keys.reshape(3, 64), [b""] * 3, sigs.reshape(3, 64))
        assert e.value.code == -1 and "item 1" in str(e.value)


def test_create_refusals(SCH, params):
    from simpleworks_amd._lib import SwmError
    with pytest.raises(SwmError) as e:
        SCH.SchnorrCircuit(params[0], 65537)
    assert e.value.code == -1
    c = SCH.SchnorrCircuit(params[1], 65536)
    assert c.shape()[1] == 6649 + 8 * 65536 + 21472 * ((160 + 65536 + 63) // 64)
    c.free()


def test_the_ledgers_message_length_satisfies_the_matrices(M, W, SCH, params, circuits):
    """msg_len 24 (examples/simple-payments/transaction.rs:101-103): the GPU's witness under the builder's matrices
    (swm_r1cs_is_satisfied), and a tampered one is not satisfied."""
    secret, nonce = 0x1234567 ** 7 % S.L, 0x7654321 ** 7 % S.L
    msg = bytes(range(24))
    pk = S.keygen(S.GENERATOR, secret)
    sig = S.sign(S.GENERATOR, None, secret, pk, nonce, msg)
    key = S.point_bytes(pk)
    cs, public = W.schnorr_verification_circuit(W.ED_GENERATOR, None, pk, msg, sig)
    assert public == []
    c = circuits(24)
    assert c.shape() == (len(cs.instance), len(cs.witness), cs.num_constraints) == (1, 71257, 72240)
    tampered = sig[:63] + bytes([sig[63] ^ 0x80])
    witness, ok = c.witness_many(np.frombuffer(key * 2, dtype=np.uint8).reshape(2, 64), [msg, msg],
                                 np.frombuffer(sig + tampered, dtype=np.uint8).reshape(2, 64))
    assert ok.tolist() == [True, False]
    want = M._to_mont_limbs(cs.witness)
    bad = np.nonzero((witness[0] != want).any(axis=1))[0]
    assert bad.size == 0, "%d witnesses differ, the first at %d" % (bad.size, bad[0])
    packed = cs.pack()
    one = M._to_mont_limbs([1])
    assert M.PackedR1cs(one, witness[0], *packed.mats).is_satisfied()
    assert not M.PackedR1cs(one, witness[1], *packed.mats).is_satisfied()


def test_proof_equals_the_builders(M, W, SCH, G, params, circuits):
    """Indexed once at the smallest shape (empty message, no salt): generate_schnorr_proof is byte-identical to generate_proof on
    the builder's system with the same rng state and verifies with no public input; a tampered signature is unsatisfied (-5), a
    circuit of another message length does not match the key (-8); the uncompressed form recodes to the compressed bytes."""
    from simpleworks_amd import serialization as Ser
    _, key, msg, sig = _valid(G, 0)
    pk_point = S.point_from_bytes(key)
    circuit_obj = W.SimpleSchnorrSignatureVerification(W.ED_GENERATOR, None, pk_point, msg, sig)
    cs = M.MarlinInst._synthesize(circuit_obj)
    packed = cs.pack()
    nnz = max(int(m[0][-1]) for m in packed.mats)
    srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, M.generate_rand())
    pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
    srs.free()
    try:
        want = M.generate_proof(cs, pk, M.generate_rand())
        c = circuits(0)
        got = M.generate_schnorr_proof(pk, c, key, msg, sig, M.generate_rand())
        assert got == Ser.serialize_proof(want)
        assert M.verify_proof(vk, [], M.MarlinProof(got), M.generate_rand())
        tampered = sig[:32] + bytes([sig[32] ^ 1]) + sig[33:]
        with pytest.raises(M.MarlinError) as e:
            M.generate_schnorr_proof(pk, c, key, msg, tampered, M.generate_rand())
        assert e.value.code == -5
        _, key1, msg1, sig1 = _valid(G, 2)
        with pytest.raises(M.MarlinError) as e:
            M.generate_schnorr_proof(pk, circuits(1), key1, msg1, sig1, M.generate_rand())
        assert e.value.code == -8
        raw = M.generate_schnorr_proof(pk, c, key, msg, sig, M.generate_rand(), uncompressed=True)
        assert len(raw) > len(got)
        assert Ser.proof_recode(raw, False) == got
        # the prover is as it was for the next caller: the device source does not outlive the call
        assert Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand())) == got
    finally:
        pk.free()

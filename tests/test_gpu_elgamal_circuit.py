"""The ElGamal encryption circuit's witness synthesised on the GPU (csrc/elgamal_witness.hip: swm_elgamal_witness, _to, the two
device forms, swm_elgamal_prove, _to) against its specification, workloads.build_elgamal_encryption run on the CPU: exact equality
of the whole witness vector in Montgomery limbs, the ciphertext against the committed fixture tests/golden/elgamal.json and
against encrypt_many, the resident-key path against the per-item path word for word, the device form's refusals, and
generate_elgamal_proof against generate_proof on the builder's system, byte for byte.
The builder costs about a tenth of a second per item; the module shares what it has built."""
import numpy as np
import pytest

import elgamal_model as E
from oracle_lib import golden

pytestmark = pytest.mark.gpu

R = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001
L = 2111115437357092606062206234695386632838870926408408195193685246394721360383
NW = 5371


class _WitnessOnly:
    """The builder's vocabulary, keeping the assignment and dropping the rows."""

    def __init__(self):
        self.instance, self.witness = [1], []

    @staticmethod
    def one():
        return ("i", 0)

    def new_input_variable(self, value):
        self.instance.append(int(value) % R)
        return ("i", len(self.instance) - 1)

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
def EG():
    from simpleworks_amd import elgamal
    return elgamal


@pytest.fixture(scope="module")
def G():
    return golden("elgamal.json")


@pytest.fixture(scope="module")
def generator(G):
    return E.point_from_bytes(bytes.fromhex(G["generator"]))


@pytest.fixture(scope="module")
def params(EG, generator):
    p = EG.Parameters(generator)
    yield p
    p.free()


@pytest.fixture(scope="module")
def circuit(EG, params):
    c = EG.ElGamalCircuit(params)
    yield c
    c.free()


@pytest.fixture(scope="module")
def oracle(M, W, generator):
    """(key bytes, message bytes, randomness bytes) -> (the builder's witness as Montgomery limbs, its ciphertext bytes); built
    once per input."""
    seen = {}

    def get(key, msg, r):
        k = (bytes(key), bytes(msg), bytes(r))
        if k not in seen:
            cs = _WitnessOnly()
            public = W.build_elgamal_encryption(cs, generator, E.point_from_bytes(k[0]), E.point_from_bytes(k[1]), k[2])
            assert len(cs.witness) == NW
            seen[k] = (M._to_mont_limbs(cs.witness), b"".join(v.to_bytes(32, "little") for v in public[2:]))
        return seen[k]
    return get


def _valid(G, i):
    v = G["valid"][i]
    return bytes.fromhex(v["public_key"]), bytes.fromhex(v["message"]), bytes.fromhex(v["randomness"])


def _edge(G, note):
    for e in G["edge"]:
        if e["note"].startswith(note):
            return e
    raise KeyError(note)


def _arrays(items):
    """items: (key, message, randomness) -> three uint8 arrays."""
    return (np.frombuffer(b"".join(it[0] for it in items), dtype=np.uint8).reshape(-1, 64),
            np.frombuffer(b"".join(it[1] for it in items), dtype=np.uint8).reshape(-1, 64),
            np.frombuffer(b"".join(it[2] for it in items), dtype=np.uint8).reshape(-1, 32))


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: %d witnesses differ, the first at %d" % (what, bad.size, bad[0])


def _check_batch(oracle, circuit, items):
    """The whole witness and the ciphertext of each item equal the builder's.  Returns (witness, ciphertexts)."""
    witness, ct = circuit.witness_many(*_arrays(items))
    assert witness.shape == (len(items), NW, 4) and witness.dtype == np.uint64
    assert ct.shape == (len(items), 128) and ct.dtype == np.uint8
    for i, it in enumerate(items):
        want_w, want_ct = oracle(*it)
        _same(witness[i], want_w, "item %d" % i)
        assert ct[i].tobytes() == want_ct, i
    return witness, ct


@pytest.mark.parametrize("index", [0, 1, 2])
def test_valid_fixtures_one_item_each(EG, G, oracle, params, circuit, index):
    item = _valid(G, index)
    _, ct = _check_batch(oracle, circuit, [item])
    v = G["valid"][index]
    assert ct[0].tobytes() == bytes.fromhex(v["c1"] + v["c2"])
    assert np.array_equal(ct, EG.encrypt_many(params, *_arrays([item])))


def test_the_edge_list_in_one_launch(G, oracle, circuit):
    """All 43 edge tuples — r = 0, the identity, keys and messages of order 2 and 4 or outside the prime subgroup, c2 = identity —
    plus r = l and r = 2^256 - 1 (bits 251 .. 255 set, which no scalar below l exercises), on the per-item path."""
    assert len(G["edge"]) == 43
    items = [(bytes.fromhex(e["point"]), bytes.fromhex(e["message"]), bytes.fromhex(e["scalar"])) for e in G["edge"]]
    key, msg, _ = _valid(G, 0)
    items += [(key, msg, L.to_bytes(32, "little")), (key, msg, b"\xff" * 32)]
    _, ct = _check_batch(oracle, circuit, items)
    for i, e in enumerate(G["edge"]):
        assert ct[i].tobytes() == bytes.fromhex(e["c1"] + e["c2"]), e["note"]
    # r = l on a key of the prime subgroup: c1 is the identity and c2 the message
    assert ct[43].tobytes() == (0).to_bytes(32, "little") + (1).to_bytes(32, "little") + msg


@pytest.mark.parametrize("which", ["valid0", "outside", "identity"])
def test_resident_key_is_the_per_item_path_word_for_word(EG, G, oracle, params, circuit, which):
    key = {"valid0": _valid(G, 0)[0],
           "outside": bytes.fromhex(_edge(G, "point = a point outside the prime subgroup")["point"]),
           "identity": bytes.fromhex(_edge(G, "point = the identity")["point"])}[which]
    if which == "identity":
        assert key == (0).to_bytes(32, "little") + (1).to_bytes(32, "little")
    items = [(key,) + _valid(G, i)[1:] for i in range(5)]
    keys, msgs, rs = _arrays(items)
    resident = EG.ResidentKey(E.point_from_bytes(key), params.ctx)
    try:
        w_to, ct_to = circuit.witness_many(resident, msgs, rs)
    finally:
        resident.free()
    w, ct = circuit.witness_many(keys, msgs, rs)
    assert np.array_equal(w_to, w) and np.array_equal(ct_to, ct)
    _same(w_to[3], oracle(*items[3])[0], "item 3")
    if which == "valid0":
        for i in range(5):
            v = G["valid"][i]
            assert ct_to[i].tobytes() == bytes.fromhex(v["c1"] + v["c2_to_key0"]), i


def test_batches_of_0_1_and_5(EG, G, oracle, params, circuit):
    w0, ct0 = circuit.witness_many(np.zeros((0, 64), np.uint8), np.zeros((0, 64), np.uint8), np.zeros((0, 32), np.uint8))   # nothing to launch
    assert w0.shape == (0, NW, 4) and ct0.shape == (0, 128)
    resident = EG.ResidentKey(E.point_from_bytes(_valid(G, 0)[0]), params.ctx)
    try:
        w0, ct0 = circuit.witness_many(resident, np.zeros((0, 64), np.uint8), np.zeros((0, 32), np.uint8))
    finally:
        resident.free()
    assert w0.shape == (0, NW, 4) and ct0.shape == (0, 128)
    _check_batch(oracle, circuit, [_valid(G, 1)])
    _check_batch(oracle, circuit, [_valid(G, i) for i in (2, 0, 1, 0, 2)])


@pytest.mark.parametrize("resident", [False, True])
def test_a_batch_of_300_on_both_paths(EG, G, oracle, params, circuit, resident):
    """More workgroups than CUs.  Every ciphertext against encrypt_many, witnesses 0, 149 and 299 against the builder."""
    n = len(G["valid"])
    items = [_valid(G, i % n) for i in range(300)]
    if resident:
        key0 = _valid(G, 0)[0]
        items = [(key0,) + it[1:] for it in items]
    keys, msgs, rs = _arrays(items)
    if resident:
        rk = EG.ResidentKey(E.point_from_bytes(key0), params.ctx)
        try:
            witness, ct = circuit.witness_many(rk, msgs, rs)
            assert np.array_equal(ct, EG.encrypt_many(params, rk, msgs, rs))
        finally:
            rk.free()
    else:
        witness, ct = circuit.witness_many(keys, msgs, rs)
    assert np.array_equal(ct, EG.encrypt_many(params, keys, msgs, rs))
    for i in (0, 149, 299):
        want_w, want_ct = oracle(*items[i])
        _same(witness[i], want_w, "item %d" % i)
        assert ct[i].tobytes() == want_ct


@pytest.mark.parametrize("count,chunk", [(7, 3), (3, 1)])
def test_batch_across_a_chunk_seam(EG, G, oracle, params, circuit, count, chunk):
    """The host forms with their stage cap moved (swm_selftest_witness_stage): 7 items at a cap of 3 items' witness bytes + 5 go in
    chunks of 3, 3 and 1, 3 items at a cap one byte short of an item one by one (a cap below one item once meant no progress: this
    unit had no floor of one item).  Every witness and ciphertext the builder's; the resident key's path gives the same words."""
    items = [_valid(G, i % 3) for i in (2, 0, 1, 0, 2, 1, 0)][:count]
    cap = 3 * 32 * NW + 5 if chunk == 3 else 32 * NW - 1
    with circuit.ctx.selftest_witness_stage(cap):
        _check_batch(oracle, circuit, items)
        key0 = _valid(G, 0)[0]
        keys, msgs, rs = _arrays([(key0,) + it[1:] for it in items])
        resident = EG.ResidentKey(E.point_from_bytes(key0), params.ctx)
        try:
            w_to, ct_to = circuit.witness_many(resident, msgs, rs)
        finally:
            resident.free()
        w, ct = circuit.witness_many(keys, msgs, rs)
    assert np.array_equal(w_to, w) and np.array_equal(ct_to, ct)
    assert np.array_equal(ct, EG.encrypt_many(params, keys, msgs, rs))


def test_device_form_with_a_bad_item_in_the_middle(EG, G, oracle, params, circuit):
    from simpleworks_amd._lib import DeviceBuffer, SwmError
    ctx = circuit.ctx
    a, b = _valid(G, 0), _valid(G, 1)
    off_curve = a[0][:32] + (int.from_bytes(a[0][32:], "little") ^ 1).to_bytes(32, "little")
    assert E.point_from_bytes(off_curve) is None
    not_canonical = R.to_bytes(32, "little") + a[1][32:]
    key0 = EG.ResidentKey(E.point_from_bytes(a[0]), params.ctx)
    try:
        for bad_key, bad_msg in ((off_curve, a[1]), (a[0], not_canonical)):
            keys, msgs, rs = _arrays([a, (bad_key, bad_msg, a[2]), b])
            forms = [None] if bad_key != a[0] else [None, key0]   # a resident key is never a bad key
            for key in forms:
                bufs = [DeviceBuffer(ctx, 256).upload(keys.reshape(-1)), DeviceBuffer(ctx, 256).upload(msgs.reshape(-1)),
                        DeviceBuffer(ctx, 256).upload(rs.reshape(-1)), DeviceBuffer(ctx, 3 * NW * 32), DeviceBuffer(ctx, 384),
                        DeviceBuffer(ctx, 256)]
                ctx.elgamal_witness_dev(circuit.h, bufs[0], bufs[1], bufs[2], 3, bufs[3], bufs[4], bufs[5], key_handle=key.h if key else None)
                w, ct, status = bufs[3].download((3, NW, 4)), bufs[4].download((3, 128), np.uint8), bufs[5].download((3,), np.uint32)
                for buf in bufs:
                    buf.free()
                assert status.tolist() == [0, 1, 0]
                assert not w[1].any() and not ct[1].any()
                last = b if key is None else (a[0],) + b[1:]
                for i, it in ((0, a), (2, last)):
                    want_w, want_ct = oracle(*it)
                    assert np.array_equal(w[i], want_w) and ct[i].tobytes() == want_ct
                # the host form refuses the whole call
                with pytest.raises(SwmError) as e:
                    circuit.witness_many(key if key else keys, msgs, rs)
                assert e.value.code == -1 and "item 1" in str(e.value)
    finally:
        key0.free()


def test_the_witness_satisfies_the_builders_matrices(M, W, G, generator, circuit):
    key, msg, r = _valid(G, 1)
    cs, public = W.elgamal_encryption_circuit(generator, E.point_from_bytes(key), E.point_from_bytes(msg), r)
    assert circuit.shape() == (len(cs.instance), len(cs.witness), cs.num_constraints) == (7, NW, 5375)
    witness, ct = circuit.witness_many(*_arrays([(key, msg, r)]))
    packed = cs.pack()
    claimed = W.elgamal_public_inputs(key, ct[0].tobytes())
    assert claimed == public
    assert M.PackedR1cs(M._to_mont_limbs([1] + claimed), witness[0], *packed.mats).is_satisfied()
    claimed[5] = (claimed[5] + 1) % R   # c2.y
    assert not M.PackedR1cs(M._to_mont_limbs([1] + claimed), witness[0], *packed.mats).is_satisfied()


def test_proof_equals_the_builders(M, W, EG, G, generator, params, circuit):
    """Indexed once: generate_elgamal_proof is byte-identical to generate_proof on the builder's system with the same rng state,
    in both key forms; it verifies with elgamal_public_inputs(pk, ciphertext) and not with another item's ciphertext; two proofs
    of different messages verify in one batch; a key of another shape does not match (-8); the uncompressed form recodes to the
    compressed bytes; and the prover is as it was for the next caller."""
    from simpleworks_amd import serialization as Ser
    key, msg, r = _valid(G, 0)
    _, msg1, r1 = _valid(G, 1)
    pk_point = E.point_from_bytes(key)
    cs = M.MarlinInst._synthesize(W.ElGamalEncryption(generator, pk_point, E.point_from_bytes(msg), r))
    packed = cs.pack()
    nnz = max(int(m[0][-1]) for m in packed.mats)
    srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, M.generate_rand())
    pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
    other_cs = W.test_circuit(3, 5)
    other_pk, _ = M.MarlinInst.index_from_constraint_system(srs, other_cs.pack())
    srs.free()
    resident = EG.ResidentKey(pk_point, params.ctx)
    try:
        want = Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand()))
        got, ct = M.generate_elgamal_proof(pk, circuit, key, msg, r, M.generate_rand())
        assert got == want
        v = G["valid"][0]
        assert ct == bytes.fromhex(v["c1"] + v["c2"])
        got_to, ct_to = M.generate_elgamal_proof(pk, circuit, resident, E.point_from_bytes(msg), int.from_bytes(r, "little"), M.generate_rand())
        assert got_to == want and ct_to == ct
        public = W.elgamal_public_inputs(key, ct)
        assert public == cs.instance[1:]
        assert M.verify_proof(vk, public, M.MarlinProof(got), M.generate_rand())
        got1, ct1 = M.generate_elgamal_proof(pk, circuit, resident, msg1, r1, M.generate_rand())
        assert ct1 == bytes.fromhex(G["valid"][1]["c1"] + G["valid"][1]["c2_to_key0"]) and ct1 != ct
        assert not M.verify_proof(vk, W.elgamal_public_inputs(key, ct1), M.MarlinProof(got), M.generate_rand())
        both = [public, W.elgamal_public_inputs(key, ct1)]
        assert M.verify_proofs(vk, both, [got, got1], M.generate_rand(), ctx=params.ctx) is True
        assert M.verify_proofs(vk, both[::-1], [got, got1], M.generate_rand(), ctx=params.ctx) is False
        with pytest.raises(M.MarlinError) as e:
            M.generate_elgamal_proof(other_pk, circuit, key, msg, r, M.generate_rand())
        assert e.value.code == -8
        raw, ct_raw = M.generate_elgamal_proof(pk, circuit, key, msg, r, M.generate_rand(), uncompressed=True)
        assert len(raw) > len(got) and ct_raw == ct
        assert Ser.proof_recode(raw, False) == got
        # the prover is as it was for the next caller: the device source does not outlive the call
        assert Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand())) == got
    finally:
        resident.free()
        pk.free()
        other_pk.free()


def test_create_and_call_refusals(EG, G, params, circuit):
    from simpleworks_amd import schnorr
    foreign = schnorr.Parameters()
    try:
        with pytest.raises(ValueError):
            EG.ElGamalCircuit(foreign)   # Schnorr parameters are not ElGamal parameters
    finally:
        foreign.free()
    freed = EG.Parameters(E.point_from_bytes(bytes.fromhex(G["generator"])))
    freed.free()
    with pytest.raises(ValueError):
        EG.ElGamalCircuit(freed)
    keys, msgs, rs = _arrays([_valid(G, 0), _valid(G, 1)])
    with pytest.raises(ValueError):
        circuit.witness_many(keys, msgs[:1], rs)
    with pytest.raises(ValueError):
        circuit.witness_many(keys, msgs, rs[:1])
    with pytest.raises(ValueError):
        circuit.witness_many(keys[:1], msgs, rs)
    c = EG.ElGamalCircuit(params)
    c.free()
    c.free()   # twice is harmless
    with pytest.raises(ValueError):
        c.witness_many(keys, msgs, rs)

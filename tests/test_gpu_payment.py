"""The payment circuit's witness and proof entries (csrc/payment_witness.hip) and the ledger over a Poseidon account tree on the
GPU, against the circuit's specification workloads.build_payment run on the CPU over the payments of tests/payment_model.py: whole
witness vectors in Montgomery limbs from all three witness entries, the flag bytes against the fixture, every item of a batch of
65 (one past the record kernel's 64-lane workgroup) against the shared matrices by the library's own row check, proof bytes
against generate_proof on the builder's system.  Heights: 2 (one level, six id bits forced to zero), 4, 9 (all eight id bits are
directions)."""
import os

import numpy as np
import pytest

import payment_model as PM
import poseidon_model as P
import poseidon_tree_model as T
from oracle_lib import golden

pytestmark = pytest.mark.gpu

R = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001
PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")
SALT = bytes(range(32))


class _WitnessOnly:
    """The builder's vocabulary, keeping the assignment and dropping the rows."""

    def __init__(self):
        self.witness = []
        self.public = []

    @staticmethod
    def one():
        return ("i", 0)

    def new_input_variable(self, value):
        self.public.append(int(value) % R)
        return ("i", len(self.public))

    def new_witness_variable(self, value):
        self.witness.append(int(value) % R)
        return ("w", len(self.witness) - 1)

    def enforce_constraint(self, a, b, c):
        pass


def rows(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(len(values), 32).copy()


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: %d witnesses differ, the first at %d" % (what, bad.size, bad[0])


@pytest.fixture(scope="module")
def M():
    from simpleworks_amd import marlin
    return marlin


@pytest.fixture(scope="module")
def W():
    from simpleworks_amd import workloads
    return workloads


@pytest.fixture(scope="module")
def L():
    from simpleworks_amd import ledger
    return ledger


@pytest.fixture(scope="module")
def ref():
    return P.load_params(PARAMS)


@pytest.fixture(scope="module")
def ref_params():
    from simpleworks_amd import hash as H
    return H.PoseidonParameters.from_json(PARAMS)


@pytest.fixture(scope="module")
def sponge(ref_params):
    from simpleworks_amd import hash as H
    s = H.PoseidonSponge(ref_params)
    yield s
    s.free()


@pytest.fixture(scope="module")
def sig_params():
    from simpleworks_amd import schnorr
    made = {None: schnorr.Parameters(), SALT: schnorr.Parameters(salt=SALT)}
    yield made
    for p in made.values():
        p.free()


@pytest.fixture(scope="module")
def circuits(L, sig_params, sponge):
    made = {}

    def get(height, salt=None):
        if (height, salt) not in made:
            made[(height, salt)] = L.PaymentCircuit(sig_params[salt], sponge, height)
        return made[(height, salt)]
    yield get
    for c in made.values():
        c.free()


@pytest.fixture(scope="module")
def world(ref):
    """(height, salt) -> (the model's payments, the account leaves, the model tree's levels), made once."""
    seen = {}

    def get(height, salt=None):
        if (height, salt) not in seen:
            leaves, levels = PM.ledger(ref, height, salt)
            seen[(height, salt)] = (PM.payments(ref, height, salt), leaves, levels)
        return seen[(height, salt)]
    return get


@pytest.fixture(scope="module")
def device_trees(sponge, world):
    from simpleworks_amd import hash as H
    made = {}

    def get(height):
        if height not in made:
            _, leaves, levels = world(height)
            tree = H.PoseidonMerkleTree.blank(sponge, height, 72)
            tree.update_many(sorted(leaves), [leaves[i] for i in sorted(leaves)])
            assert tree.root() == levels[-1][0]
            made[height] = tree
        return made[height]
    yield get
    for t in made.values():
        t.free()


@pytest.fixture(scope="module")
def oracle(M, W, ref_params):
    """(height, salt, payment) -> (the builder's witness as Montgomery limbs, its public inputs); built once per payment."""
    seen = {}

    def get(height, salt, p):
        k = (height, salt, p["name"])
        if k not in seen:
            cs = _WitnessOnly()
            public = W.build_payment(cs, PM.S.GENERATOR, salt, ref_params, height, p["message"], p["signature"], p["sender_leaf"],
                                     p["sender_path"], p["recipient_leaf"], p["recipient_path"])
            assert public == cs.public == p["public"]
            seen[k] = (M._to_mont_limbs(cs.witness), public)
        return seen[k]
    return get


def _tuples(ps):
    return [(p["message"], p["signature"], p["sender_leaf"], p["recipient_leaf"]) for p in ps]


def _device_form(circuit, tree, ps, siblings=True):
    """swm_payment_witness_dev over fresh device buffers -> (witness, flags, status, sender roots, recipient roots)."""
    ctx, n, nw, levels = circuit.ctx, len(ps), circuit.shape()[1], circuit.height - 1
    col = lambda k, width: np.frombuffer(b"".join(t[k] for t in _tuples(ps)), dtype=np.uint8).reshape(n, width)
    bufs = [ctx.to_device(col(0, 10)), ctx.to_device(col(1, 64)), ctx.to_device(col(2, 72)), ctx.to_device(col(3, 72))]
    sib = [None, None]
    if siblings:
        sib = [ctx.to_device(np.stack([rows(p[k]) for p in ps])) for k in ("sender_path", "recipient_path")]
    fill = np.full((n, nw, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)      # what a refusal must leave alone
    d_w, d_flags, d_status = ctx.to_device(fill), ctx.alloc(max(64, n)), ctx.alloc(max(64, 4 * n))
    d_rs, d_rr = ctx.alloc(max(64, 32 * n)), ctx.alloc(max(64, 32 * n))
    try:
        ctx.payment_witness_dev(circuit.h, tree.h if tree is not None else None, bufs[0], bufs[1], bufs[2], bufs[3], sib[0], sib[1], n,
                                d_w, d_flags, d_status, d_rs, d_rr)
        return (d_w.download((n, nw, 4)), d_flags.download((n,), np.uint8), d_status.download((n,), np.uint32),
                d_rs.download((n, 32), np.uint8), d_rr.download((n, 32), np.uint8))
    finally:
        for b in bufs + [s for s in sib if s is not None] + [d_w, d_flags, d_status, d_rs, d_rr]:
            b.free()


@pytest.mark.parametrize("height,salt,names", [(2, None, ("to oneself", "overdraft to oneself")),
                                               (4, None, tuple(p[0] for p in PM.PAYMENTS)),
                                               (9, None, ("valid", "overdraft by 1", "blank recipient")),
                                               (4, SALT, ("valid", "balance 2^64 - 1"))])
def test_whole_witness_from_all_three_entries(M, ref, oracle, circuits, world, device_trees, height, salt, names):
    """Every witness of every payment equals the builder's assignment, from the no-tree form, from the resident tree word for
    word, and from the device form; the flag bytes are the model's and the walked roots the model tree's (a blank recipient's
    path leads elsewhere)."""
    payments, leaves, levels = world(height, salt)
    ps = [p for p in payments if p["name"] in names]
    assert len(ps) == len(names)
    c = circuits(height, salt)
    assert c.shape() == M.payment_circuit_shape(c.sponge.params, height, salt is not None)
    witness, flags, roots_s, roots_r = c.witness_many(_tuples(ps), [p["sender_path"] for p in ps], [p["recipient_path"] for p in ps])
    assert witness.shape == (len(ps), c.shape()[1], 4)
    assert list(flags) == [p["flag"] for p in ps]
    root = levels[-1][0]
    assert roots_s == [root] * len(ps)
    for p, got in zip(ps, roots_r):
        want = T.root_of(ref, p["recipient_leaf"], p["message"][1], p["recipient_path"]) if p["wrong"] == "recipient" else root
        assert got == want and (got != root) == (p["wrong"] == "recipient"), p["name"]
    for k, p in enumerate(ps):
        w, public = oracle(height, salt, p)
        _same(witness[k], w, p["name"])
        assert public[0] == root
    dev = _device_form(c, None, ps)
    assert np.array_equal(dev[0], witness) and list(dev[1]) == list(flags) and not dev[2].any()
    assert [int.from_bytes(r.tobytes(), "little") for r in dev[3]] == roots_s
    assert [int.from_bytes(r.tobytes(), "little") for r in dev[4]] == roots_r
    # the leaves, and so the tree, do not depend on the salt
    at, at_flags = c.witness_at(device_trees(height), _tuples(ps))
    assert np.array_equal(at_flags, flags)
    for k, p in enumerate(ps):
        if p["wrong"] != "recipient":      # the tree's running digests at a blank leaf are not those of the claimed leaf's walk
            assert np.array_equal(at[k], witness[k]), p["name"]
    dev_at = _device_form(c, device_trees(height), ps, siblings=False)
    assert np.array_equal(dev_at[0], at) and list(dev_at[1]) == list(flags) and not dev_at[2].any()


@pytest.mark.parametrize("count,chunk", [(7, 3), (3, 1)])
def test_witness_across_a_chunk_seam(oracle, circuits, world, device_trees, count, chunk):
    """Both host forms with their stage cap moved (swm_selftest_witness_stage): 7 payments at a cap of 3 payments' witness bytes + 5
    go in chunks of 3, 3 and 1, 3 payments at a cap one byte short of a payment one by one.  Height 2, whose two payments
    alternate through the batch, so that neighbours differ; witnesses, flags and roots are the one-chunk test's."""
    payments, leaves, levels = world(2)
    assert len(payments) == 2
    ps = [payments[k % 2] for k in range(count)]      # A B A | B A B | A: a chunk read or written at another chunk's base shows
    c = circuits(2)
    item = 32 * c.shape()[1]
    with c.ctx.selftest_witness_stage(3 * item + 5 if chunk == 3 else item - 1):
        witness, flags, roots_s, roots_r = c.witness_many(_tuples(ps), [p["sender_path"] for p in ps], [p["recipient_path"] for p in ps])
        at, at_flags = c.witness_at(device_trees(2), _tuples(ps))
    assert witness.shape == (count, c.shape()[1], 4) and list(flags) == [p["flag"] for p in ps] == list(at_flags)
    assert roots_s == [levels[-1][0]] * count == roots_r
    for k, p in enumerate(ps):
        _same(witness[k], oracle(2, None, p)[0], "item %d: %s" % (k, p["name"]))
    assert np.array_equal(at, witness)


@pytest.fixture(scope="module")
def system(M, W, ref_params, world):
    """The builder's system of the valid payment at height 4, packed once: its matrices serve every payment of that shape."""
    p = world(4)[0][0]
    cs, public = W.payment_circuit(ref_params, 4, p["message"], p["signature"], p["sender_leaf"], p["sender_path"], p["recipient_leaf"],
                                   p["recipient_path"])
    assert public == p["public"] and p["name"] == "valid"
    return cs, cs.pack()


# positions 0, 63 and 64 of the batch hold the three kinds of invalid payment; the rest cycle through the fixture
def _batch_order(n_payments):
    order = [(1 + k) % n_payments for k in range(65)]
    order[0], order[63], order[64] = 4, 5, 6
    return order


def test_batch_of_65(M, oracle, circuits, world, device_trees, system):
    payments = world(4)[0]
    G = golden("payment.json")
    assert [p["name"] for p in payments] == [g["name"] for g in G["payments"]]
    order = _batch_order(len(payments))
    ps = [payments[k] for k in order]
    assert [p["wrong"] for p in (ps[0], ps[63], ps[64])] == ["overdraft", "signature", "recipient"]
    c = circuits(4)
    witness, flags = c.witness_at(device_trees(4), _tuples(ps))
    assert list(flags) == [G["payments"][k]["flag"] for k in order]
    for k in (0, 63, 64):
        if ps[k]["wrong"] != "recipient":
            _same(witness[k], oracle(4, None, ps[k])[0], "item %d" % k)
    # the blank recipient's block holds the tree's digests, not its own walk's: everything before it is the builder's
    at = _recipient_at(c)
    _same(witness[64][:at], oracle(4, None, ps[64])[0][:at], "item 64 up to the recipient's block")
    cs, packed = system
    for k, p in enumerate(ps):
        item = M.PackedR1cs(M._to_mont_limbs([1] + p["public"]), witness[k], *packed.mats)
        assert item.is_satisfied(c.ctx) == (p["wrong"] is None), (k, p["name"])


def _recipient_at(circuit):
    from simpleworks_amd import workloads
    return workloads.payment_circuit_layout(circuit.sponge.params, circuit.height, circuit.sig_params.salt is not None)["recipient"]


def test_refusals(W, L, circuits, world, device_trees, sponge, sig_params):
    from simpleworks_amd._lib import SwmError
    payments, leaves, levels = world(4)
    valid = payments[0]
    c = circuits(4)
    lay = W.payment_circuit_layout(c.sponge.params, 4)
    s_end = lay["schnorr"]["num_witness"]

    def changed(**kw):
        q = dict(valid)
        q.update(kw)
        return q
    off_curve = changed(sender_leaf=bytes([valid["sender_leaf"][0] ^ 1]) + valid["sender_leaf"][1:])
    not_canonical = changed(sender_leaf=R.to_bytes(32, "little") + valid["sender_leaf"][32:])
    big_sibling = changed(recipient_path=valid["recipient_path"][:2] + [R])
    big_id = changed(message=bytes([1, 8]) + valid["message"][2:])
    # the host forms refuse the whole call and name the item
    for bad in (off_curve, not_canonical, big_sibling, big_id):
        ps = [valid, bad]
        with pytest.raises(SwmError) as e:
            c.witness_many(_tuples(ps), [p["sender_path"] for p in ps], [p["recipient_path"] for p in ps])
        assert e.value.code == -1 and "item 1" in str(e.value)
    for bad in (off_curve, big_id):
        with pytest.raises(SwmError) as e:
            c.witness_at(device_trees(4), _tuples([valid, bad]))
        assert e.value.code == -1 and "item 1" in str(e.value)
    with pytest.raises(SwmError) as e:          # a tree of another height
        c.witness_at(device_trees(2), _tuples([valid]))
    assert e.value.code == -1
    for height in (1, 10):
        with pytest.raises(SwmError):
            L.PaymentCircuit(sig_params[None], sponge, height)
    lib, ctx = c.ctx.lib, c.ctx
    assert lib.swm_payment_witness(ctx.h, c.h, None, None, None, None, None, None, 0, None, None, None, None) == 0
    assert lib.swm_payment_witness_at(ctx.h, c.h, device_trees(4).h, None, None, None, None, 0, None, None) == 0
    # the device form reports per item; the neighbours are the honest witnesses, and of a refused key only the Schnorr block is cleared
    ps = [valid, off_curve, valid, big_sibling, big_id, not_canonical, valid]
    w, flags, status, _, _ = _device_form(c, None, ps)
    assert list(status) == [0, 1, 0, 2, 4, 1, 0]
    honest = c.witness_many(_tuples([valid]), [valid["sender_path"]], [valid["recipient_path"]])[0][0]
    for k in (0, 2, 6):
        assert np.array_equal(w[k], honest), k
    assert list(flags[[0, 2, 6]]) == [3, 3, 3] and flags[1] & 1 == 0 and flags[5] & 1 == 0
    for k in (1, 5):
        assert not w[k][:s_end].any()
        assert np.array_equal(w[k][s_end:lay["sender"]], honest[s_end:lay["sender"]])                      # balance and diff bits
        assert np.array_equal(w[k][lay["recipient_bits"]:], honest[lay["recipient_bits"]:])                # the recipient's side
        assert not (w[k][lay["sender"]:lay["recipient_bits"]] == 0xA5A5A5A5A5A5A5A5).all(axis=1).any()      # the sender's block is written
    # an id of 8 in a tree of 8 leaves: the Schnorr block is that of the message as given, the recipient's block that of leaf 0
    assert np.array_equal(w[4][lay["sender"]:lay["recipient_bits"]], honest[lay["sender"]:lay["recipient_bits"]])
    assert w[4][lay["recipient"]].tolist() == [0, 0, 0, 0]      # index bit 0 of 8 & 7


@pytest.fixture(scope="module")
def keys(M, system):
    cs, packed = system
    nnz = max(int(m[0][-1]) for m in packed.mats)
    srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, M.generate_rand())
    pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
    srs.free()
    yield pk, vk
    pk.free()


def test_proof_equals_the_builders(M, circuits, world, device_trees, system, keys):
    """swm_payment_prove_at is byte-identical to generate_proof on the builder's system from the same rng state; the proof verifies
    with the four public inputs and with none of them changed; a wrong sender leaf, an overdraft and a bad signature are
    SWM_ERR_UNSATISFIED (-5)."""
    from simpleworks_amd import serialization as Ser
    payments = world(4)[0]
    p = payments[0]
    cs, packed = system
    pk, vk = keys
    c, tree = circuits(4), device_trees(4)
    want = Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand()))
    got = M.generate_payment_proof(pk, c, tree, p["message"], p["signature"], p["sender_leaf"], p["recipient_leaf"], M.generate_rand())
    assert got == want
    public = p["public"]
    assert M.verify_proof(vk, public, M.MarlinProof(got), M.generate_rand())
    for k in range(4):
        other = list(public)
        other[k] = (other[k] + 1) % R
        assert not M.verify_proof(vk, other, M.MarlinProof(got), M.generate_rand()), k
    wrong_leaf = p["sender_leaf"][:64] + (1001).to_bytes(8, "little")
    for q in (dict(p, sender_leaf=wrong_leaf), payments[4], payments[5], payments[6]):
        with pytest.raises(M.MarlinError) as e:
            M.generate_payment_proof(pk, c, tree, q["message"], q["signature"], q["sender_leaf"], q["recipient_leaf"], M.generate_rand())
        assert e.value.code == -5, q["name"]
    # the prover is as it was for the next caller: the device source does not outlive the call
    assert Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand())) == got


def test_block_of_proofs_equals_single_calls(M, circuits, world, device_trees, keys):
    payments = world(4)[0]
    pk, vk = keys
    c, tree = circuits(4), device_trees(4)
    # valid, overdraft, valid, bad signature, a recipient leaf that is not the tree's (flags 3, no proof: the block goes on), valid
    block = [payments[0], payments[4], payments[2], payments[5], payments[6], payments[7]]
    rng = M.generate_rand()
    proofs, flags = M.generate_payment_proofs(pk, c, tree, _tuples(block), rng)
    assert flags == [3, 1, 3, 2, 3, 3] and [pr is None for pr in proofs] == [False, True, False, True, True, False]
    rng = M.generate_rand()
    for q, proof in zip(block, proofs):
        if q["flag"] != 3:
            continue      # the block entry does not call the prover for these
        if q["wrong"] is None:
            single = M.generate_payment_proof(pk, c, tree, q["message"], q["signature"], q["sender_leaf"], q["recipient_leaf"], rng)
            assert proof == single, q["name"]
            assert M.verify_proof(vk, q["public"], M.MarlinProof(proof), M.generate_rand())
        else:
            with pytest.raises(M.MarlinError) as e:
                M.generate_payment_proof(pk, c, tree, q["message"], q["signature"], q["sender_leaf"], q["recipient_leaf"], rng)
            assert e.value.code == -5
    assert M.generate_payment_proofs(pk, c, tree, [], M.generate_rand()) == ([], [])


def test_block_of_proofs_across_chunk_seams(M, circuits, world, device_trees, keys):
    """swm_payment_prove_many_at with the stage cap one byte short of a payment (swm_selftest_witness_stage): every payment is a
    chunk of its own, and proofs and lengths are those of three single calls from the same rng state."""
    payments = world(4)[0]
    pk, _ = keys
    c, tree = circuits(4), device_trees(4)
    block = [payments[0], payments[2], payments[7]]
    assert pk.ctx is c.ctx      # the prover's context is the one whose cap moves
    with c.ctx.selftest_witness_stage(32 * c.shape()[1] - 1):
        proofs, flags = M.generate_payment_proofs(pk, c, tree, _tuples(block), M.generate_rand())
    assert flags == [3, 3, 3]
    rng = M.generate_rand()
    for q, proof in zip(block, proofs):
        single = M.generate_payment_proof(pk, c, tree, q["message"], q["signature"], q["sender_leaf"], q["recipient_leaf"], rng)
        assert proof == single and len(single) > 0, q["name"]


def test_ledger_over_a_poseidon_tree(M, L, ref_params):
    """Three accounts, a transfer: validate(prove=True) is true, the payment proof verifies against the root before the transfer
    and not against the root after it; validate_many(prove=True) equals validate one by one."""
    from simpleworks_amd import schnorr
    rng = M.generate_rand()
    pp = L.Parameters.sample(rng, poseidon=ref_params)
    state = L.State(16, pp, account_tree="poseidon")
    try:
        assert state.account_merkle_tree.height() == 4
        people = [state.sample_keys_and_register(pp, rng) for _ in range(3)]
        assert [p[0] for p in people] == [1, 2, 3]
        state.update_balance(1, 10)
        tx = L.Transaction.create(pp, 1, 2, 4, people[0][2], rng)
        root_before = state.root()
        proof, public = tx.prove_payment(pp, state, rng)
        assert public == [root_before, 1, 2, 4]
        vk = state.payment_keys(rng)[2]
        assert L.verify_payment(vk, public, proof, rng)
        assert tx.validate(pp, state, rng, prove=True) is True
        assert state.apply_transaction(pp, tx, rng, prove=False) is True
        assert state.root() != root_before
        assert not L.verify_payment(vk, [state.root()] + public[1:], proof, rng)
        assert L.verify_payment(vk, public, proof, rng)
        block = [L.Transaction.create(pp, 1, 2, 6, people[0][2], rng),       # all Alice has left
                 L.Transaction.create(pp, 1, 2, 7, people[0][2], rng),       # one more
                 L.Transaction.create(pp, 2, 3, 1, people[0][2], rng),       # not the sender's signature
                 L.Transaction.create(pp, 2, 9, 1, people[1][2], rng),       # no such recipient
                 L.Transaction.create(pp, 3, 3, 0, people[2][2], rng)]
        one_by_one = [t.validate(pp, state, rng, prove=True) for t in block]
        assert one_by_one == [True, False, False, False, True]
        assert L.validate_many(pp, state, block, rng, prove=True) == one_by_one
        assert L.validate_many(pp, state, block) == one_by_one
    finally:
        state.free()
        pp.free()


def test_a_pedersen_state_behaves_as_before(M, L, ref_params):
    rng = M.generate_rand()
    pp = L.Parameters.sample(rng, poseidon=ref_params)
    state = L.State(8, pp)
    try:
        assert state.account_tree == "pedersen" and type(state.account_merkle_tree).__name__ == "DeviceMerkleTree"
        a, b = state.sample_keys_and_register(pp, rng), state.sample_keys_and_register(pp, rng)
        state.update_balance(a[0], 3)
        tx = L.Transaction.create(pp, a[0], b[0], 3, a[2], rng)
        assert tx.validate(pp, state, rng, prove=False) is True
        # with proofs: the signature circuit's, as before — the block form and the single form
        over = L.Transaction.create(pp, a[0], b[0], 4, a[2], rng)
        assert L.validate_many(pp, state, [tx, over], rng, prove=True) == [True, False]
        assert tx.validate(pp, state, rng, prove=True) is True and state._payment_keys is None and state._proof_keys is not None
        with pytest.raises(ValueError):
            state.payment_keys(rng)
        with pytest.raises(ValueError):
            L.State(8, L.Parameters(pp.sig_params, pp.leaf_crh, pp.two_to_one_crh), account_tree="poseidon")
    finally:
        state.free()
        pp.free()

"""The Pedersen payment circuit's witness and proof entries (csrc/pedersen_payment_witness.hip) and the ledger over its default,
Pedersen, account tree on the GPU, against the circuit's specification workloads.build_pedersen_payment run on the CPU: whole
witness vectors in Montgomery limbs, element for element, from the sibling form, from the resident tree and from the device form
over a buffer pre-filled with 0xFF.  Heights 2 (one level), 3 and 9 (all eight id bits are directions), accounts at index 0 and at
2^L - 1 (all directions zero, all one), recipient leaves that put the 144-window leaf stage's set bits at its wave boundaries."""
import numpy as np
import pytest

import pedersen_payment_model as PM

pytestmark = pytest.mark.gpu

R = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001
SECRETS = (1234567, 1234584)       # the account at index 0, the account at the last leaf
BALANCES = (1000, 5)


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


def _ints(rows_):
    return [int.from_bytes(r.tobytes(), "little") for r in rows_]


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
def params(W):
    return W.MerkleParams()


@pytest.fixture(scope="module")
def crh(params):
    from simpleworks_amd import hash as H
    made = (H.PedersenCRH(params.leaf_gens), H.PedersenCRH(params.inner_gens))
    yield made
    for c in made:
        c.free()


@pytest.fixture(scope="module")
def sig_params():
    from simpleworks_amd import schnorr
    p = schnorr.Parameters()
    yield p
    p.free()


@pytest.fixture(scope="module")
def circuits(L, sig_params, crh):
    made = {}

    def get(height):
        if height not in made:
            made[height] = L.PedersenPaymentCircuit(sig_params, crh[0], crh[1], height)
        return made[height]
    yield get
    for c in made.values():
        c.free()


def _payment(tree, leaves, secret, sender, recipient, amount, **kw):
    """A payment whose two paths are the resident tree's."""
    return PM.payment(None, leaves, secret, sender, recipient, amount,
                      paths=(tree.root(), tree.generate_proof(sender), tree.generate_proof(recipient)), **kw)


@pytest.fixture(scope="module")
def world(crh):
    """height -> (the resident tree, its leaves by index): an account at index 0 and one at the last leaf, the others blank."""
    from simpleworks_amd import hash as H
    made = {}

    def get(height):
        if height not in made:
            last = (1 << (height - 1)) - 1
            leaves = {0: PM.leaf(SECRETS[0], BALANCES[0]), last: PM.leaf(SECRETS[1], BALANCES[1])}
            tree = H.DeviceMerkleTree.blank(crh[0], crh[1], height, 72)
            tree.update_many(sorted(leaves), [leaves[i] for i in sorted(leaves)])
            made[height] = (tree, leaves)
        return made[height]
    yield get
    for tree, _ in made.values():
        tree.free()


def _oracle(M, params, height, p, root=None):
    """The builder's witness as Montgomery limbs and its public inputs."""
    cs = _WitnessOnly()
    public = PM.build(params, height, p, root=root, cs=cs)[1]
    assert public == cs.public
    return M._to_mont_limbs(cs.witness), public


def _tuples(ps):
    return [(p["message"], p["signature"], p["sender_leaf"], p["recipient_leaf"]) for p in ps]


def _device_form(circuit, tree, ps, siblings=True):
    """swm_pedersen_payment_witness_dev over a witness buffer of 0xFF bytes -> (witness, flags, status, sender roots, recipient roots)."""
    ctx, n, nw = circuit.ctx, len(ps), circuit.shape()[1]
    col = lambda k, width: np.frombuffer(b"".join(t[k] for t in _tuples(ps)), dtype=np.uint8).reshape(n, width)
    bufs = [ctx.to_device(col(0, 10)), ctx.to_device(col(1, 64)), ctx.to_device(col(2, 72)), ctx.to_device(col(3, 72))]
    sib = [None, None]
    if siblings:
        sib = [ctx.to_device(np.stack([rows(p[k]) for p in ps])) for k in ("sender_path", "recipient_path")]
    fill = np.full((n, nw, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)      # no field element: an unwritten witness shows
    d_w, d_flags, d_status = ctx.to_device(fill), ctx.alloc(max(64, n)), ctx.alloc(max(64, 4 * n))
    d_rs, d_rr = ctx.alloc(max(64, 32 * n)), ctx.alloc(max(64, 32 * n))
    try:
        ctx.pedersen_payment_witness_dev(circuit.h, tree.h if tree is not None else None, bufs[0], bufs[1], bufs[2], bufs[3], sib[0], sib[1],
                                         n, d_w, d_flags, d_status, d_rs, d_rr)
        return (d_w.download((n, nw, 4)), d_flags.download((n,), np.uint8), d_status.download((n,), np.uint32),
                d_rs.download((n, 32), np.uint8), d_rr.download((n, 32), np.uint8))
    finally:
        for b in bufs + [s for s in sib if s is not None] + [d_w, d_flags, d_status, d_rs, d_rr]:
            b.free()


@pytest.mark.parametrize("height", [2, 3, 9])
def test_whole_witness_from_all_three_entries(M, params, circuits, world, height):
    """Index 0 pays the last leaf and the last leaf pays index 0: every witness of both equals the builder's assignment, from the
    sibling form, from the resident tree and from the device form in both ways; the walked roots are the tree's root."""
    tree, leaves = world(height)
    last = (1 << (height - 1)) - 1
    ps = [_payment(tree, leaves, SECRETS[0], 0, last, 300), _payment(tree, leaves, SECRETS[1], last, 0, 5)]
    c = circuits(height)
    assert c.shape() == M.pedersen_payment_circuit_shape(height)
    witness, flags, roots_s, roots_r = c.witness_many(_tuples(ps), [p["sender_path"] for p in ps], [p["recipient_path"] for p in ps])
    assert witness.shape == (2, c.shape()[1], 4) and list(flags) == [3, 3]
    root = tree.root()
    assert roots_s == [root, root] and roots_r == [root, root]
    for k, p in enumerate(ps):
        w, public = _oracle(M, params, height, p)
        assert public == [root] + p["public"][1:]
        _same(witness[k], w, "payment %d" % k)
    at, at_flags = c.witness_at(tree, _tuples(ps))
    assert np.array_equal(at, witness) and np.array_equal(at_flags, flags)
    dev = _device_form(c, None, ps)
    assert np.array_equal(dev[0], witness) and list(dev[1]) == [3, 3] and not dev[2].any()
    assert _ints(dev[3]) == roots_s and _ints(dev[4]) == roots_r
    dev_at = _device_form(c, tree, ps, siblings=False)
    assert np.array_equal(dev_at[0], witness) and list(dev_at[1]) == [3, 3] and not dev_at[2].any()


def _leaf_with(**byte_values):
    leaf = bytearray(72)
    for k, v in byte_values.items():
        leaf[int(k[1:])] = v
    return bytes(leaf)


# window w of the leaf hash is bits 4 w .. 4 w + 3: the low nibble of byte w / 2 for an even w, the high one for an odd w
EDGE_LEAVES = [("all 0x00", bytes(72)),
               ("all 0xFF", b"\xff" * 72),
               ("bit 575", _leaf_with(b71=0x80)),
               ("windows 63 | 64", _leaf_with(b31=0xF0, b32=0x0F)),
               ("windows 127 | 128", _leaf_with(b63=0xF0, b64=0x0F)),
               ("windows 143 and 0", _leaf_with(b71=0xF0, b0=0x0F))]


def test_recipient_leaves_at_the_edges_of_the_144_window_stage(M, params, circuits, crh):
    """The recipient's leaf is any 72 bytes.  Each edge leaf sits at index 3 of a tree of its own at height 3: the builder's witness,
    the sibling form and the form over the tree are equal element for element."""
    from simpleworks_amd import hash as H
    c = circuits(3)
    sender = PM.leaf(SECRETS[0], BALANCES[0])
    ps = []
    for name, edge in EDGE_LEAVES:
        leaves = {0: sender, 3: edge}
        tree = H.DeviceMerkleTree.new(crh[0], crh[1], [leaves.get(i, bytes(72)) for i in range(4)])
        try:
            p = _payment(tree, leaves, SECRETS[0], 0, 3, 7)
            w, public = _oracle(M, params, 3, p)
            assert public[0] == tree.root(), name
            at, flags = c.witness_at(tree, _tuples([p]))
            _same(at[0], w, name + " (resident tree)")
            assert list(flags) == [3]
            ps.append((p, w))
        finally:
            tree.free()
    # one sibling equal to r - 1, with the last edge leaf: the largest canonical digest, every one of its low 253 bits' rows
    p = dict(ps[-1][0])
    p["recipient_path"] = [R - 1, p["recipient_path"][1]]
    ps.append((p, _oracle(M, params, 3, p)[0]))
    witness, flags, _, _ = c.witness_many(_tuples([q for q, _ in ps]), [q["sender_path"] for q, _ in ps], [q["recipient_path"] for q, _ in ps])
    assert list(flags) == [3] * len(ps)
    for k, (_, w) in enumerate(ps):
        _same(witness[k], w, (EDGE_LEAVES + [("a sibling r - 1", None)])[k][0])


@pytest.mark.parametrize("count", [1, 2, 5])
def test_item_i_of_a_block_equals_the_single_call(circuits, world, count):
    """Blocks of 1, 2 and 5 payments through the device form over 0xFF bytes: no element is left unwritten and item i is the
    single call's witness, flags and status, with sibling arrays and with the resident tree."""
    tree, leaves = world(3)
    c = circuits(3)
    pool = [_payment(tree, leaves, SECRETS[0], 0, 3, 300), _payment(tree, leaves, SECRETS[1], 3, 0, 6),      # an overdraft
            _payment(tree, leaves, SECRETS[0], 0, 0, 1000), _payment(tree, leaves, SECRETS[1], 3, 3, 0),
            _payment(tree, leaves, SECRETS[0], 0, 3, 1, flip_signature=True)]
    ps = pool[:count]
    for with_tree in (False, True):
        block = _device_form(c, tree if with_tree else None, ps, siblings=not with_tree)
        assert not (block[0] == 0xFFFFFFFFFFFFFFFF).all(axis=2).any()
        for i, p in enumerate(ps):
            single = _device_form(c, tree if with_tree else None, [p], siblings=not with_tree)
            assert np.array_equal(block[0][i], single[0][0]), (with_tree, i)
            assert block[1][i] == single[1][0] == p["flag"] and block[2][i] == single[2][0] == 0
            if not with_tree:
                assert _ints(block[3][i:i + 1]) == _ints(single[3]) == [tree.root()] == _ints(block[4][i:i + 1])
    host, flags = c.witness_at(tree, _tuples(ps))
    assert np.array_equal(host, block[0]) and list(flags) == [p["flag"] for p in ps]


@pytest.fixture(scope="module")
def seam_pool(M, params, world):
    """Seven payments at height 2 with the builder's witness of each: valid both ways, to oneself, an amount of zero, a flipped
    signature, an overdraft."""
    tree, leaves = world(2)
    ps = [_payment(tree, leaves, SECRETS[0], 0, 1, 300), _payment(tree, leaves, SECRETS[1], 1, 0, 5),
          _payment(tree, leaves, SECRETS[0], 0, 0, 1000), _payment(tree, leaves, SECRETS[1], 1, 1, 0),
          _payment(tree, leaves, SECRETS[0], 0, 1, 1, flip_signature=True), _payment(tree, leaves, SECRETS[1], 1, 0, 6),
          _payment(tree, leaves, SECRETS[0], 0, 1, 7)]
    return [(p, _oracle(M, params, 2, p)[0]) for p in ps]


@pytest.mark.parametrize("count,chunk", [(7, 3), (3, 1)])
def test_witness_across_a_chunk_seam(circuits, world, seam_pool, count, chunk):
    """Both host forms with their stage cap moved (swm_selftest_witness_stage): 7 payments at a cap of 3 payments' witness bytes + 5
    go in chunks of 3, 3 and 1, 3 payments at a cap one byte short of a payment one by one.  Height 2; witnesses, flags and roots
    are what one chunk gives: the builder's, the model's, the tree's."""
    tree, _ = world(2)
    ps = [p for p, _ in seam_pool[:count]]
    c = circuits(2)
    item = 32 * c.shape()[1]
    with c.ctx.selftest_witness_stage(3 * item + 5 if chunk == 3 else item - 1):
        witness, flags, roots_s, roots_r = c.witness_many(_tuples(ps), [p["sender_path"] for p in ps], [p["recipient_path"] for p in ps])
        at, at_flags = c.witness_at(tree, _tuples(ps))
    assert witness.shape == (count, c.shape()[1], 4) and list(flags) == [p["flag"] for p in ps] == list(at_flags)
    assert [p["flag"] for p in seam_pool[4][0:1]] == [2] and seam_pool[5][0]["flag"] == 1
    assert roots_s == [tree.root()] * count == roots_r
    for k, (_, w) in enumerate(seam_pool[:count]):
        _same(witness[k], w, "payment %d" % k)
    assert np.array_equal(at, witness)


def test_refusals(W, L, circuits, world, crh, sig_params):
    from simpleworks_amd import hash as H
    from simpleworks_amd._lib import SwmError
    tree, leaves = world(3)
    c = circuits(3)
    lay = W.pedersen_payment_circuit_layout(3)
    s_end = lay["schnorr"]["num_witness"]
    valid = _payment(tree, leaves, SECRETS[0], 0, 3, 300)
    off_curve = dict(valid, sender_leaf=bytes([valid["sender_leaf"][0] ^ 1]) + valid["sender_leaf"][1:])
    big_sibling = dict(valid, recipient_path=[valid["recipient_path"][0], R])
    big_id = dict(valid, message=bytes([0, 4]) + valid["message"][2:])
    # the host form refuses the whole call and names the item
    for bad in (off_curve, big_sibling, big_id):
        ps = [valid, bad]
        with pytest.raises(SwmError) as e:
            c.witness_many(_tuples(ps), [p["sender_path"] for p in ps], [p["recipient_path"] for p in ps])
        assert e.value.code == -1 and "item 1" in str(e.value)
    for bad in (off_curve, big_id):
        with pytest.raises(SwmError) as e:
            c.witness_at(tree, _tuples([valid, bad]))
        assert e.value.code == -1 and "item 1" in str(e.value)
    # a tree of another height, of another leaf length, of other parameters
    other = H.DeviceMerkleTree.blank(crh[0], crh[1], 3, 64)
    swapped = H.DeviceMerkleTree.blank(crh[0], crh[0], 3, 72)
    try:
        for t in (world(2)[0], other, swapped):
            with pytest.raises(SwmError) as e:
                c.witness_at(t, _tuples([valid]))
            assert e.value.code == -1
    finally:
        other.free()
        swapped.free()
    for height in (1, 10):
        with pytest.raises(SwmError):
            L.PedersenPaymentCircuit(sig_params, crh[0], crh[1], height)
    with pytest.raises(SwmError):       # a two-to-one CRH as the leaf CRH: 128 windows do not hold 72 bytes
        L.PedersenPaymentCircuit(sig_params, crh[1], crh[1], 3)
    # count = 0 launches nothing
    lib, ctx = c.ctx.lib, c.ctx
    assert lib.swm_pedersen_payment_witness(ctx.h, c.h, None, None, None, None, None, None, 0, None, None, None, None) == 0
    assert lib.swm_pedersen_payment_witness_at(ctx.h, c.h, tree.h, None, None, None, None, 0, None, None) == 0
    # the device form reports per item as the Poseidon payment does; the neighbours are the honest witnesses
    ps = [valid, off_curve, valid, big_sibling, big_id]
    w, flags, status, _, _ = _device_form(c, None, ps)
    assert list(status) == [0, 1, 0, 2, 4]
    honest = c.witness_many(_tuples([valid]), [valid["sender_path"]], [valid["recipient_path"]])[0][0]
    for k in (0, 2):
        assert np.array_equal(w[k], honest), k
    assert list(flags[[0, 2]]) == [3, 3] and flags[1] & 1 == 0
    assert not w[1][:s_end].any()                                                  # of a refused key only the Schnorr block is cleared
    assert np.array_equal(w[1][s_end:lay["sender"]], honest[s_end:lay["sender"]])
    assert np.array_equal(w[1][lay["recipient_bits"]:], honest[lay["recipient_bits"]:])
    assert not (w[1][lay["sender"]:lay["recipient_bits"]] == 0xFFFFFFFFFFFFFFFF).all(axis=1).any()
    # an id of 4 in a tree of 4 leaves: the recipient's section is that of leaf 0
    assert np.array_equal(w[4][lay["sender"]:lay["recipient_bits"]], honest[lay["sender"]:lay["recipient_bits"]])
    assert w[4][lay["recipient"] + W.PEDERSEN_PAYMENT_LEAF_WITNESSES].tolist() == [0, 0, 0, 0]      # the direction of level 0


@pytest.fixture(scope="module")
def system(W, params, world):
    """The builder's system of the valid payment at height 3, packed once: its matrices serve every payment of that shape."""
    tree, leaves = world(3)
    p = _payment(tree, leaves, SECRETS[0], 0, 3, 300)
    cs, public = PM.build(params, 3, p)
    assert public == [tree.root(), 0, 3, 300]
    return p, cs, cs.pack()


@pytest.fixture(scope="module")
def keys(M, system):
    _, cs, packed = system
    nnz = max(int(m[0][-1]) for m in packed.mats)
    srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, M.generate_rand())
    pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
    srs.free()
    yield pk, vk
    pk.free()


def test_proof_at_height_3(M, circuits, world, system, keys):
    """A valid payment's system is satisfied and its proof verifies with [root, sender, recipient, amount], not with another root
    or amount; a bad signature, an overdraft and a foreign leaf are SWM_ERR_UNSATISFIED (-5)."""
    tree, leaves = world(3)
    p, cs, packed = system
    pk, vk = keys
    c = circuits(3)
    witness, flags = c.witness_at(tree, _tuples([p]))
    assert list(flags) == [3]
    assert M.PackedR1cs(M._to_mont_limbs([1] + p["public"]), witness[0], *packed.mats).is_satisfied(c.ctx)
    proof = M.generate_pedersen_payment_proof(pk, c, tree, p["message"], p["signature"], p["sender_leaf"], p["recipient_leaf"],
                                              M.generate_rand())
    public = [tree.root(), 0, 3, 300]
    assert M.verify_proof(vk, public, M.MarlinProof(proof), M.generate_rand())
    assert not M.verify_proof(vk, [(public[0] + 1) % R] + public[1:], M.MarlinProof(proof), M.generate_rand())
    assert not M.verify_proof(vk, public[:3] + [301], M.MarlinProof(proof), M.generate_rand())
    foreign = dict(p, recipient_leaf=p["recipient_leaf"][:64] + (6).to_bytes(8, "little"))
    for q in (_payment(tree, leaves, SECRETS[0], 0, 3, 300, flip_signature=True), _payment(tree, leaves, SECRETS[0], 0, 3, 1001), foreign):
        with pytest.raises(M.MarlinError) as e:
            M.generate_pedersen_payment_proof(pk, c, tree, q["message"], q["signature"], q["sender_leaf"], q["recipient_leaf"],
                                              M.generate_rand())
        assert e.value.code == -5
    # a foreign leaf's honest witness: the leaf hash is satisfied, the system is not
    w, flags = c.witness_at(tree, _tuples([foreign]))
    assert list(flags) == [3]
    assert not M.PackedR1cs(M._to_mont_limbs([1] + p["public"]), w[0], *packed.mats).is_satisfied(c.ctx)


def test_block_of_proofs_goes_on_after_each_failure(M, circuits, world, system, keys):
    tree, leaves = world(3)
    p = system[0]
    pk, vk = keys
    c = circuits(3)
    foreign = dict(p, sender_leaf=p["sender_leaf"][:64] + (1001).to_bytes(8, "little"))
    block = [p, _payment(tree, leaves, SECRETS[1], 3, 0, 6), foreign, _payment(tree, leaves, SECRETS[1], 3, 0, 5)]
    proofs, flags = M.generate_pedersen_payment_proofs(pk, c, tree, _tuples(block), M.generate_rand())
    assert flags == [3, 1, 3, 3] and [pr is None for pr in proofs] == [False, True, True, False]
    root = tree.root()
    assert M.verify_proof(vk, [root, 0, 3, 300], M.MarlinProof(proofs[0]), M.generate_rand())
    assert M.verify_proof(vk, [root, 3, 0, 5], M.MarlinProof(proofs[3]), M.generate_rand())
    assert not M.verify_proof(vk, [root, 0, 3, 300], M.MarlinProof(proofs[3]), M.generate_rand())
    assert M.generate_pedersen_payment_proofs(pk, c, tree, [], M.generate_rand()) == ([], [])


def test_block_of_proofs_across_chunk_seams(M, circuits, world, system, keys):
    """swm_pedersen_payment_prove_many_at with the stage cap one byte short of a payment (swm_selftest_witness_stage): every
    payment is a chunk of its own, and proofs and lengths are those of three single calls from the same rng state."""
    tree, leaves = world(3)
    pk, _ = keys
    c = circuits(3)
    block = [system[0], _payment(tree, leaves, SECRETS[1], 3, 0, 5), _payment(tree, leaves, SECRETS[0], 0, 0, 1000)]
    assert pk.ctx is c.ctx      # the prover's context is the one whose cap moves
    with c.ctx.selftest_witness_stage(32 * c.shape()[1] - 1):
        proofs, flags = M.generate_pedersen_payment_proofs(pk, c, tree, _tuples(block), M.generate_rand())
    assert flags == [3, 3, 3]
    rng = M.generate_rand()
    for q, proof in zip(block, proofs):
        single = M.generate_pedersen_payment_proof(pk, c, tree, q["message"], q["signature"], q["sender_leaf"], q["recipient_leaf"], rng)
        assert proof == single and len(single) > 0


def test_ledger_over_its_default_pedersen_tree(M, L):
    """State(16, pp): three accounts, one with a balance.  The payment proof verifies against the root before the transfer and not
    against the root after it; the block form proves exactly the valid transactions; the Poseidon form's keys stay refused."""
    from simpleworks_amd import hash as H
    rng = M.generate_rand()
    pp = L.Parameters.sample(rng)
    state = L.State(16, pp)
    try:
        assert state.account_tree == "pedersen" and state.account_merkle_tree.height() == 4
        people = [state.sample_keys_and_register(pp, rng) for _ in range(3)]
        assert [p[0] for p in people] == [1, 2, 3]
        state.update_balance(1, 10)
        tx = L.Transaction.create(pp, 1, 2, 4, people[0][2], rng)
        root_before = state.root()
        proof, public = tx.prove_pedersen_payment(pp, state, rng)
        assert public == [root_before, 1, 2, 4]
        vk = state.pedersen_payment_keys(rng)[2]
        assert L.verify_payment(vk, public, proof, rng)
        assert state.apply_transaction(pp, tx, rng, prove=False) is True
        assert state.root() != root_before
        assert not L.verify_payment(vk, [state.root()] + public[1:], proof, rng)
        block = [L.Transaction.create(pp, 1, 2, 6, people[0][2], rng),       # all Alice has left
                 L.Transaction.create(pp, 1, 2, 7, people[0][2], rng),       # one more
                 L.Transaction.create(pp, 2, 3, 1, people[0][2], rng),       # not the sender's signature
                 L.Transaction.create(pp, 2, 9, 1, people[1][2], rng)]       # no such recipient
        got = L.prove_pedersen_payments(pp, state, block, rng)
        assert [g is None for g in got] == [False, True, True, True]
        assert got[0][1] == [state.root(), 1, 2, 6] and L.verify_payment(vk, got[0][1], got[0][0], rng)
        with pytest.raises(ValueError):
            state.payment_keys(rng)
        assert state._payment_keys is None and state._pedersen_payment_keys is not None
    finally:
        state.free()
        pp.free()
    assert state._pedersen_payment_keys is None


def test_pedersen_payment_keys_on_a_poseidon_state(M, L):
    import os
    from simpleworks_amd import hash as H
    ref_params = H.PoseidonParameters.from_json(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json"))
    rng = M.generate_rand()
    pp = L.Parameters.sample(rng, poseidon=ref_params)
    state = L.State(8, pp, account_tree="poseidon")
    try:
        with pytest.raises(ValueError):
            state.pedersen_payment_keys(rng)
    finally:
        state.free()
        pp.free()

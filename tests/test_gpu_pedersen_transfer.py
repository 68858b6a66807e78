"""The Pedersen transfer circuit's witness and proof entries (csrc/pedersen_transfer_witness.hip) and
State.apply_pedersen_transactions on the GPU, against the circuit's specification workloads.build_pedersen_transfer run on the CPU
over the blocks of tests/pedersen_transfer_model.py: whole witness vectors in Montgomery limbs over buffers pre-filled with 0xFF,
root pairs, flag bytes, status words, the account table and every node of the tree after a block; a dependent chain and a ring with
refusals in the middle against a twin tree taken through the same debits and credits by update_many; a block of 65 against 65
single calls; a table that is not the tree's; proof bytes against generate_proof on the builder's system.  Heights 2 (the paths meet
at the only level), 3 (both meeting levels, one with a level above), 4 (two levels above) and 9."""
import os

import numpy as np
import pytest

import pedersen_payment_model as PM
import pedersen_transfer_model as TM

pytestmark = pytest.mark.gpu

R = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001
POSEIDON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")
BLANK_SENDER = ("blank sender", TM.BLANK_ID, 1, 1, "sender")
# the transfers whose whole witness is compared with the builder's (every transfer's roots, flag, status and table are compared):
# d = 0 with the sender to the left and to the right, d = L - 1, levels above d, and each kind of refusal once
WITNESSED = {2: ("zero to one", "one to zero", "to oneself", "id out of range"),
             3: ("meet at level 0", "sender to the right", "amount zero", "overflow by 1", "overdraft by 1", "flipped signature"),
             4: ("meet at the top level", "sum 2^64 - 1", "blank recipient", "after the refusals"),
             9: ("meet at level 0", "meet at the top level")}
# the ring after transfer_model.CHAIN, which leaves account 2 empty: every account is credited and then debited by the next transfer
RING_AFTER_CHAIN = [("ring, one to two", 1, 2, 7, None), ("ring, two to three", 2, 3, 5, None), ("ring, three to one", 3, 1, 11, None)]
AT_9 = [c for c in TM.TRANSFERS if c[0] in ("meet at level 0", "meet at the top level", "overflow by 1", "to oneself", "after the refusals")]


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


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: %d witnesses differ, the first at %d" % (what, bad.size, bad[0])


def _node_rows(levels):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for level in levels for v in level), dtype=np.uint8).reshape(-1, 32)


def _pairs(ts):
    return [(t["message"], t["signature"]) for t in ts]


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
            made[height] = L.PedersenTransferCircuit(sig_params, crh[0], crh[1], height)
        return made[height]
    yield get
    for c in made.values():
        c.free()


@pytest.fixture(scope="module")
def world(params):
    """(height, block name) -> pedersen_transfer_model.transfers of that block, made once and left unchanged."""
    seen = {}
    blocks = {"cases": TM.TRANSFERS, "at 9": AT_9, "chain": TM.CHAIN + RING_AFTER_CHAIN, "blank sender": [TM.RING[0], BLANK_SENDER, TM.RING[1]]}

    def get(height, block="cases"):
        if (height, block) not in seen:
            seen[(height, block)] = TM.transfers(params, height, which=blocks[block])
        return seen[(height, block)]
    return get


@pytest.fixture
def fresh_tree(crh):
    """table -> a resident tree whose leaf level is that table; freed after the test."""
    from simpleworks_amd import hash as H
    made = []

    def get(height, table):
        tree = H.DeviceMerkleTree.blank(crh[0], crh[1], height, 72)
        held = [i for i, leaf in enumerate(table) if any(leaf)]
        tree.update_many(held, [table[i] for i in held])
        made.append(tree)
        return tree
    yield get
    for t in made:
        t.free()


@pytest.fixture(scope="module")
def oracle(M, params):
    """(height, block, transfer) -> the builder's witness as Montgomery limbs; built once per transfer."""
    seen = {}

    def get(height, block, t):
        k = (height, block, t["name"])
        if k not in seen:
            cs = _WitnessOnly()
            public = TM.build(params, height, t, cs=cs)[1]
            assert public == cs.public and public[0] == t["public"][0] and public[2:] == t["public"][2:]
            assert public[1] == t["walked_new_root"]
            seen[k] = M._to_mont_limbs(cs.witness)
        return seen[k]
    return get


def _check_block(c, tree, first, block, table, levels):
    """One call over the whole block into 0xFF-filled buffers: roots, flags, status, table and every node against the model."""
    w, after, old, new, flags, status = c.witness_at(tree, first, _pairs(block), fill=0xFF)
    assert list(flags) == [t["flag"] for t in block] and list(status) == [t["status"] for t in block]
    assert old == [t["public"][0] for t in block] and new == [t["public"][1] for t in block]
    assert [bool(f & 16) for f in flags] == [t["applied"] for t in block]
    assert after == table and tree.root() == levels[-1][0]
    assert np.array_equal(c.ctx.merkle_tree_nodes(tree.h).reshape(-1, 32), _node_rows(levels))
    return w, old, new


@pytest.mark.parametrize("height", [2, 3, 4, 9])
def test_whole_witness_roots_flags_and_table(M, circuits, world, fresh_tree, oracle, height):
    name = "at 9" if height == 9 else "cases"
    first, block, table, levels = world(height, name)
    c, tree = circuits(height), fresh_tree(height, first)
    assert c.shape() == M.pedersen_transfer_circuit_shape(height)
    w, old, new = _check_block(c, tree, first, block, table, levels)
    assert w.shape == (len(block), c.shape()[1], 4)
    names = [t["name"] for t in block]
    assert set(WITNESSED[height]) <= set(names)
    for k, t in enumerate(block):
        if t["name"] in WITNESSED[height]:
            _same(w[k], oracle(height, name, t), t["name"])
    # the ids the block covers: d = 0 (the recipient is the sender's sibling leaf) from both sides, and d = L - 1
    ds = {((t["message"][0] ^ t["message"][1]) & ((1 << (height - 1)) - 1)).bit_length() - 1 for t in block if t["applied"]}
    assert 0 in ds and height - 2 in ds


def test_a_dependent_chain_and_a_ring_in_one_block(circuits, world, fresh_tree, oracle):
    """1 -> 2, 2 -> 3, refusals, 3 -> 1, 2 -> 1, then the ring 1 -> 2 -> 3 -> 1: every later transfer is witnessed against the state the
    refused ones left unchanged, new_root_i = old_root_{i+1}, and the resident tree equals a twin taken through the same debits and
    credits by update_many: the root, every node, every leaf's path."""
    height = 3
    first, block, table, levels = world(height, "chain")
    assert [t["applied"] for t in block] == [True, True, False, False, True, True, True, True, True]
    c, tree, twin = circuits(height), fresh_tree(height, first), fresh_tree(height, first)
    w, old, new = _check_block(c, tree, first, block, table, levels)
    assert all(new[i] == old[i + 1] for i in range(len(block) - 1))
    assert old[2] == new[2] == old[3] == new[3]
    for t in block:
        if t["applied"]:
            s, r = t["message"][0], t["message"][1]
            twin.update_many([s], [t["debited_leaf"]])
            twin.update_many([r], [t["table"][r]])
    assert tree.root() == twin.root()
    assert np.array_equal(c.ctx.merkle_tree_nodes(tree.h), c.ctx.merkle_tree_nodes(twin.h))
    n = 1 << (height - 1)
    assert np.array_equal(tree.generate_proofs(list(range(n))), twin.generate_proofs(list(range(n))))
    assert [tree.generate_proof(i) for i in range(n)] == [PM.path(levels, i) for i in range(n)]
    for k in (3, 4, 7):     # a refused one in the middle, the one after it, and one of the ring (credited, then debited)
        _same(w[k], oracle(height, "chain", block[k]), block[k]["name"])


@pytest.mark.parametrize("count,chunk", [(7, 3), (3, 1)])
def test_the_dependent_chain_across_chunk_seams(circuits, world, fresh_tree, oracle, count, chunk):
    """The host form with its stage cap moved (swm_selftest_witness_stage): the chain's first 7 transfers at a cap of 3 transfers'
    witness bytes + 5 go in chunks of 3, 3 and 1, its first 3 at a cap one byte short of a transfer one by one.  Transfer i + 1 is
    witnessed against the state transfer i left, so a seam that lost the table or the tree would show: roots, flags, status, the
    table and every node as the chain test compares them, every witness the one-chunk run's, the first of each later chunk the
    builder's."""
    height = 3
    first, block = world(height, "chain")[0], world(height, "chain")[1][:count]
    table = block[-1]["table"]
    c, tree, twin, whole = circuits(height), fresh_tree(height, first), fresh_tree(height, first), fresh_tree(height, first)
    item = 32 * c.shape()[1]
    with c.ctx.selftest_witness_stage(3 * item + 5 if chunk == 3 else item - 1):
        w, after, old, new, flags, status = c.witness_at(tree, first, _pairs(block), fill=0xFF)
    assert list(flags) == [t["flag"] for t in block] and list(status) == [t["status"] for t in block]
    assert old == [t["public"][0] for t in block] and new == [t["public"][1] for t in block]
    assert [bool(f & 16) for f in flags] == [t["applied"] for t in block]
    assert all(new[i] == old[i + 1] for i in range(count - 1))
    assert after == table and tree.root() == new[-1]
    for t in block:
        if t["applied"]:
            s, r = t["message"][0], t["message"][1]
            twin.update_many([s], [t["debited_leaf"]])
            twin.update_many([r], [t["table"][r]])
    assert tree.root() == twin.root()
    assert np.array_equal(c.ctx.merkle_tree_nodes(tree.h), c.ctx.merkle_tree_nodes(twin.h))
    w1, after1, old1, new1, flags1, status1 = c.witness_at(whole, first, _pairs(block), fill=0xFF)      # one chunk: the default cap
    assert np.array_equal(w, w1) and after1 == after and (old1, new1) == (old, new)
    assert np.array_equal(flags1, flags) and np.array_equal(status1, status)
    for k in ((3, 6) if chunk == 3 else (1, 2)):
        _same(w[k], oracle(height, "chain", block[k]), block[k]["name"])


def test_a_blank_sender_in_the_middle(circuits, world, fresh_tree, oracle):
    """A blank sender: the Schnorr kernel refuses the key (status bit 0, its block zero), nothing is applied, equal roots; the
    transfers around it are the builder's."""
    height = 4
    first, block, table, levels = world(height, "blank sender")
    assert [(t["flag"], t["status"], t["applied"]) for t in block] == [(31, 0, True), (4, 1, False), (31, 0, True)]
    c, tree = circuits(height), fresh_tree(height, first)
    w, old, new = _check_block(c, tree, first, block, table, levels)
    assert old[1] == new[1] == new[0] == old[2]
    from simpleworks_amd import workloads as W
    lay = W.pedersen_transfer_circuit_layout(height)
    assert not w[1][:lay["balance"]].any()      # the refused key's Schnorr block
    _same(w[2], oracle(height, "blank sender", block[2]), block[2]["name"])


def _block_of_65():
    """65 transfers among accounts 1, 2, 3 whose outcomes depend on their order; items 0, 63 and 64 are refused."""
    ring = [(1, 2), (2, 3), (3, 1)]
    which = []
    for k in range(65):
        s, r = ring[k % 3]
        wrong = "signature" if k in (0, 63) else "overdraft" if k == 64 else None
        which.append(("item %d" % k, s, r, 1 << 62 if wrong == "overdraft" else 1 + k % 5, wrong))
    return which


def test_block_of_65_equals_single_calls(params, circuits, fresh_tree):
    height = 3
    first, block, table, levels = TM.transfers(params, height, which=_block_of_65())
    assert len(block) == 65 and [k for k, t in enumerate(block) if not t["applied"]] == [0, 63, 64]
    c, tree, twin = circuits(height), fresh_tree(height, first), fresh_tree(height, first)
    w, old, new = _check_block(c, tree, first, block, table, levels)
    accounts = first
    for k, t in enumerate(block):
        w1, accounts, o1, n1, f1, s1 = c.witness_at(twin, accounts, _pairs([t]))
        assert (o1[0], n1[0], int(f1[0]), int(s1[0])) == (old[k], new[k], t["flag"], 0), k
        assert np.array_equal(w1[0], w[k]), k
    assert accounts == table
    assert np.array_equal(c.ctx.merkle_tree_nodes(tree.h), c.ctx.merkle_tree_nodes(twin.h))


def test_a_table_that_is_not_the_trees_is_refused(L, circuits, world, fresh_tree, crh, sig_params):
    from simpleworks_amd._lib import SwmError
    height = 4
    first, block, _, _ = world(height)
    c, tree = circuits(height), fresh_tree(height, first)
    before = c.ctx.merkle_tree_nodes(tree.h)
    for wrong in ([first[k] if k != 2 else first[2][:64] + (6).to_bytes(8, "little") for k in range(len(first))],      # a balance
                  [first[k] if k != 5 else first[1] for k in range(len(first))],                                    # a leaf the tree holds blank
                  [first[k] if k != 3 else bytes(72) for k in range(len(first))]):                                  # blank where the tree holds one
        with pytest.raises(SwmError) as e:
            c.witness_at(tree, wrong, _pairs(block[:2]))
        assert e.value.code == -1 and "account table" in str(e.value)
        assert np.array_equal(c.ctx.merkle_tree_nodes(tree.h), before)
    # the entry itself at height 2, two transfers: a refused table leaves the caller's result arrays byte for byte
    small, pairs = world(2)[0], _pairs(world(2)[1][:2])
    c2, tree2 = circuits(2), fresh_tree(2, small)
    acc = np.frombuffer(small[0][:64] + bytes([small[0][64] ^ 1]) + small[0][65:] + small[1], dtype=np.uint8).copy()
    msgs, sigs = (np.frombuffer(b"".join(p[k] for p in pairs), dtype=np.uint8).copy() for k in (0, 1))
    w = np.zeros((2 * c2.shape()[1], 4), dtype=np.uint64)
    old, new = np.full((2, 32), 0xA5, dtype=np.uint8), np.full((2, 32), 0xA5, dtype=np.uint8)
    flags, status = np.full(2, 0xA5, dtype=np.uint8), np.full(2, 0xA5A5A5A5, dtype=np.uint32)
    rc = c2.ctx.lib.swm_pedersen_transfer_witness_at(c2.ctx.h, c2.h, tree2.h, acc.ctypes.data, msgs.ctypes.data, sigs.ctypes.data, 2,
                                                     w.ctypes.data, old.ctypes.data, new.ctypes.data, flags.ctypes.data, status.ctypes.data)
    assert rc == -1 and b"account table" in c2.ctx.lib.swm_last_error(c2.ctx.h)
    for out in (old, new, flags, status):
        assert np.all(out.view(np.uint8) == 0xA5)
    with pytest.raises(SwmError):       # a tree of another height
        circuits(2).witness_at(tree, first[:2], _pairs(block[:1]))
    for h in (1, 10):
        with pytest.raises(SwmError):
            L.PedersenTransferCircuit(sig_params, crh[0], crh[1], h)
    # and the same call with the right table goes through
    _, _, old, new, flags, _ = c.witness_at(tree, first, _pairs(block[:2]))
    assert list(flags) == [31, 31] and new[0] == old[1]


@pytest.fixture(scope="module")
def system(W, params, world):
    """The builder's system of the block's first transfer at height 3, packed once: its matrices serve every transfer."""
    t = world(3)[1][0]
    cs, public = TM.build(params, 3, t)
    assert public == t["public"] and t["applied"]
    return cs, cs.pack()


@pytest.fixture(scope="module")
def keys(M, system):
    cs, packed = system
    nnz = max(int(m[0][-1]) for m in packed.mats)
    srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, M.generate_rand())
    pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
    srs.free()
    yield pk, vk
    pk.free()


def test_proof_equals_the_builders(M, L, circuits, world, fresh_tree, system, keys):
    """swm_pedersen_transfer_prove_at is byte-identical to generate_proof on the builder's system from the same rng state; the proof
    verifies with its five public inputs and not with new_root bumped or replaced by old_root."""
    from simpleworks_amd import serialization as Ser
    first, block, _, _ = world(3)
    t = block[0]
    cs, _ = system
    pk, vk = keys
    c, tree = circuits(3), fresh_tree(3, first)
    want = Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand()))
    got, public, flag, status, after = M.generate_pedersen_transfer_proof(pk, c, tree, first, t["message"], t["signature"], M.generate_rand())
    assert got == want and public == t["public"] and (flag, status) == (31, 0) and after == t["table"]
    assert tree.root() == t["public"][1]
    assert L.verify_transfer(vk, public, got, M.generate_rand())
    assert not L.verify_transfer(vk, public[:1] + [(public[1] + 1) % R] + public[2:], got, M.generate_rand())
    assert not L.verify_transfer(vk, [public[0], public[0]] + public[2:], got, M.generate_rand())
    # a refused transfer has no proof and leaves tree and table alone
    bad = next(b for b in block if b["wrong"] == "signature")
    none, public, flag, status, again = M.generate_pedersen_transfer_proof(pk, c, tree, after, bad["message"], bad["signature"],
                                                                           M.generate_rand())
    assert none is None and public[0] == public[1] == t["public"][1] and not flag & 16 and again == after
    # the prover is as it was for the next caller: the device source does not outlive the call
    assert Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand())) == got


def test_block_of_proofs_equals_single_calls(M, L, circuits, world, fresh_tree, keys):
    first, block, table, levels = world(3, "chain")
    block = block[:6]
    table, root = block[-1]["table"], block[-1]["public"][1]
    pk, vk = keys
    c, tree, twin = circuits(3), fresh_tree(3, first), fresh_tree(3, first)
    rng = M.generate_rand()
    proofs, public, flags, status, after = M.generate_pedersen_transfer_proofs(pk, c, tree, first, _pairs(block), rng)
    assert flags == [t["flag"] for t in block] and status == [0] * len(block) and after == table
    assert public == [t["public"] for t in block] and tree.root() == root
    assert [p is not None for p in proofs] == [t["applied"] for t in block] == [True, True, False, False, True, True]
    rng = M.generate_rand()
    accounts = first
    for t, proof, pub in zip(block, proofs, public):
        single, pub1, _, _, accounts = M.generate_pedersen_transfer_proof(pk, c, twin, accounts, t["message"], t["signature"], rng)
        assert single == proof and pub1 == pub, t["name"]
        if proof is not None:
            assert L.verify_transfer(vk, pub, proof, M.generate_rand())
    assert accounts == table
    assert M.generate_pedersen_transfer_proofs(pk, c, tree, table, [], M.generate_rand())[0] == []


def test_block_of_proofs_across_chunk_seams(M, circuits, world, fresh_tree, keys):
    """swm_pedersen_transfer_prove_many_at with the stage cap one byte short of a transfer (swm_selftest_witness_stage): every
    transfer is a chunk of its own, and proofs, public inputs and the table are those of three single calls from the same rng
    state."""
    first, block = world(3, "chain")[0], world(3, "chain")[1][:3]
    pk, _ = keys
    c, tree, twin = circuits(3), fresh_tree(3, first), fresh_tree(3, first)
    assert pk.ctx is c.ctx      # the prover's context is the one whose cap moves
    with c.ctx.selftest_witness_stage(32 * c.shape()[1] - 1):
        proofs, public, flags, status, after = M.generate_pedersen_transfer_proofs(pk, c, tree, first, _pairs(block), M.generate_rand())
    assert flags == [t["flag"] for t in block] and status == [0, 0, 0] and after == block[-1]["table"]
    assert [p is not None for p in proofs] == [True, True, False] and public == [t["public"] for t in block]
    rng = M.generate_rand()
    accounts = first
    for t, proof, pub in zip(block, proofs, public):
        single, pub1, _, _, accounts = M.generate_pedersen_transfer_proof(pk, c, twin, accounts, t["message"], t["signature"], rng)
        assert single == proof and pub1 == pub, t["name"]
    assert accounts == after and tree.root() == twin.root()


def test_the_ledger_applies_a_block_over_its_pedersen_tree(M, L):
    """Over the default (Pedersen) state, apply_pedersen_transactions gives the balances and the root of a loop of
    apply_transaction(prove=False), refused transactions included; the proofs chain from root to root.  (Payments to oneself are left
    out: the two disagree.)"""
    from simpleworks_amd import hash as H, schnorr
    rng = M.generate_rand()
    pp = L.Parameters.sample(rng, poseidon=H.PoseidonParameters.from_json(POSEIDON))
    state, twin = L.State(8, pp), L.State(8, pp)
    try:
        people = [schnorr.keygen(pp.sig_params, rng) for _ in range(3)]
        for s in (state, twin):
            assert [s.register(pk) for pk, _ in people] == [1, 2, 3]
            s.update_balance(1, 10)
            s.update_balance(3, (1 << 64) - 2)
        txs = [L.Transaction.create(pp, 1, 2, 4, people[0][1], rng),
               L.Transaction.create(pp, 2, 3, 1, people[1][1], rng),
               L.Transaction.create(pp, 2, 3, 2, people[1][1], rng),       # overflows the recipient
               L.Transaction.create(pp, 1, 2, 7, people[0][1], rng),       # overdraft
               L.Transaction.create(pp, 2, 3, 1, people[0][1], rng),       # not the sender's signature
               L.Transaction.create(pp, 2, 0, 1, people[1][1], rng),       # no such recipient
               L.Transaction.create(pp, 3, 1, 5, people[2][1], rng)]
        want = [twin.apply_transaction(pp, tx, rng, prove=False) is True for tx in txs]
        assert want == [True, True, False, False, False, False, True]
        root_before = state.root()
        got = state.apply_pedersen_transactions(pp, txs, rng, prove=True)
        assert [g[0] for g in got] == want
        assert state.root() == twin.root()
        assert {i: a.balance for i, a in state.id_to_account_info.items()} == {i: a.balance for i, a in twin.id_to_account_info.items()}
        vk = state.pedersen_transfer_keys(rng)[2]
        root = root_before
        for (applied, proof, public), tx in zip(got, txs):
            assert public[0] == root and public[2:] == [tx.sender, tx.recipient, tx.amount]
            assert (proof is not None) == applied and (public[1] != public[0]) == applied
            if applied:
                assert L.verify_transfer(vk, public, proof, rng)
            root = public[1]
        assert root == state.root()
        # without proofs: the same advance
        more = [L.Transaction.create(pp, 3, 2, 1, people[2][1], rng)]
        assert [g[:2] for g in state.apply_pedersen_transactions(pp, more, rng, prove=False)] == [(True, None)]
        assert twin.apply_transaction(pp, more[0], rng, prove=False) is True and state.root() == twin.root()
        poseidon = L.State(8, pp, account_tree="poseidon")
        try:
            with pytest.raises(ValueError):
                poseidon.pedersen_transfer_keys(rng)
            with pytest.raises(ValueError):
                poseidon.apply_pedersen_transactions(pp, more, rng)
        finally:
            poseidon.free()
    finally:
        state.free()
        twin.free()
        pp.free()

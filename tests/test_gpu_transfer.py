"""The transfer circuit's witness and proof entries (csrc/transfer_witness.hip) and State.apply_transactions on the GPU, against the
circuit's specification workloads.build_transfer run on the CPU over the blocks of tests/transfer_model.py: whole witness vectors
in Montgomery limbs, root pairs, flag bytes, status words, the account table and every node of the tree after a block; a dependent
chain with refusals in the middle against a twin tree that received two updates per applied transfer; a block of 65 (one past the
record launch's 64-lane workgroup) against 65 single calls; a table that is not the tree's; proof bytes against generate_proof on
the builder's system.  Heights 2, 4 and 9."""
import os

import numpy as np
import pytest

import poseidon_model as P
import poseidon_tree_model as T
import transfer_model as TM
from oracle_lib import golden

pytestmark = pytest.mark.gpu

R = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001
PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")


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
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in T.nodes(levels)), dtype=np.uint8).reshape(-1, 32)


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
    p = schnorr.Parameters()
    yield p
    p.free()


@pytest.fixture(scope="module")
def circuits(L, sig_params, sponge):
    made = {}

    def get(height):
        if height not in made:
            made[height] = L.TransferCircuit(sig_params, sponge, height)
        return made[height]
    yield get
    for c in made.values():
        c.free()


@pytest.fixture(scope="module")
def world(ref):
    """(height, block name) -> transfer_model.transfers of that block, made once."""
    seen = {}
    blocks = {"cases": TM.TRANSFERS, "chain": TM.CHAIN}

    def get(height, block="cases"):
        if (height, block) not in seen:
            seen[(height, block)] = TM.transfers(ref, height, which=blocks[block])
        return seen[(height, block)]
    return get


@pytest.fixture
def fresh_tree(sponge):
    """table -> a resident tree whose leaf level is that table; freed after the test."""
    from simpleworks_amd import hash as H
    made = []

    def get(height, table):
        tree = H.PoseidonMerkleTree.blank(sponge, height, 72)
        held = [i for i, leaf in enumerate(table) if any(leaf)]
        tree.update_many(held, [table[i] for i in held])
        made.append(tree)
        return tree
    yield get
    for t in made:
        t.free()


@pytest.fixture(scope="module")
def oracle(M, W, ref_params):
    """(height, transfer) -> the builder's witness as Montgomery limbs; built once per transfer."""
    seen = {}

    def get(height, block, t):
        k = (height, block, t["name"])
        if k not in seen:
            cs = _WitnessOnly()
            public = W.build_transfer(cs, TM.S.GENERATOR, None, ref_params, height, t["message"], t["signature"], t["sender_leaf"],
                                      t["sender_path"], t["recipient_leaf"], t["recipient_path"])
            assert public == cs.public and public[0] == t["public"][0] and public[2:] == t["public"][2:]
            assert public[1] == t["walked_new_root"] or t["wrong"] == "recipient"
            seen[k] = M._to_mont_limbs(cs.witness)
        return seen[k]
    return get


def _pairs(ts):
    return [(t["message"], t["signature"]) for t in ts]


def _check_item(W, c, oracle, height, block, t, w):
    lay = W.transfer_circuit_layout(c.sponge.params, height)
    want = oracle(height, block, t)
    if t["wrong"] == "recipient":
        # a blank leaf's digest in the tree is zero, not its own walk's: the recipient's membership block holds the tree's digests
        _same(w[:lay["recipient"]], want[:lay["recipient"]], t["name"] + ", up to the recipient's block")
        _same(w[lay["sum"]:], want[lay["sum"]:], t["name"] + ", after the recipient's block")
    else:
        _same(w, want, t["name"])


# at height 9 the builder runs for the transfers that are about the tree's shape and for one of each kind of refusal
NAMES_AT_9 = ("meet at level 0", "sender to the right", "meet at the top level", "overflow by 1", "to oneself")


@pytest.mark.parametrize("height", [2, 4, 9])
def test_whole_witness_roots_flags_and_table(W, circuits, world, fresh_tree, oracle, height):
    first, block, table, levels = world(height)
    G = golden("transfer.json")
    if height == G["height"]:
        assert [t["name"] for t in block] == [g["name"] for g in G["transfers"]] == [t[0] for t in TM.TRANSFERS]
        assert [t["flag"] for t in block] == [g["flag"] for g in G["transfers"]]
    c, tree = circuits(height), fresh_tree(height, first)
    w, after, old, new, flags, status = c.witness_at(tree, first, _pairs(block))
    assert list(flags) == [t["flag"] for t in block] and list(status) == [t["status"] for t in block]
    assert old == [t["public"][0] for t in block] and new == [t["public"][1] for t in block]
    assert [bool(f & 16) for f in flags] == [t["applied"] for t in block]
    assert after == table and tree.root() == levels[-1][0]
    assert np.array_equal(c.ctx.poseidon_tree_nodes(tree.h), _node_rows(levels))
    for k, t in enumerate(block):
        if height == 9 and t["name"] not in NAMES_AT_9:
            continue
        _check_item(W, c, oracle, height, "cases", t, w[k])


def test_a_dependent_chain_in_one_block(W, circuits, world, fresh_tree, oracle):
    """1 -> 2, 2 -> 3, 3 -> 1 with refused transfers in the middle: every later transfer is witnessed against the state the refused
    ones left unchanged, new_root_i = old_root_{i+1}, and the nodes are those of a twin tree after two updates per applied
    transfer."""
    height = 4
    first, block, table, levels = world(height, "chain")
    assert [t["applied"] for t in block] == [True, True, False, False, True, True]
    c, tree, twin = circuits(height), fresh_tree(height, first), fresh_tree(height, first)
    w, after, old, new, flags, status = c.witness_at(tree, first, _pairs(block))
    assert list(flags) == [t["flag"] for t in block] and not status.any()
    assert old == [t["public"][0] for t in block] and new == [t["public"][1] for t in block]
    assert all(new[i] == old[i + 1] for i in range(len(block) - 1))
    assert old[2] == new[2] == old[3] == new[3]
    assert new[-1] == tree.root() == levels[-1][0] and after == table
    for t in block:
        if t["applied"]:
            s, r = t["message"][0], t["message"][1]
            twin.update(s, t["table"][s])
            twin.update(r, t["table"][r])
    assert np.array_equal(c.ctx.poseidon_tree_nodes(tree.h), c.ctx.poseidon_tree_nodes(twin.h))
    for k in (3, 4, 5):
        _check_item(W, c, oracle, height, "chain", block[k], w[k])


@pytest.fixture(scope="module")
def chain7(ref):
    """The dependent chain and one more transfer out of the account the chain's last one credited: seven in all."""
    first, block, table, levels = TM.transfers(ref, 4, which=TM.CHAIN + [("one to three", 1, 3, 5, None)])
    assert [t["applied"] for t in block] == [True, True, False, False, True, True, True]
    return first, block, table, levels


@pytest.mark.parametrize("count,chunk", [(7, 3), (3, 1)])
def test_the_dependent_chain_across_chunk_seams(W, circuits, chain7, fresh_tree, oracle, count, chunk):
    """The host form with its stage cap moved (swm_selftest_witness_stage): the chain's 7 transfers at a cap of 3 transfers' witness
    bytes + 5 go in chunks of 3, 3 and 1, its first 3 at a cap one byte short of a transfer one by one.  Transfer i + 1 is
    witnessed against the state transfer i left, so a seam that lost the table or the tree would show: roots, flags, status, the
    table and every node as the chain test compares them, every witness the one-chunk run's, the first of each later chunk the
    builder's."""
    height = 4
    first, block = chain7[0], chain7[1][:count]
    table = block[-1]["table"]
    c, tree, twin, whole = circuits(height), fresh_tree(height, first), fresh_tree(height, first), fresh_tree(height, first)
    item = 32 * c.shape()[1]
    with c.ctx.selftest_witness_stage(3 * item + 5 if chunk == 3 else item - 1):
        w, after, old, new, flags, status = c.witness_at(tree, first, _pairs(block))
    assert list(flags) == [t["flag"] for t in block] and not status.any()
    assert old == [t["public"][0] for t in block] and new == [t["public"][1] for t in block]
    assert all(new[i] == old[i + 1] for i in range(count - 1))
    assert new[-1] == tree.root() and after == table and (count < 7 or (after == chain7[2] and tree.root() == chain7[3][-1][0]))
    for t in block:
        if t["applied"]:
            s, r = t["message"][0], t["message"][1]
            twin.update(s, t["table"][s])
            twin.update(r, t["table"][r])
    assert np.array_equal(c.ctx.poseidon_tree_nodes(tree.h), c.ctx.poseidon_tree_nodes(twin.h))
    w1, after1, old1, new1, flags1, status1 = c.witness_at(whole, first, _pairs(block))      # one chunk: the default cap
    assert np.array_equal(w, w1) and after1 == after and (old1, new1) == (old, new)
    assert np.array_equal(flags1, flags) and np.array_equal(status1, status)
    for k in ((3, 6) if chunk == 3 else (1, 2)):
        _check_item(W, c, oracle, height, "chain7", block[k], w[k])


def _block_of_65():
    """65 transfers among accounts 1, 2, 3 whose outcomes depend on their order; items 0, 63 and 64 are refused."""
    ring = [(1, 2), (2, 3), (3, 1)]
    which = []
    for k in range(65):
        s, r = ring[k % 3]
        wrong = "signature" if k in (0, 63) else "overdraft" if k == 64 else None
        which.append(("item %d" % k, s, r, 1 << 62 if wrong == "overdraft" else 1 + k % 5, wrong))
    return which


def test_block_of_65_equals_single_calls(ref, circuits, fresh_tree):
    height = 4
    first, block, table, levels = TM.transfers(ref, height, which=_block_of_65())
    assert len(block) == 65 and [k for k, t in enumerate(block) if not t["applied"]] == [0, 63, 64]
    c, tree, twin = circuits(height), fresh_tree(height, first), fresh_tree(height, first)
    w, after, old, new, flags, status = c.witness_at(tree, first, _pairs(block))
    assert list(flags) == [t["flag"] for t in block] and not status.any()
    assert old == [t["public"][0] for t in block] and new == [t["public"][1] for t in block]
    assert after == table and tree.root() == levels[-1][0]
    accounts = first
    for k, t in enumerate(block):
        w1, accounts, o1, n1, f1, s1 = c.witness_at(twin, accounts, _pairs([t]))
        assert (o1[0], n1[0], int(f1[0]), int(s1[0])) == (old[k], new[k], int(flags[k]), 0), k
        assert np.array_equal(w1[0], w[k]), k
    assert accounts == table
    assert np.array_equal(c.ctx.poseidon_tree_nodes(tree.h), c.ctx.poseidon_tree_nodes(twin.h))


def test_a_table_that_is_not_the_trees_is_refused(L, circuits, world, fresh_tree, sponge, sig_params):
    from simpleworks_amd._lib import SwmError
    height = 4
    first, block, _, _ = world(height)
    c, tree = circuits(height), fresh_tree(height, first)
    before = c.ctx.poseidon_tree_nodes(tree.h)
    for wrong in ([first[k] if k != 2 else first[2][:64] + (6).to_bytes(8, "little") for k in range(len(first))],      # a balance
                  [first[k] if k != 5 else first[1] for k in range(len(first))],                                    # a leaf the tree holds blank
                  [first[k] if k != 3 else bytes(72) for k in range(len(first))]):                                  # blank where the tree holds one
        with pytest.raises(SwmError) as e:
            c.witness_at(tree, wrong, _pairs(block[:2]))
        assert e.value.code == -1 and "account table" in str(e.value)
        assert np.array_equal(c.ctx.poseidon_tree_nodes(tree.h), before)
    # the entry itself at height 2, two transfers: a refused table leaves the caller's result arrays byte for byte
    small, pairs = world(2)[0], _pairs(world(2)[1][:2])
    c2, tree2 = circuits(2), fresh_tree(2, small)
    acc = np.frombuffer(small[0][:64] + bytes([small[0][64] ^ 1]) + small[0][65:] + small[1], dtype=np.uint8).copy()
    msgs, sigs = (np.frombuffer(b"".join(p[k] for p in pairs), dtype=np.uint8).copy() for k in (0, 1))
    w = np.zeros((2 * c2.shape()[1], 4), dtype=np.uint64)
    old, new = np.full((2, 32), 0xA5, dtype=np.uint8), np.full((2, 32), 0xA5, dtype=np.uint8)
    flags, status = np.full(2, 0xA5, dtype=np.uint8), np.full(2, 0xA5A5A5A5, dtype=np.uint32)
    rc = c2.ctx.lib.swm_transfer_witness_at(c2.ctx.h, c2.h, tree2.h, acc.ctypes.data, msgs.ctypes.data, sigs.ctypes.data, 2, w.ctypes.data,
                                            old.ctypes.data, new.ctypes.data, flags.ctypes.data, status.ctypes.data)
    assert rc == -1 and b"account table" in c2.ctx.lib.swm_last_error(c2.ctx.h)
    for out in (old, new, flags, status):
        assert np.all(out.view(np.uint8) == 0xA5)
    with pytest.raises(SwmError):       # a tree of another height
        circuits(2).witness_at(tree, first[:2], _pairs(block[:1]))
    for h in (1, 10):
        with pytest.raises(SwmError):
            L.TransferCircuit(sig_params, sponge, h)
    # and the same call with the right table goes through
    _, _, old, new, flags, _ = c.witness_at(tree, first, _pairs(block[:2]))
    assert list(flags) == [31, 31] and new[0] == old[1]


@pytest.fixture(scope="module")
def system(W, ref_params, world):
    """The builder's system of the block's first transfer at height 4, packed once: its matrices serve every transfer."""
    t = world(4)[1][0]
    cs, public = W.transfer_circuit(ref_params, 4, t["message"], t["signature"], t["sender_leaf"], t["sender_path"], t["recipient_leaf"],
                                    t["recipient_path"])
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
    """swm_transfer_prove_at is byte-identical to generate_proof on the builder's system from the same rng state; the proof
    verifies with its five public inputs, with none of them changed, and not with new_root replaced by old_root."""
    from simpleworks_amd import serialization as Ser
    first, block, _, _ = world(4)
    t = block[0]
    cs, _ = system
    pk, vk = keys
    c, tree = circuits(4), fresh_tree(4, first)
    want = Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand()))
    got, public, flag, status, after = M.generate_transfer_proof(pk, c, tree, first, t["message"], t["signature"], M.generate_rand())
    assert got == want and public == t["public"] and (flag, status) == (31, 0) and after == t["table"]
    assert tree.root() == t["public"][1]
    assert L.verify_transfer(vk, public, got, M.generate_rand())
    for k in range(5):
        other = list(public)
        other[k] = (other[k] + 1) % R
        assert not L.verify_transfer(vk, other, got, M.generate_rand()), k
    assert not L.verify_transfer(vk, [public[0], public[0]] + public[2:], got, M.generate_rand())
    # a refused transfer has no proof and leaves tree and table alone
    bad = block[8]
    assert bad["wrong"] == "signature"
    none, public, flag, status, again = M.generate_transfer_proof(pk, c, tree, after, bad["message"], bad["signature"], M.generate_rand())
    assert none is None and public[0] == public[1] == t["public"][1] and not flag & 16 and again == after
    # the prover is as it was for the next caller: the device source does not outlive the call
    assert Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand())) == got


def test_block_of_proofs_equals_single_calls(M, L, circuits, world, fresh_tree, keys):
    first, block, table, levels = world(4, "chain")
    pk, vk = keys
    c, tree, twin = circuits(4), fresh_tree(4, first), fresh_tree(4, first)
    rng = M.generate_rand()
    proofs, public, flags, status, after = M.generate_transfer_proofs(pk, c, tree, first, _pairs(block), rng)
    assert flags == [t["flag"] for t in block] and status == [0] * len(block) and after == table
    assert public == [t["public"] for t in block] and tree.root() == levels[-1][0]
    assert [p is not None for p in proofs] == [t["applied"] for t in block]
    rng = M.generate_rand()
    accounts = first
    for t, proof, pub in zip(block, proofs, public):
        single, pub1, _, _, accounts = M.generate_transfer_proof(pk, c, twin, accounts, t["message"], t["signature"], rng)
        assert single == proof and pub1 == pub, t["name"]
        if proof is not None:
            assert L.verify_transfer(vk, pub, proof, M.generate_rand())
            assert not L.verify_transfer(vk, [pub[0], pub[0]] + pub[2:], proof, M.generate_rand())
    assert accounts == table
    assert M.generate_transfer_proofs(pk, c, tree, table, [], M.generate_rand())[0] == []


def test_block_of_proofs_across_chunk_seams(M, circuits, chain7, fresh_tree, keys):
    """swm_transfer_prove_many_at with the stage cap one byte short of a transfer (swm_selftest_witness_stage): every transfer is a
    chunk of its own, and proofs, public inputs and the table are those of three single calls from the same rng state."""
    first, block = chain7[0], chain7[1][:3]
    pk, _ = keys
    c, tree, twin = circuits(4), fresh_tree(4, first), fresh_tree(4, first)
    assert pk.ctx is c.ctx      # the prover's context is the one whose cap moves
    with c.ctx.selftest_witness_stage(32 * c.shape()[1] - 1):
        proofs, public, flags, status, after = M.generate_transfer_proofs(pk, c, tree, first, _pairs(block), M.generate_rand())
    assert flags == [t["flag"] for t in block] and status == [0, 0, 0] and after == block[-1]["table"]
    assert [p is not None for p in proofs] == [True, True, False] and public == [t["public"] for t in block]
    rng = M.generate_rand()
    accounts = first
    for t, proof, pub in zip(block, proofs, public):
        single, pub1, _, _, accounts = M.generate_transfer_proof(pk, c, twin, accounts, t["message"], t["signature"], rng)
        assert single == proof and pub1 == pub, t["name"]
    assert accounts == after and tree.root() == twin.root()


def test_the_ledger_applies_a_block(M, L, ref_params):
    """Over a Poseidon state, apply_transactions gives the balances and the root of a loop of apply_transaction(prove=False),
    refused transactions included; the proofs chain from root to root.  (Payments to oneself are left out: the two disagree.)"""
    from simpleworks_amd import schnorr
    rng = M.generate_rand()
    pp = L.Parameters.sample(rng, poseidon=ref_params)
    state, twin = L.State(16, pp, account_tree="poseidon"), L.State(16, pp, account_tree="poseidon")
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
               L.Transaction.create(pp, 2, 9, 1, people[1][1], rng),       # no such recipient
               L.Transaction.create(pp, 3, 1, 5, people[2][1], rng)]
        want = [twin.apply_transaction(pp, tx, rng, prove=False) is True for tx in txs]
        assert want == [True, True, False, False, False, False, True]
        root_before = state.root()
        got = state.apply_transactions(pp, txs, rng, prove=True)
        assert [g[0] for g in got] == want
        assert state.root() == twin.root()
        assert {i: a.balance for i, a in state.id_to_account_info.items()} == {i: a.balance for i, a in twin.id_to_account_info.items()}
        vk = state.transfer_keys(rng)[2]
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
        assert [g[:2] for g in state.apply_transactions(pp, more, rng, prove=False)] == [(True, None)]
        assert twin.apply_transaction(pp, more[0], rng, prove=False) is True and state.root() == twin.root()
        pedersen = L.State(8, pp)
        try:
            with pytest.raises(ValueError):
                pedersen.apply_transactions(pp, more, rng)
        finally:
            pedersen.free()
    finally:
        state.free()
        twin.free()
        pp.free()

"""The account-update circuit's witness and proof entries (csrc/account_update_witness.hip) and State.apply_updates on the GPU,
against the circuit's specification workloads.build_account_update run on the CPU over the blocks of tests/account_update_model.py:
whole witness vectors in Montgomery limbs with 0xFF guard elements behind them, root pairs, flags, status words, the account table
and every node of the tree after a block; blocks of 1, 2, 64 and 65 (one past the record launch's 64-lane workgroup); each refusal
in the middle of a block against a twin tree taken through the applied operations by swm_poseidon_tree_update; a table that is not
the tree's; a chunk seam inside a small batch; proof bytes against generate_proof on the builder's system; and the chain of proofs
from State::new's blank root through registrations, balance updates and a transfer to the state's root."""
import os

import numpy as np
import pytest

import account_update_model as AM
import poseidon_model as P
import poseidon_tree_model as T

pytestmark = pytest.mark.gpu

R = AM.R
PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")
GUARD = 3


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
def circuits(L, sponge):
    made = {}

    def get(height):
        if height not in made:
            made[height] = L.AccountUpdateCircuit(sponge, height)
        return made[height]
    yield get
    for c in made.values():
        c.free()


@pytest.fixture
def fresh_tree(sponge):
    """table -> a resident tree whose leaf level is that table; freed after the test."""
    from simpleworks_amd import hash as H
    made = []

    def get(height, table):
        tree = H.PoseidonMerkleTree.blank(sponge, height, 72)
        held = [i for i, leaf in enumerate(table) if any(leaf)]
        if held:
            tree.update_many(held, [table[i] for i in held])
        made.append(tree)
        return tree
    yield get
    for t in made:
        t.free()


@pytest.fixture(scope="module")
def oracle(M, W, ref_params):
    """(height, operation of the model) -> the builder's witness as Montgomery limbs; built once per distinct input."""
    seen = {}

    def get(height, t):
        k = (height, t["id"], t["key"], t["old_balance"], t["new_balance"], t["fresh"], tuple(t["path"]))
        if k not in seen:
            cs = _WitnessOnly()
            public = W.build_account_update(cs, ref_params, height, t["id"], t["key"], t["old_balance"], t["new_balance"], t["fresh"], t["path"])
            assert public == cs.public and public[:2] == [t["old_root"], t["new_root"]]
            seen[k] = M._to_mont_limbs(cs.witness)
        return seen[k]
    return get


def _run(c, tree, table, ops, guard=GUARD):
    """witness_at with guard elements: -> (witness [count, num_witness, 4], table, old, new, flags, status); the guard is checked."""
    nw = c.shape()[1]
    w, after, old, new, flags, status = c.witness_at(tree, table, ops, guard=guard)
    assert w.shape == (len(ops) * nw + guard, 4)
    assert (w[len(ops) * nw:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "the guard elements behind the last witness were written"
    return w[:len(ops) * nw].reshape(len(ops), nw, 4), after, old, new, flags, status


def _check_block(c, oracle, height, block, got, what):
    """Roots, flags, status and every witness vector of a block against the model and the builder."""
    w, _, old, new, flags, status = got
    assert list(status) == [t["status"] for t in block], what
    assert [bool(f & 1) for f in flags] == [t["applied"] for t in block] and not (np.asarray(flags) & 0xFE).any(), what
    assert old == [t["old_root"] for t in block] and new == [t["new_root"] for t in block], what
    for k, t in enumerate(block):
        if t["applied"]:
            _same(w[k], oracle(height, t), "%s, item %d" % (what, k))
        else:
            assert not w[k].any() and old[k] == new[k], "%s, item %d: a refused operation's witness is zero, its roots equal" % (what, k)


@pytest.mark.parametrize("height", [2, 4])
def test_whole_witness_vectors_of_the_dependence_block(ref, circuits, fresh_tree, oracle, height):
    """From the blank tree: a registration followed by a balance update of the same leaf, two sibling leaves (the second's sibling is
    the first's new digest), the leftmost and the rightmost leaf."""
    table, levels = AM.blank(ref, height)
    block, final, levels = AM.apply(ref, height, table, levels, AM.dependences(height))
    assert all(t["applied"] for t in block)
    if height > 2:
        a, b = next((i, j) for i, s in enumerate(block) for j, t in enumerate(block) if j == i + 1 and s["id"] ^ t["id"] == 1)
        assert block[b]["path"][0] == T.HL(ref, block[a]["new_leaf"])
    c, tree = circuits(height), fresh_tree(height, table)
    got = _run(c, tree, table, [t["op"] for t in block])
    _check_block(c, oracle, height, block, got, "dependences at height %d" % height)
    _, after, old, new, _, _ = got
    assert old[0] == T.blank(ref, height)[-1][0] and all(new[i] == old[i + 1] for i in range(len(block) - 1))
    assert after == final and new[-1] == tree.root() == levels[-1][0]
    assert np.array_equal(c.ctx.poseidon_tree_nodes(tree.h), _node_rows(levels))


@pytest.fixture(scope="module")
def block65(ref):
    table, levels = AM.blank(ref, 2)
    block, final, levels = AM.apply(ref, 2, table, levels, AM.block_of(65, 2))
    assert [k for k, t in enumerate(block) if not t["applied"]] == [9, 63]
    return table, block


@pytest.mark.parametrize("count", [1, 2, 64, 65])
def test_counts_around_the_record_workgroup(ref, circuits, fresh_tree, oracle, block65, count):
    table, block = block65
    block = block[:count]
    c, tree = circuits(2), fresh_tree(2, table)
    got = _run(c, tree, table, [t["op"] for t in block])
    _check_block(c, oracle, 2, block, got, "%d operations" % count)
    assert got[1] == block[-1]["table"] and tree.root() == block[-1]["new_root"]


@pytest.mark.parametrize("which", range(7))
def test_each_refusal_in_the_middle_of_a_block(ref, circuits, fresh_tree, oracle, which):
    """[a registration, the refusal, a balance update of the account the first one made]: the refused item's status bit stands
    alone, its witness is zero and its roots are equal; the operations around it are as if it were not there; tree nodes and table
    equal those of a twin tree taken through the applied operations alone by swm_poseidon_tree_update."""
    height = 4
    held, cases = AM.refusals(height)
    name, bad, st = cases[which]
    table, levels = AM.blank(ref, height)
    _, first, levels = AM.apply(ref, height, table, levels, [(held, AM.REGISTER, AM.key(held), 0), (held, AM.SET, AM.NO_KEY, 100)])
    ops = [(5, AM.REGISTER, AM.key(5), 0), bad, (5, AM.SET, AM.NO_KEY, 55)]
    block, final, after_levels = AM.apply(ref, height, first, levels, ops)
    assert [t["status"] for t in block] == [0, st, 0] and bin(st).count("1") == 1, name
    c, tree, twin = circuits(height), fresh_tree(height, first), fresh_tree(height, first)
    got = _run(c, tree, first, ops)
    _check_block(c, oracle, height, block, got, name)
    assert int(got[5][1]) == st and int(got[4][1]) == 0
    assert got[1] == final and got[3][0] == got[2][1] == got[3][1] == got[2][2]
    for t in block:
        if t["applied"]:
            twin.update(t["id"], t["new_leaf"])
    assert np.array_equal(c.ctx.poseidon_tree_nodes(tree.h), c.ctx.poseidon_tree_nodes(twin.h))
    assert np.array_equal(c.ctx.poseidon_tree_nodes(tree.h), _node_rows(after_levels))


def test_a_table_that_is_not_the_trees_is_refused(L, ref, circuits, fresh_tree, sponge):
    """Any difference between the table and the tree's leaf level refuses the call and leaves both byte for byte: the entry is called
    through ctypes here, so that the caller's table is seen after the refusal."""
    from simpleworks_amd._lib import SwmError
    height = 4
    table, levels = AM.blank(ref, height)
    _, first, levels = AM.apply(ref, height, table, levels, [(1, AM.REGISTER, AM.key(1), 3), (6, AM.REGISTER, AM.key(6), 0)])
    c, tree = circuits(height), fresh_tree(height, first)
    nw = c.shape()[1]
    before = c.ctx.poseidon_tree_nodes(tree.h)
    ops = [(2, AM.REGISTER, AM.key(2), 0), (1, AM.SET, AM.NO_KEY, 9)]
    for wrong in ([first[k] if k != 1 else first[1][:64] + (4).to_bytes(8, "little") for k in range(len(first))],      # a balance
                  [first[k] if k != 5 else first[1] for k in range(len(first))],                                    # a leaf the tree holds blank
                  [first[k] if k != 6 else bytes(72) for k in range(len(first))]):                                  # blank where the tree holds one
        acc = np.frombuffer(b"".join(wrong), dtype=np.uint8).reshape(-1, 72).copy()
        kept = acc.copy()
        ids, kinds = np.array([o[0] for o in ops], dtype=np.uint8), np.array([o[1] for o in ops], dtype=np.uint8)
        keys = np.frombuffer(b"".join(o[2] for o in ops), dtype=np.uint8).copy()
        bal = np.array([o[3] for o in ops], dtype="<u8")
        w = np.zeros((2 * nw, 4), dtype=np.uint64)
        old, new = np.full((2, 32), 0xA5, dtype=np.uint8), np.full((2, 32), 0xA5, dtype=np.uint8)
        flags, status = np.full(2, 0xA5, dtype=np.uint8), np.full(2, 0xA5A5A5A5, dtype=np.uint32)
        rc = c.ctx.lib.swm_account_update_witness_at(c.ctx.h, c.h, tree.h, acc.ctypes.data, ids.ctypes.data, kinds.ctypes.data, keys.ctypes.data,
                                                     bal.ctypes.data, 2, w.ctypes.data, old.ctypes.data, new.ctypes.data, flags.ctypes.data,
                                                     status.ctypes.data)
        assert rc == -1 and b"account table" in c.ctx.lib.swm_last_error(c.ctx.h)
        assert np.array_equal(acc, kept) and np.array_equal(c.ctx.poseidon_tree_nodes(tree.h), before)
        for out in (old, new, flags, status):    # nothing is copied out after a refused table
            assert np.all(out.view(np.uint8) == 0xA5)
    with pytest.raises(SwmError) as e:       # a kind that is neither
        c.witness_at(tree, first, [(2, 2, AM.key(2), 0)])
    assert e.value.code == -1 and "kind 2" in str(e.value)
    with pytest.raises(SwmError):            # a tree of another height
        circuits(2).witness_at(tree, first[:2], ops[:1])
    assert np.array_equal(c.ctx.poseidon_tree_nodes(tree.h), before)
    for h in (1, 10):
        with pytest.raises(SwmError):
            L.AccountUpdateCircuit(sponge, h)
    # and the same call with the right table goes through
    _, after, old, new, flags, _ = c.witness_at(tree, first, ops)
    assert list(flags) == [1, 1] and new[0] == old[1] and after[2] == AM.key(2) + bytes(8)


def test_a_chunk_seam_inside_a_small_batch(ref, circuits, fresh_tree, oracle):
    """The host form with its stage cap moved (swm_selftest_witness_stage): the dependence block's 9 operations at a cap of 4 items'
    witness bytes + 5 go in chunks of 4, 4 and 1.  Operation i + 1 is witnessed against the state operation i left, so a seam that
    lost the table or the tree would show."""
    height = 4
    table, levels = AM.blank(ref, height)
    block, final, levels = AM.apply(ref, height, table, levels, AM.dependences(height))
    assert len(block) == 9
    c, tree, whole = circuits(height), fresh_tree(height, table), fresh_tree(height, table)
    item = 32 * c.shape()[1]
    with c.ctx.selftest_witness_stage(4 * item + 5):
        got = _run(c, tree, table, [t["op"] for t in block])
    _check_block(c, oracle, height, block, got, "chunks of 4, 4 and 1")
    assert got[1] == final and tree.root() == levels[-1][0]
    one = _run(c, whole, table, [t["op"] for t in block])      # one chunk: the default cap
    assert np.array_equal(got[0], one[0]) and got[1:4] == one[1:4]
    assert np.array_equal(c.ctx.poseidon_tree_nodes(tree.h), c.ctx.poseidon_tree_nodes(whole.h))


@pytest.fixture(scope="module")
def world4(ref):
    table, levels = AM.blank(ref, 4)
    block, final, levels = AM.apply(ref, 4, table, levels, AM.dependences(4))
    return table, block


@pytest.fixture(scope="module")
def system(W, ref_params, world4):
    """The builder's systems of the block's first two operations at height 4 (a registration, then the balance update of the same
    leaf); the first one's matrices serve every operation."""
    out = []
    for t in world4[1][:2]:
        cs, public = W.account_update_circuit(ref_params, 4, t["id"], t["key"], t["old_balance"], t["new_balance"], t["fresh"], t["path"])
        assert public[:2] == [t["old_root"], t["new_root"]]
        out.append((cs, public))
    return out, out[0][0].pack()


@pytest.fixture(scope="module")
def keys(M, system):
    (cs, _), packed = system[0][0], system[1]
    nnz = max(int(m[0][-1]) for m in packed.mats)
    srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, M.generate_rand())
    pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
    srs.free()
    yield pk, vk
    pk.free()


def test_proof_equals_the_builders(M, W, L, circuits, world4, fresh_tree, system, keys):
    """swm_account_update_prove_at is byte-identical to generate_proof on the builder's system from the same rng state, for the
    registration and for the balance update under the ONE key; verify_update accepts the proof with its eight public inputs and
    rejects it with each of them changed in turn; a key of another shape gives SWM_ERR_MISMATCH with the tree untouched."""
    from simpleworks_amd import serialization as Ser
    table, block = world4
    pk, vk = keys
    c, tree = circuits(4), fresh_tree(4, table)
    accounts = table
    for t, (cs, want_public) in zip(block[:2], system[0]):
        want = Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand()))
        got, public, flag, status, accounts = M.generate_account_update_proof(pk, c, tree, accounts, t["op"], M.generate_rand())
        assert got == want and public == want_public and (flag, status) == (1, 0) and accounts == t["table"]
        assert tree.root() == t["new_root"]
        assert L.verify_update(vk, public, got, M.generate_rand())
        for k in range(8):
            other = list(public)
            other[k] = (other[k] + 1) % R
            assert not L.verify_update(vk, other, got, M.generate_rand()), k
    # a refused operation has no proof and leaves tree and table alone
    none, public, flag, status, again = M.generate_account_update_proof(pk, c, tree, accounts, block[0]["op"], M.generate_rand())
    assert none is None and public[0] == public[1] == block[1]["new_root"] and (flag, status) == (0, AM.ST_OCCUPIED) and again == accounts
    # a key of another shape: refused before anything runs
    small = W.synthetic_circuit(32, 3, 5)
    srs = M.generate_universal_srs(64, 64, 256, M.generate_rand())
    other_pk, _ = M.generate_proving_and_verifying_keys(srs, small)
    srs.free()
    try:
        before = c.ctx.poseidon_tree_nodes(tree.h)
        with pytest.raises(M.MarlinError) as e:
            M.generate_account_update_proof(other_pk, c, tree, accounts, block[2]["op"], M.generate_rand())
        assert e.value.code == -8
        with pytest.raises(M.MarlinError) as e:
            M.generate_account_update_proofs(other_pk, c, tree, accounts, [block[2]["op"]], M.generate_rand())
        assert e.value.code == -8
        assert np.array_equal(c.ctx.poseidon_tree_nodes(tree.h), before) and tree.root() == block[1]["new_root"]
    finally:
        other_pk.free()
    # the prover is as it was for the next caller: the device source does not outlive the call
    cs = system[0][0][0]
    assert Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand())) == \
        Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand()))


def test_block_of_proofs_equals_single_calls(M, L, ref, circuits, world4, fresh_tree, keys):
    """swm_account_update_prove_many_at over [a registration, a refused one, the balance update]: lens = 0 for the refused one, and
    proofs, public inputs and the table are those of three single calls from the same rng state."""
    table, block = world4
    pk, vk = keys
    ops = [block[0]["op"], block[0]["op"], block[1]["op"]]
    c, tree, twin = circuits(4), fresh_tree(4, table), fresh_tree(4, table)
    proofs, public, flags, status, after = M.generate_account_update_proofs(pk, c, tree, table, ops, M.generate_rand())
    assert flags == [1, 0, 1] and status == [0, AM.ST_OCCUPIED, 0] and after == block[1]["table"]
    assert [p is not None for p in proofs] == [True, False, True] and tree.root() == block[1]["new_root"]
    assert public[1][0] == public[1][1] == public[0][1] == public[2][0]
    rng = M.generate_rand()
    accounts = table
    for op, proof, pub in zip(ops, proofs, public):
        single, pub1, _, _, accounts = M.generate_account_update_proof(pk, c, twin, accounts, op, rng)
        assert single == proof and pub1 == pub
        if proof is not None:
            assert L.verify_update(vk, pub, proof, M.generate_rand())
    assert accounts == after
    assert M.generate_account_update_proofs(pk, c, tree, after, [], M.generate_rand())[0] == []


def test_the_chain_from_the_blank_root(M, L, ref, ref_params):
    """A Poseidon State at height 4 from its blank root: three register_proved, two update_balance_proved, then one transfer through
    apply_transactions.  Every proof verifies, each proof's new_root is the next one's old_root, the first old_root is the blank
    tree's root and the last new_root is state.root()."""
    from simpleworks_amd import schnorr
    rng = M.generate_rand()
    pp = L.Parameters.sample(rng, poseidon=ref_params)
    state, twin = L.State(16, pp, account_tree="poseidon"), L.State(16, pp, account_tree="poseidon")
    try:
        assert state.account_merkle_tree.height() == 4
        blank_root = state.root()
        assert blank_root == T.blank(ref, 4)[-1][0]
        people = [schnorr.keygen(pp.sig_params, rng) for _ in range(3)]
        links = []      # (verifying key, verifier, public inputs, proof)
        vk = state.update_keys(rng)[2]
        for pub_key, _ in people:
            acc, proof, public = state.register_proved(pub_key, rng)
            assert acc == twin.register(pub_key) and public[2:] == [acc, pub_key[0], pub_key[1], 0, 0, 1]
            links.append((vk, L.verify_update, public, proof))
        for acc, amount in ((1, 10), (3, (1 << 64) - 2)):
            proof, public = state.update_balance_proved(acc, amount, rng)
            assert twin.update_balance(acc, amount) is True
            assert public[2:] == [acc, people[acc - 1][0][0], people[acc - 1][0][1], 0, amount, 0]
            links.append((vk, L.verify_update, public, proof))
        assert state.update_balance_proved(9, 1, rng) is None and state.next_available_account == twin.next_available_account == 4
        assert state.pub_key_to_id == twin.pub_key_to_id and state.root() == twin.root()
        tx = L.Transaction.create(pp, 1, 2, 4, people[0][1], rng)
        (applied, proof, public), = state.apply_transactions(pp, [tx], rng, prove=True)
        assert applied and twin.apply_transaction(pp, tx, rng, prove=False) is True
        links.append((state.transfer_keys(rng)[2], L.verify_transfer, public, proof))
        root = blank_root
        for key, verify, public, proof in links:
            assert proof is not None and verify(key, public, proof, rng)
            assert public[0] == root and public[1] != root
            root = public[1]
        assert root == state.root() == twin.root()
        assert {i: a.balance for i, a in state.id_to_account_info.items()} == {i: a.balance for i, a in twin.id_to_account_info.items()}
        # a block through apply_updates without proofs: a refused registration in the middle leaves the books as they were
        got = state.apply_updates(pp, [("balance", 2, 77), ("register", 2, people[0][0]), ("balance", 7, 1)], rng, prove=False)
        assert [g[:2] for g in got] == [(True, None), (False, None), (False, None)] and got[1][2][0] == got[1][2][1] == state.root()
        assert twin.update_balance(2, 77) is True and state.root() == twin.root() and state.id_to_account_info[2].balance == 77
        assert state.pub_key_to_id == twin.pub_key_to_id and state.next_available_account == 4
        pedersen = L.State(8, pp)
        try:
            with pytest.raises(ValueError):
                pedersen.apply_updates(pp, [("balance", 1, 1)], rng)
            with pytest.raises(ValueError):
                pedersen.update_keys(rng)
        finally:
            pedersen.free()
    finally:
        state.free()
        twin.free()
        pp.free()

"""The rollup entries (csrc/rollup_witness.hip) and State.apply_rollup on the GPU: ONE vector and ONE proof for a block of transfers,
all or nothing.  Against the circuit's specification workloads.build_rollup / build_pedersen_rollup run on the CPU over dependent
chains of tests/transfer_model.py and tests/pedersen_transfer_model.py: whole vectors in Montgomery limbs with 0xFF guard elements
behind them, proof bytes against generate_proof on the builder's system under keys made from workloads.rollup_system, the verifier
on changed public inputs; N = 1 against the transfer entries byte for byte; rolled-back blocks against the nodes and the table
before the call and against swm_transfer_witness_at on a twin tree; the refusals."""
import os

import numpy as np
import pytest

import pedersen_transfer_model as PTM
import poseidon_model as P
import transfer_model as TM

pytestmark = pytest.mark.gpu

R = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001
PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")
KEYS = ("message", "signature", "sender_leaf", "sender_path", "recipient_leaf", "recipient_path")
# height 2 holds the ids 0 (50) and 1 (1000): every transfer spends what the one before it credited
CHAIN_2 = [("zero to one", 0, 1, 50, None), ("one back, with the credit", 1, 0, 1030, None), ("zero spends it", 0, 1, 1000, None)]
# height 4 (transfer_model.CHAIN's accounts): 1 holds 1000, 2 holds 5, 3 holds 2^64 - 301
GOOD_4 = [("one to two", 1, 2, 600, None), ("two to three", 2, 3, 200, None), ("three to one", 3, 1, 100, None)]
BAD_SIGNATURE_4 = [GOOD_4[0], ("refused in the middle", 3, 1, 1, "signature"), GOOD_4[1]]
OVERDRAFT_4 = [GOOD_4[0], GOOD_4[1], ("overdrawn at the end", 2, 1, 406, "overdraft")]


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: %d witnesses differ, the first at %d" % (what, bad.size, bad[0])


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

    def get(height, n):
        if (height, n) not in made:
            made[(height, n)] = L.RollupCircuit(sig_params, sponge, height, n)
        return made[(height, n)]
    yield get
    for c in made.values():
        c.free()


@pytest.fixture(scope="module")
def world(ref):
    """(height, block) -> transfer_model.transfers of that block, made once and left unchanged."""
    seen = {}

    def get(height, which):
        k = (height, tuple(which))
        if k not in seen:
            seen[k] = TM.transfers(ref, height, which=list(which))
        return seen[k]
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
def built(M, W, ref_params, world):
    """(height, block) -> (the builder's system of the honest block, its witness as Montgomery limbs); built once."""
    seen = {}

    def get(height, which):
        k = (height, tuple(which))
        if k not in seen:
            block = world(height, which)[1]
            assert all(t["applied"] for t in block)
            cs, public = W.rollup_circuit(ref_params, height, block)
            assert public == W.rollup_public_inputs(block[0]["public"][0], block[-1]["public"][1], [t["message"] for t in block])
            seen[k] = (cs, M._to_mont_limbs(cs.witness))
        return seen[k]
    return get


def _check_vector(c, tree, first, block, want, guard=3):
    w, after, old, new, flags, status, applied = c.witness_at(tree, first, _pairs(block), guard=guard, fill=0xEE)
    assert applied and list(flags) == [31] * len(block) and list(status) == [0] * len(block)
    assert (old, new) == (block[0]["public"][0], block[-1]["public"][1]) and after == block[-1]["table"] and tree.root() == new
    n = c.shape()[1]
    assert w.shape == (n + guard, 4) and (w[n:].view(np.uint8) == 0xFF).all()        # nothing is stored behind the vector
    wt = c.transfer_shape()[1]
    for k in range(len(block)):      # first, middle and last section, then the whole vector with its linking roots
        _same(w[k * (wt + 1):k * (wt + 1) + wt], want[k * (wt + 1):k * (wt + 1) + wt], "section %d" % k)
    _same(w[:n], want, "the whole vector")


@pytest.mark.parametrize("height,which", [(2, CHAIN_2[:2]), (2, CHAIN_2), (4, GOOD_4[:2])], ids=["h2-n2", "h2-n3", "h4-n2"])
def test_whole_vector_against_the_builder(circuits, world, fresh_tree, built, height, which):
    first, block, _, _ = world(height, which)
    c, tree = circuits(height, len(block)), fresh_tree(height, first)
    _check_vector(c, tree, first, block, built(height, which)[1])


@pytest.fixture(scope="module")
def transfer_system(W, ref_params, world):
    """ONE packed transfer system at height 2: rollup_system relabels it for every block size."""
    t = world(2, CHAIN_2)[1][0]
    cs, _ = W.transfer_circuit(ref_params, 2, *[t[k] for k in KEYS])
    return cs, cs.pack()


@pytest.fixture(scope="module")
def keys(M, W, transfer_system):
    """n -> (pk, vk) of the rollup of n transfers at height 2, from the relabelled system."""
    made = {}

    def get(n):
        if n not in made:
            packed = W.rollup_system(transfer_system[1], n)
            nnz = max(int(m[0][-1]) for m in packed.mats)
            srs = M.MarlinInst.universal_setup(packed.num_constraints, packed.instance.shape[0] + packed.witness.shape[0], nnz, M.generate_rand())
            made[n] = M.MarlinInst.index_from_constraint_system(srs, packed)
            srs.free()
        return made[n]
    yield get
    for pk, _ in made.values():
        pk.free()


def test_one_transfer_is_the_transfer_entries_byte_for_byte(M, L, circuits, world, fresh_tree, keys, sig_params, sponge):
    first, block, _, _ = world(2, CHAIN_2)
    t = block[0]
    c, tree, twin = circuits(2, 1), fresh_tree(2, first), fresh_tree(2, first)
    plain = L.TransferCircuit(sig_params, sponge, 2)
    try:
        want, want_after, want_old, want_new, want_flags, want_status = plain.witness_at(twin, first, _pairs([t]))
        w, after, old, new, flags, status, applied = c.witness_at(tree, first, _pairs([t]))
        assert applied and w.tobytes() == want.tobytes() and after == want_after and ([old], [new]) == (want_old, want_new)
        assert list(flags) == list(want_flags) and list(status) == list(want_status) and tree.root() == twin.root()
        pk, vk = keys(1)
        tree, twin = fresh_tree(2, first), fresh_tree(2, first)
        single, single_public, _, _, single_after = M.generate_transfer_proof(pk, plain, twin, first, t["message"], t["signature"],
                                                                              M.generate_rand())
        proof, public, flags, status, after, applied = M.generate_rollup_proof(pk, c, tree, first, _pairs([t]), M.generate_rand())
        assert applied and proof == single and public == single_public and after == single_after and (flags, status) == ([31], [0])
        assert L.verify_rollup(vk, public, proof, M.generate_rand()) and L.verify_transfer(vk, public, proof, M.generate_rand())
    finally:
        plain.free()


@pytest.mark.parametrize("n", [2, 3])
def test_proof_equals_the_builders(M, L, circuits, world, fresh_tree, built, keys, n):
    """swm_rollup_prove_at is byte-identical to generate_proof on the builder's system from the same rng state, under a key made from
    the relabelled system; the proof verifies with its public inputs and with none of these changed: new_root, a swapped pair of
    transfers, an amount."""
    from simpleworks_amd import serialization as Ser
    which = CHAIN_2[:n]
    first, block, _, _ = world(2, which)
    cs, _ = built(2, which)
    pk, vk = keys(n)
    c, tree = circuits(2, n), fresh_tree(2, first)
    want = Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand()))
    got, public, flags, status, after, applied = M.generate_rollup_proof(pk, c, tree, first, _pairs(block), M.generate_rand())
    assert applied and got == want and [1] + public == cs.instance and (flags, status) == ([31] * n, [0] * n)
    assert after == block[-1]["table"] and tree.root() == block[-1]["public"][1] == public[1]
    assert L.verify_rollup(vk, public, got, M.generate_rand())
    wrong_root = [public[0], (public[1] + 1) % R] + public[2:]
    swapped = public[:2] + public[5:8] + public[2:5] + public[8:]
    amount = list(public)
    amount[4] = (amount[4] + 1) % R
    for other in (wrong_root, [public[0], public[0]] + public[2:], swapped, amount):
        assert other != public and not L.verify_rollup(vk, other, got, M.generate_rand())
    # the prover is as it was for the next caller: the device source does not outlive the call
    assert Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand())) == got


@pytest.mark.parametrize("which", [BAD_SIGNATURE_4, OVERDRAFT_4], ids=["bad signature in the middle", "overdraft at the end"])
def test_a_block_with_a_refused_transfer_is_rolled_back(L, circuits, world, fresh_tree, sig_params, sponge, which):
    first, block, _, _ = world(4, which)
    assert [t["applied"] for t in block].count(False) == 1
    c, tree, twin = circuits(4, 3), fresh_tree(4, first), fresh_tree(4, first)
    before = c.ctx.poseidon_tree_nodes(tree.h).copy()
    w, after, old, new, flags, status, applied = c.witness_at(tree, first, _pairs(block), fill=0xEE)
    assert not applied and after == first and old == new == block[0]["public"][0]
    assert np.array_equal(c.ctx.poseidon_tree_nodes(tree.h), before)       # byte for byte
    # flags and status are what the sequential pass met: swm_transfer_witness_at's for the same block on a twin tree
    plain = L.TransferCircuit(sig_params, sponge, 4)
    try:
        _, twin_after, _, _, twin_flags, twin_status = plain.witness_at(twin, first, _pairs(block))
        assert list(flags) == list(twin_flags) == [t["flag"] for t in block] and list(status) == list(twin_status)
        assert twin_after != first
        # the same tree then takes a good block and lands where a twin gets by the transfer entry
        good = world(4, GOOD_4)[1]
        twin2 = fresh_tree(4, first)
        _, want_after, _, want_new, _, _ = plain.witness_at(twin2, first, _pairs(good))
        w, after, old, new, flags, status, applied = c.witness_at(tree, first, _pairs(good))
        assert applied and after == want_after == good[-1]["table"] and new == want_new[-1] == tree.root() == twin2.root()
        assert np.array_equal(c.ctx.poseidon_tree_nodes(tree.h), c.ctx.poseidon_tree_nodes(twin2.h))
    finally:
        plain.free()


def test_a_rolled_back_block_has_no_proof(M, circuits, world, fresh_tree, keys):
    """swm_rollup_prove_at on a block whose last transfer is overdrawn: no proof, nothing changed."""
    which = CHAIN_2[:2] + [("overdrawn", 0, 1, 1031, "overdraft")]
    first, block, _, _ = world(2, which)
    assert [t["applied"] for t in block] == [True, True, False]
    pk, _ = keys(3)
    c, tree = circuits(2, 3), fresh_tree(2, first)
    before = c.ctx.poseidon_tree_nodes(tree.h).copy()
    proof, public, flags, status, after, applied = M.generate_rollup_proof(pk, c, tree, first, _pairs(block), M.generate_rand())
    assert proof is None and not applied and after == first and public[0] == public[1] == block[0]["public"][0]
    assert flags == [31, 31, 15 - 2] and status == [0, 0, 0]
    assert np.array_equal(c.ctx.poseidon_tree_nodes(tree.h), before)


def test_refusals(M, L, circuits, world, fresh_tree, keys):
    from simpleworks_amd._lib import SwmError
    first, block, _, _ = world(2, CHAIN_2)
    tree = fresh_tree(2, first)
    c3 = circuits(2, 3)
    before = c3.ctx.poseidon_tree_nodes(tree.h).copy()
    # N above 64
    c65 = circuits(2, 65)
    with pytest.raises(M.MarlinError):
        c65.shape()
    m = np.frombuffer(b"".join(t["message"] for t in block) * 22, dtype=np.uint8).reshape(-1, 10)[:65]
    s = np.frombuffer(b"".join(t["signature"] for t in block) * 22, dtype=np.uint8).reshape(-1, 64)[:65]
    acc = np.frombuffer(b"".join(first), dtype=np.uint8).reshape(-1, 72)
    with pytest.raises(SwmError) as e:
        c3.ctx.rollup_witness_at(c3.h, tree.h, 16, acc, m, s)
    assert e.value.code == -1 and "65 transfers" in str(e.value)
    # a count that differs from the key's N: refused before anything is advanced
    with pytest.raises(M.MarlinError) as e:
        M.generate_rollup_proof(keys(2)[0], c3, tree, first, _pairs(block), M.generate_rand())
    assert e.value.code == -8
    assert np.array_equal(c3.ctx.poseidon_tree_nodes(tree.h), before)
    # a block above the stage cap is not chunked: it is refused
    with c3.ctx.selftest_witness_stage(32 * c3.shape()[1] - 1):
        with pytest.raises(SwmError) as e:
            c3.witness_at(tree, first, _pairs(block))
        assert e.value.code == -1 and "not chunked" in str(e.value)
    # a table that is not the tree's
    wrong = [first[0], first[1][:64] + (6).to_bytes(8, "little")]
    with pytest.raises(SwmError) as e:
        c3.witness_at(tree, wrong, _pairs(block))
    assert e.value.code == -1 and "account table" in str(e.value)
    # a tree of another height, a block that is not the circuit's size
    with pytest.raises(SwmError):
        circuits(4, 3).ctx.rollup_witness_at(circuits(4, 3).h, tree.h, c3.shape()[1], acc, m[:3], s[:3])
    with pytest.raises(ValueError):
        c3.witness_at(tree, first, _pairs(block[:2]))
    assert np.array_equal(c3.ctx.poseidon_tree_nodes(tree.h), before)
    # and the same call with the right arguments goes through, with the cap at exactly the block's bytes
    with c3.ctx.selftest_witness_stage(32 * c3.shape()[1]):
        applied = c3.witness_at(tree, first, _pairs(block))[-1]
    assert applied and tree.root() == block[-1]["public"][1]


def test_the_ledger_applies_two_blocks(M, L, ref_params):
    """After two good blocks through State.apply_rollup the root and the balances are those of a twin state advanced by
    apply_transactions(prove=False); a block with a refused transaction leaves the state as it was."""
    from simpleworks_amd import schnorr
    rng = M.generate_rand()
    pp = L.Parameters.sample(rng, poseidon=ref_params)
    state, twin = L.State(16, pp, account_tree="poseidon"), L.State(16, pp, account_tree="poseidon")
    try:
        people = [schnorr.keygen(pp.sig_params, rng) for _ in range(3)]
        for s in (state, twin):
            assert [s.register(pk) for pk, _ in people] == [1, 2, 3]
            s.update_balance(1, 10)
        blocks = [[L.Transaction.create(pp, 1, 2, 4, people[0][1], rng), L.Transaction.create(pp, 2, 3, 3, people[1][1], rng)],
                  [L.Transaction.create(pp, 3, 1, 2, people[2][1], rng), L.Transaction.create(pp, 1, 2, 8, people[0][1], rng)]]
        balances = lambda s: {i: a.balance for i, a in s.id_to_account_info.items()}
        # a bad block first: the second transaction overdraws
        bad = [blocks[0][0], L.Transaction.create(pp, 2, 3, 5, people[1][1], rng)]
        root = state.root()
        applied, proof, public = state.apply_rollup(pp, bad, rng, prove=False)
        assert (applied, proof) == (False, None) and public[0] == public[1] == root == state.root() and balances(state) == balances(twin)
        vk = state.rollup_keys(2, rng)[2]
        for k, txs in enumerate(blocks):
            root = state.root()
            applied, proof, public = state.apply_rollup(pp, txs, rng, prove=k == 0)
            assert [g[0] for g in twin.apply_transactions(pp, txs, rng, prove=False)] == [True, True]
            assert applied and (proof is not None) == (k == 0)
            assert public == [root, state.root()] + [v for tx in txs for v in (tx.sender, tx.recipient, tx.amount)]
            assert state.root() == twin.root() and balances(state) == balances(twin)
            if proof is not None:
                assert L.verify_rollup(vk, public, proof, rng)
                assert not L.verify_rollup(vk, [public[0], public[0]] + public[2:], proof, rng)
        assert balances(state) == {1: 0, 2: 9, 3: 1}
        assert state.rollup_keys(2, rng)[1] is state.rollup_keys(2, rng)[1]       # cached per n
        with pytest.raises(ValueError):
            state.pedersen_rollup_keys(2, rng)
        with pytest.raises(ValueError):
            state.apply_rollup(pp, [], rng)
    finally:
        state.free()
        twin.free()
        pp.free()


# ---- the Pedersen tree

@pytest.fixture(scope="module")
def merkle(W):
    return W.MerkleParams()


@pytest.fixture(scope="module")
def crh(merkle):
    from simpleworks_amd import hash as H
    made = (H.PedersenCRH(merkle.leaf_gens), H.PedersenCRH(merkle.inner_gens))
    yield made
    for c in made:
        c.free()


@pytest.fixture(scope="module")
def pedersen_circuits(L, sig_params, crh):
    made = {}

    def get(n):
        if n not in made:
            made[n] = L.PedersenRollupCircuit(sig_params, crh[0], crh[1], 2, n)
        return made[n]
    yield get
    for c in made.values():
        c.free()


@pytest.fixture
def fresh_pedersen_tree(crh):
    from simpleworks_amd import hash as H
    made = []

    def get(table):
        tree = H.DeviceMerkleTree.blank(crh[0], crh[1], 2, 72)
        held = [i for i, leaf in enumerate(table) if any(leaf)]
        tree.update_many(held, [table[i] for i in held])
        made.append(tree)
        return tree
    yield get
    for t in made:
        t.free()


@pytest.fixture(scope="module")
def pedersen_built(M, W, merkle):
    """n -> (initial table, block, the builder's system, its witness as Montgomery limbs) of the chain's first n transfers."""
    seen = {}

    def get(n):
        if n not in seen:
            first, block, _, _ = PTM.transfers(merkle, 2, which=CHAIN_2[:n])
            assert all(t["applied"] for t in block)
            cs, _ = W.pedersen_rollup_circuit(merkle, 2, block)
            seen[n] = (first, block, cs, M._to_mont_limbs(cs.witness))
        return seen[n]
    return get


@pytest.mark.parametrize("n", [2, 3])
def test_pedersen_whole_vector_against_the_builder(pedersen_circuits, fresh_pedersen_tree, pedersen_built, n):
    first, block, _, want = pedersen_built(n)
    _check_vector(pedersen_circuits(n), fresh_pedersen_tree(first), first, block, want)


def test_pedersen_proof_equals_the_builders(M, W, L, merkle, pedersen_circuits, fresh_pedersen_tree, pedersen_built):
    from simpleworks_amd import serialization as Ser
    first, block, cs, _ = pedersen_built(2)
    one, _ = PTM.build(merkle, 2, block[1])
    packed = W.rollup_system(one, 2)
    nnz = max(int(m[0][-1]) for m in packed.mats)
    srs = M.MarlinInst.universal_setup(packed.num_constraints, packed.instance.shape[0] + packed.witness.shape[0], nnz, M.generate_rand())
    pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
    srs.free()
    try:
        c, tree = pedersen_circuits(2), fresh_pedersen_tree(first)
        want = Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand()))
        got, public, flags, status, after, applied = M.generate_pedersen_rollup_proof(pk, c, tree, first, _pairs(block), M.generate_rand())
        assert applied and got == want and [1] + public == cs.instance and (flags, status) == ([31, 31], [0, 0])
        assert after == block[-1]["table"] and tree.root() == public[1]
        assert L.verify_rollup(vk, public, got, M.generate_rand())
        assert not L.verify_rollup(vk, [public[0], public[0]] + public[2:], got, M.generate_rand())
    finally:
        pk.free()


def test_pedersen_block_with_a_refused_transfer_is_rolled_back(L, pedersen_circuits, fresh_pedersen_tree, merkle, sig_params, crh):
    which = [CHAIN_2[0], ("flipped signature", 1, 0, 3, "signature"), ("one to zero", 1, 0, 5, None)]
    first, block, _, _ = PTM.transfers(merkle, 2, which=which)
    assert [t["applied"] for t in block] == [True, False, True]
    c, tree, twin = pedersen_circuits(3), fresh_pedersen_tree(first), fresh_pedersen_tree(first)
    before = c.ctx.merkle_tree_nodes(tree.h).copy()
    w, after, old, new, flags, status, applied = c.witness_at(tree, first, _pairs(block), fill=0xEE)
    assert not applied and after == first and old == new == block[0]["public"][0]
    assert np.array_equal(c.ctx.merkle_tree_nodes(tree.h), before)
    plain = L.PedersenTransferCircuit(sig_params, crh[0], crh[1], 2)
    try:
        _, _, _, _, twin_flags, twin_status = plain.witness_at(twin, first, _pairs(block))
        assert list(flags) == list(twin_flags) == [31, 15 - 1, 31] and list(status) == list(twin_status)
    finally:
        plain.free()
    good = PTM.transfers(merkle, 2, which=CHAIN_2)[1]
    applied = c.witness_at(tree, first, _pairs(good))[-1]
    assert applied and tree.root() == good[-1]["public"][1]

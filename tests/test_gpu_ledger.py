"""The ledger (simpleworks_amd/ledger.py) on the GPU: the end_to_end scenario of examples/simple-payments/ledger.rs:201-250, once
with the Marlin proof of the signature circuit, and validate_many against validate one by one.  After every state change the
account tree's nodes equal those of a tree made independently of the State: blank, then one update per account with the
account's 72-byte leaf, at the same height."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from simpleworks_amd import ledger
    return ledger


@pytest.fixture(scope="module")
def world(L):
    """Parameters::sample from a fresh test_rng, and the keys of Alice and Bob, made once."""
    from simpleworks_amd import marlin as M, schnorr
    rng = M.generate_rand()
    pp = L.Parameters.sample(rng)
    alice = schnorr.keygen(pp.sig_params, rng)
    bob = schnorr.keygen(pp.sig_params, rng)
    yield pp, rng, alice, bob
    pp.free()


def _expected_nodes(L, pp, height, accounts):
    """accounts: {id: (public key, balance)} -> the nodes of blank + per-leaf update."""
    from simpleworks_amd import hash as H
    tree = H.DeviceMerkleTree.blank(pp.leaf_crh, pp.two_to_one_crh, height, 72)
    for acc, (key, balance) in sorted(accounts.items()):
        tree.update(acc, L.AccountInformation(key, balance).to_bytes_le())
    nodes = tree.ctx.merkle_tree_nodes(tree.h)
    tree.free()
    return nodes


def _state_nodes(state):
    tree = state.account_merkle_tree
    return tree.ctx.merkle_tree_nodes(tree.h)


def _scenario(L, world, num_accounts):
    """Alice (10) and Bob (0) registered in a fresh State -> (state, alice id, bob id, the accounts as a plain dict)."""
    pp, rng, (alice_pk, alice_sk), (bob_pk, bob_sk) = world
    state = L.State(num_accounts, pp)
    height = state.account_merkle_tree.height()
    accounts = {}
    assert np.array_equal(_state_nodes(state), _expected_nodes(L, pp, height, accounts))
    alice_id = state.register(alice_pk)
    accounts[alice_id] = (alice_pk, 0)
    assert alice_id == 1 and np.array_equal(_state_nodes(state), _expected_nodes(L, pp, height, accounts))
    assert state.update_balance(alice_id, 10) is True
    accounts[alice_id] = (alice_pk, 10)
    assert np.array_equal(_state_nodes(state), _expected_nodes(L, pp, height, accounts))
    bob_id = state.register(bob_pk)
    accounts[bob_id] = (bob_pk, 0)
    assert bob_id == 2 and np.array_equal(_state_nodes(state), _expected_nodes(L, pp, height, accounts))
    assert state.update_balance(9, 1) is None
    return state, alice_id, bob_id, accounts


def test_end_to_end_with_proofs(L, world):
    """ledger.rs:201-250 at height 3 (State::new(8)): a transfer of 5 validates and applies; 6 from the remaining 5, Bob's key on
    Alice's transaction and recipient 10 do not validate, and apply_transaction returns None for each."""
    pp, rng, (alice_pk, alice_sk), (bob_pk, bob_sk) = world
    state, alice_id, bob_id, accounts = _scenario(L, world, 8)
    assert state.account_merkle_tree.height() == 3
    tx1 = L.Transaction.create(pp, alice_id, bob_id, 5, alice_sk, rng)
    assert len(tx1.message()) == 10
    assert tx1.validate(pp, state, rng) is True
    root_before = state.root()
    assert state.apply_transaction(pp, tx1, rng) is True
    accounts[alice_id], accounts[bob_id] = (alice_pk, 5), (bob_pk, 5)
    assert np.array_equal(_state_nodes(state), _expected_nodes(L, pp, 3, accounts))
    assert state.root() != root_before
    assert state.id_to_account_info[alice_id].balance == 5 and state.id_to_account_info[bob_id].balance == 5
    bad = [L.Transaction.create(pp, alice_id, bob_id, 6, alice_sk, rng),      # more than Alice has left
           L.Transaction.create(pp, alice_id, bob_id, 5, bob_sk, rng),        # not Alice's signature
           L.Transaction.create(pp, alice_id, 10, 5, alice_sk, rng)]          # no such recipient
    for tx in bad:
        assert tx.validate(pp, state, rng) is False
        assert state.apply_transaction(pp, tx, rng) is None
        assert np.array_equal(_state_nodes(state), _expected_nodes(L, pp, 3, accounts))
    # a sender without an account: the reference's Err, and None from apply_transaction
    ghost = L.Transaction.create(pp, 7, bob_id, 1, alice_sk, rng)
    with pytest.raises(KeyError):
        ghost.validate(pp, state, rng)
    assert state.apply_transaction(pp, ghost, rng) is None
    # the block form against one state: the same four answers, with and without proofs
    block = [L.Transaction.create(pp, alice_id, bob_id, 5, alice_sk, rng)] + bad
    one_by_one = [tx.validate(pp, state, rng, prove=False) for tx in block]
    assert one_by_one == [True, False, False, False]
    assert L.validate_many(pp, state, block) == one_by_one
    assert L.validate_many(pp, state, block + [ghost], rng, prove=True) == one_by_one + [False]
    assert L.validate_many(pp, state, []) == []
    assert np.array_equal(_state_nodes(state), _expected_nodes(L, pp, 3, accounts))
    state.free()


def test_32_accounts_give_16_leaves_and_registering_past_them_raises(L, world):
    """ledger.rs:106-112 hands log2(num_accounts) to MerkleTree::blank as a height."""
    pp, rng, (alice_pk, _), (bob_pk, _) = world
    state, alice_id, bob_id, accounts = _scenario(L, world, 32)
    tree = state.account_merkle_tree
    assert tree.height() == 5 and len(_state_nodes(state)) == 31
    for acc in range(3, 16):
        assert state.register(bob_pk) == acc
    assert state.pub_key_to_id[bob_pk] == 15
    before = _state_nodes(state)
    with pytest.raises(IndexError):
        state.register(alice_pk)
    assert np.array_equal(_state_nodes(state), before) and state.next_available_account == 16
    state.free()

"""The account-update entries on a CALLER's stream, in the manner of tests/test_gpu_stream_order.py (whose harness this module
uses): swm_account_update_witness_at and swm_account_update_prove_many_at take host arrays and hand host results back, so they WAIT;
what they read on the device is the resident tree.  Here the context runs on the caller's torch stream, the tree's node buffer holds
0xFF bytes (no field element, and not the table's leaf level) until, behind a GATE on that stream, the nodes are copied in; then the
entry is called, and a snapshot of the nodes is taken behind it on the same stream.  The host waits for the caller's stream alone.
An entry whose launches or copies were not ordered behind the caller's stream would read 0xFF nodes and refuse the table; one whose
work was not joined back into the stream would leave the old nodes in the snapshot.  The expectation is the model
(tests/account_update_model.py) and the builder, never a second call of the entry."""
import os

import numpy as np
import pytest

import account_update_model as AM
import poseidon_model as P
import poseidon_tree_model as T
from test_gpu_stream_order import Env, WAITS, _same_rows

pytestmark = pytest.mark.gpu

PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")
HEIGHT = 4


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


@pytest.fixture(scope="module")
def ref():
    return P.load_params(PARAMS)


@pytest.fixture(scope="module")
def sponge(env):
    from simpleworks_amd import hash as H
    s = H.PoseidonSponge(H.PoseidonParameters.from_json(PARAMS), env.ctx)
    yield s
    s.free()


@pytest.fixture(scope="module")
def circuit(sponge):
    from simpleworks_amd import ledger as L
    c = L.AccountUpdateCircuit(sponge, HEIGHT)
    yield c
    c.free()


@pytest.fixture(scope="module")
def world(ref):
    """(the table two accounts in, its tree's levels, a block of four operations on it with a refusal, the model's results)."""
    table, levels = AM.blank(ref, HEIGHT)
    _, first, levels = AM.apply(ref, HEIGHT, table, levels, [(1, AM.REGISTER, AM.key(1), 3), (6, AM.REGISTER, AM.key(6), 0)])
    ops = [(7, AM.REGISTER, AM.key(7), 0), (6, AM.SET, AM.NO_KEY, 41), (6, AM.REGISTER, AM.key(2), 0), (7, AM.SET, AM.NO_KEY, 5)]
    block, final, after = AM.apply(ref, HEIGHT, first, levels, ops)
    assert [t["applied"] for t in block] == [True, True, False, True]
    return first, levels, ops, block, final, after


def _node_rows(levels):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in T.nodes(levels)), dtype=np.uint8).reshape(-1, 32)


def _trees(sponge, first):
    from simpleworks_amd import hash as H
    out = []
    for _ in range(2):
        tree = H.PoseidonMerkleTree.blank(sponge, HEIGHT, 72)
        held = [i for i, leaf in enumerate(first) if any(leaf)]
        tree.update_many(held, [first[i] for i in held])
        out.append(tree)
    return out


def test_witness_at_behind_a_busy_stream(env, sponge, circuit, world):
    from test_gpu_account_update import _WitnessOnly
    from simpleworks_amd import marlin as M, workloads as W
    first, levels, ops, block, final, after = world
    tree, other = _trees(sponge, first)
    try:
        ptr, count = env.ctx.poseidon_tree_dev_nodes(tree.h)
        nodes = env.alias(ptr, count * 32)
        src = env.pinned(_node_rows(levels))
        snap, = env.run("account_update_witness_at 4", [(nodes, src)], lambda: circuit.witness_at(tree, first, ops), [], mode=WAITS,
                        warm=lambda: circuit.witness_at(other, first, ops), late_outs=lambda _: [nodes], late_bytes=[count * 32])
        w, table, old, new, flags, status = env.result
        assert list(flags) == [1, 1, 0, 1] and list(status) == [t["status"] for t in block] and table == final
        assert old == [t["old_root"] for t in block] and new == [t["new_root"] for t in block]
        _same_rows(snap, _node_rows(after), "the nodes behind the call")
        for k, t in enumerate(block):
            if not t["applied"]:
                assert not w[k].any()
                continue
            cs = _WitnessOnly()
            W.build_account_update(cs, sponge.params, HEIGHT, t["id"], t["key"], t["old_balance"], t["new_balance"], t["fresh"], t["path"])
            assert np.array_equal(w[k], M._to_mont_limbs(cs.witness)), k
    finally:
        tree.free()
        other.free()


def test_prove_many_at_behind_a_busy_stream(env, sponge, circuit, world):
    from simpleworks_amd import ledger as L, marlin as M, workloads as W
    first, levels, ops, block, final, after = world
    t = block[0]
    cs, _ = W.account_update_circuit(sponge.params, HEIGHT, t["id"], t["key"], t["old_balance"], t["new_balance"], t["fresh"], t["path"])
    packed = cs.pack()
    srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), max(int(m[0][-1]) for m in packed.mats),
                                       M.generate_rand(), env.ctx)
    pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
    srs.free()
    tree, other = _trees(sponge, first)
    try:
        ptr, count = env.ctx.poseidon_tree_dev_nodes(tree.h)
        nodes = env.alias(ptr, count * 32)
        src = env.pinned(_node_rows(levels))
        snap, = env.run("account_update_prove_many_at 4", [(nodes, src)],
                        lambda: M.generate_account_update_proofs(pk, circuit, tree, first, ops, M.generate_rand()), [], mode=WAITS,
                        warm=lambda: M.generate_account_update_proofs(pk, circuit, other, first, ops, M.generate_rand()),
                        late_outs=lambda _: [nodes], late_bytes=[count * 32])
        proofs, public, flags, status, table = env.result
        assert flags == [1, 1, 0, 1] and status == [t["status"] for t in block] and table == final
        assert [p[:2] for p in public] == [[t["old_root"], t["new_root"]] for t in block]
        _same_rows(snap, _node_rows(after), "the nodes behind the call")
        for proof, pub, t in zip(proofs, public, block):
            assert (proof is not None) == t["applied"]
            if proof is not None:
                assert L.verify_update(vk, pub, proof, M.generate_rand())
    finally:
        tree.free()
        other.free()
        pk.free()

"""The Pedersen account-update entries on a CALLER's stream, in the manner of tests/test_gpu_account_update_stream_order.py (and
with the harness of tests/test_gpu_stream_order.py): swm_pedersen_account_update_witness_at and
swm_pedersen_account_update_prove_many_at take host arrays and hand host results back, so they WAIT; what they read on the device is
the resident tree.  Here the context runs on the caller's torch stream, the tree's node buffer holds 0xFF bytes (no field element,
and not the table's leaf level) until, behind a GATE on that stream, the nodes are copied in; then the entry is called, and a
snapshot of the nodes is taken behind it on the same stream.  The host waits for the caller's stream alone.  An entry whose launches
or copies were not ordered behind the caller's stream would read 0xFF nodes and refuse the table; one whose work was not joined back
into the stream would leave the old nodes in the snapshot.  The expectation is the model (tests/pedersen_account_update_model.py)
and the builder, never a second call of the entry."""
import ctypes

import numpy as np
import pytest

import pedersen_account_update_model as AM
from test_gpu_stream_order import Env, WAITS, _same_rows

pytestmark = pytest.mark.gpu

HEIGHT = 3


class _OwnStreamsEnv(Env):
    """Env with two streams of its own, made with hipStreamCreate and destroyed in close().  Env takes its streams from torch's
    pool, which keeps them for the life of the process: every module that makes an Env leaves two more live streams behind, and
    which hardware queue a later stream lands on depends on how many there are — with this module's two on top of
    tests/test_gpu_account_update_stream_order.py's, the library's own stream and the gated stream of
    test_gpu_stream_order.py::test_d_set_stream_waits_for_pending_work_and_lets_go_of_the_callers_stream came to share a queue.
    This module leaves the process as it found it."""

    def __init__(self):
        import torch
        import simpleworks_amd as swm
        self.torch = torch
        self.ctx = swm.Context(0)      # the HIP runtime is loaded and initialised from here on
        with open("/proc/self/maps") as f:
            path = next(line.split()[-1] for line in f if "libamdhip64" in line)
        self._hip = ctypes.CDLL(path)  # the runtime torch and the library already use: the same handle
        self._raw = []
        for _ in range(2):
            p = ctypes.c_void_p()
            assert self._hip.hipStreamCreate(ctypes.byref(p)) == 0
            self._raw.append(p)
        self.s, self.s2 = (torch.cuda.ExternalStream(p.value) for p in self._raw)
        self.ctx.set_stream(self.s.cuda_stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.s):
            torch.cuda._sleep(1000000)            # loads the kernel
            e0.record()
            torch.cuda._sleep(20000000)
            e1.record()
        self.s.synchronize()
        self.cycles_per_ms = 20000000 / e0.elapsed_time(e1)

    def close(self):
        super().close()
        self.torch.cuda.synchronize()
        for p in self._raw:
            assert self._hip.hipStreamDestroy(p) == 0
        self._raw = []


@pytest.fixture(scope="module")
def env():
    e = _OwnStreamsEnv()
    yield e
    e.close()


@pytest.fixture(scope="module")
def params():
    from simpleworks_amd import workloads as W
    return W.MerkleParams()


@pytest.fixture(scope="module")
def crh(env, params):
    from simpleworks_amd import hash as H
    made = (H.PedersenCRH(params.leaf_gens, env.ctx), H.PedersenCRH(params.inner_gens, env.ctx))
    yield made
    for c in made:
        c.free()


@pytest.fixture(scope="module")
def circuit(crh):
    from simpleworks_amd import ledger as L
    c = L.PedersenAccountUpdateCircuit(crh[0], crh[1], HEIGHT)
    yield c
    c.free()


@pytest.fixture(scope="module")
def world(params):
    """(the table two accounts in, its tree's levels, a block of four operations on it with a refusal, the model's results)."""
    table, levels = AM.blank(params, HEIGHT)
    _, first, levels = AM.apply(params, HEIGHT, table, levels, [(1, AM.REGISTER, AM.key(1), 3), (2, AM.REGISTER, AM.key(2), 0)])
    ops = [(3, AM.REGISTER, AM.key(3), 0), (2, AM.SET, AM.NO_KEY, 41), (2, AM.REGISTER, AM.key(5), 0), (3, AM.SET, AM.NO_KEY, 5)]
    block, final, after = AM.apply(params, HEIGHT, first, levels, ops)
    assert [t["applied"] for t in block] == [True, True, False, True]
    return first, levels, ops, block, final, after


def _node_rows(levels):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for level in levels for v in level), dtype=np.uint8).reshape(-1, 32)


def _trees(crh, first):
    from simpleworks_amd import hash as H
    out = []
    for _ in range(2):
        tree = H.DeviceMerkleTree.blank(crh[0], crh[1], HEIGHT, 72)
        held = [i for i, leaf in enumerate(first) if any(leaf)]
        tree.update_many(held, [first[i] for i in held])
        out.append(tree)
    return out


def test_witness_at_behind_a_busy_stream(env, params, crh, circuit, world):
    from test_gpu_pedersen_account_update import _WitnessOnly
    from simpleworks_amd import marlin as M, workloads as W
    first, levels, ops, block, final, after = world
    tree, other = _trees(crh, first)
    try:
        ptr, count = env.ctx.merkle_tree_dev_nodes(tree.h)
        nodes = env.alias(ptr, count * 32)
        src = env.pinned(_node_rows(levels))
        snap, = env.run("pedersen_account_update_witness_at 4", [(nodes, src)], lambda: circuit.witness_at(tree, first, ops), [], mode=WAITS,
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
            W.build_pedersen_account_update(cs, params, HEIGHT, t["id"], t["key"], t["old_balance"], t["new_balance"], t["fresh"], t["path"],
                                            old_root=t["old_root"], new_root=t["new_root"])
            assert np.array_equal(w[k], M._to_mont_limbs(cs.witness)), k
    finally:
        tree.free()
        other.free()


def test_prove_many_at_behind_a_busy_stream(env, params, crh, circuit, world):
    from simpleworks_amd import ledger as L, marlin as M
    first, levels, ops, block, final, after = world
    cs, _ = AM.build(params, HEIGHT, block[0])
    packed = cs.pack()
    srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), max(int(m[0][-1]) for m in packed.mats),
                                       M.generate_rand(), env.ctx)
    pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
    srs.free()
    tree, other = _trees(crh, first)
    try:
        ptr, count = env.ctx.merkle_tree_dev_nodes(tree.h)
        nodes = env.alias(ptr, count * 32)
        src = env.pinned(_node_rows(levels))
        snap, = env.run("pedersen_account_update_prove_many_at 4", [(nodes, src)],
                        lambda: M.generate_pedersen_account_update_proofs(pk, circuit, tree, first, ops, M.generate_rand()), [], mode=WAITS,
                        warm=lambda: M.generate_pedersen_account_update_proofs(pk, circuit, other, first, ops, M.generate_rand()),
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

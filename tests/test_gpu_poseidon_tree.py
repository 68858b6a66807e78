"""The resident Poseidon Merkle tree (csrc/poseidon_tree.hip) and the membership circuit's witness and proof entries
(csrc/poseidon_tree_witness.hip) on the GPU, against the big-integer model tests/poseidon_tree_model.py and the circuit's
specification workloads.build_poseidon_membership run on the CPU: ALL nodes after every build and update, whole witness vectors in
Montgomery limbs, proof bytes against generate_proof on the builder's system.  Sizes are the smallest at which each kernel can go
wrong: 64 | 128 leaves is the one-workgroup | two-workgroup edge, 64 | 65 dirty nodes the finishing wave | index-list edge."""
import os

import numpy as np
import pytest

import poseidon_model as P
import poseidon_tree_model as T

pytestmark = pytest.mark.gpu

R = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001
PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")
LEAF_LENS = (1, 23, 24, 54, 55, 72)


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


def ints(a):
    return [int.from_bytes(r.tobytes(), "little") for r in np.asarray(a).reshape(-1, 32)]


def rows(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(len(values), 32).copy()


@pytest.fixture(scope="module")
def M():
    from simpleworks_amd import marlin
    return marlin


@pytest.fixture(scope="module")
def W():
    from simpleworks_amd import workloads
    return workloads


@pytest.fixture(scope="module")
def HASH():
    from simpleworks_amd import hash
    return hash


@pytest.fixture(scope="module")
def ref():
    return P.load_params(PARAMS)


@pytest.fixture(scope="module")
def ref_params(HASH):
    return HASH.PoseidonParameters.from_json(PARAMS)


@pytest.fixture(scope="module")
def sponge(HASH, ref_params):
    s = HASH.PoseidonSponge(ref_params)
    yield s
    s.free()


@pytest.fixture(scope="module")
def model_tree(ref):
    """(leaf_len, n) -> (leaves, model levels), built once and never changed: callers copy before updating."""
    seen = {}

    def get(leaf_len, n):
        if (leaf_len, n) not in seen:
            leaves = [T.leaf(leaf_len, i) for i in range(n)]
            seen[(leaf_len, n)] = (leaves, T.build(ref, leaves))
        return seen[(leaf_len, n)]
    return get


def _nodes(tree):
    return ints(tree.ctx.poseidon_tree_nodes(tree.h))


@pytest.mark.parametrize("height", [2, 3, 9])
def test_blank(HASH, ref, sponge, height):
    tree = HASH.PoseidonMerkleTree.blank(sponge, height, 72)
    try:
        want = T.blank(ref, height)
        assert _nodes(tree) == T.nodes(want)
        assert tree.root() == want[-1][0] and tree.height() == height
        assert tree.ctx.poseidon_tree_dev_nodes(tree.h)[1] == (1 << height) - 1
    finally:
        tree.free()


@pytest.mark.parametrize("leaf_len", LEAF_LENS)
@pytest.mark.parametrize("n", [2, 64, 128, 256])
def test_from_leaves_every_node(HASH, sponge, model_tree, n, leaf_len):
    leaves, want = model_tree(leaf_len, n)
    tree = HASH.PoseidonMerkleTree.new(sponge, leaves)
    try:
        assert _nodes(tree) == T.nodes(want)
        assert tree.height() == n.bit_length() and tree.root() == want[-1][0]
        down = tree.to_merkle_tree()
        assert down.root() == want[-1][0] and down.generate_proof(n - 1) == T.path(want, n - 1)
    finally:
        tree.free()


def test_level_one_is_the_sponges_two_to_one_hash(HASH, sponge, model_tree):
    leaves, want = model_tree(24, 64)
    tree = HASH.PoseidonMerkleTree.new(sponge, leaves)
    try:
        nodes = tree.ctx.poseidon_tree_nodes(tree.h)
        pairs = nodes[:64].reshape(32, 2, 32)
        assert np.array_equal(sponge.hash_elements_many(pairs).reshape(32, 32), nodes[64:96])
        assert np.array_equal(sponge.hash_many(np.frombuffer(b"".join(leaves), dtype=np.uint8).reshape(64, 24)), nodes[:64])
    finally:
        tree.free()


@pytest.fixture(scope="module")
def tree9(HASH, sponge, model_tree):
    """A height-9 tree of 55-byte leaves and its model, updated in step by the tests below."""
    leaves, levels = model_tree(55, 256)
    tree = HASH.PoseidonMerkleTree.new(sponge, leaves)
    state = {"tree": tree, "model": [list(level) for level in levels], "round": 0}
    yield state
    tree.free()


def _update_and_compare(ref, state, indices):
    state["round"] += 1
    leaves = [T.leaf(55, i, 100 * state["round"] + k) for k, i in enumerate(indices)]
    state["tree"].update_many(indices, leaves)
    T.update(ref, state["model"], indices, leaves)
    assert _nodes(state["tree"]) == T.nodes(state["model"])
    assert state["tree"].root() == state["model"][-1][0]


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 129])
def test_update_distinct_leaves(ref, tree9, k):
    """k <= 64: the leaf launch and the finishing wave from level 0; 65 and 129: index-list launches first."""
    stride = {1: 1, 2: 255, 63: 4, 64: 3, 65: 3, 129: 1}[k]
    indices = [(7 + stride * j) % 256 for j in range(k)]
    assert len(set(indices)) == k
    _update_and_compare(ref, tree9, indices)


def test_update_repeated_index_siblings_and_the_two_ends(ref, tree9):
    _update_and_compare(ref, tree9, [5, 9, 5, 200, 5])          # last writer wins
    _update_and_compare(ref, tree9, [10, 11])                   # both children of one parent
    _update_and_compare(ref, tree9, [0, 255])                   # leaf 0 and leaf n - 1
    _update_and_compare(ref, tree9, [255])
    _update_and_compare(ref, tree9, [0])                        # two updates in a row
    _update_and_compare(ref, tree9, list(range(256)))           # every leaf: every level behind a list down to 64
    _update_and_compare(ref, tree9, [2 * j for j in range(128)] + [1])


def test_update_refusals_leave_the_tree(tree9):
    from simpleworks_amd._lib import SwmError
    tree = tree9["tree"]
    before = _nodes(tree)
    with pytest.raises(SwmError) as e:
        tree.update_many([3, 256], [T.leaf(55, 0), T.leaf(55, 1)])
    assert e.value.code == -1 and "256" in str(e.value)
    with pytest.raises(SwmError) as e:
        tree.update_many([3], [T.leaf(54, 0)])
    assert e.value.code == -1
    assert tree.ctx.lib.swm_poseidon_tree_update(tree.ctx.h, tree.h, None, None, 55, 0) == 0
    assert _nodes(tree) == before
    for height, leaf_len in ((1, 1), (32, 1), (4, 0), (4, 65537)):
        with pytest.raises(SwmError):
            tree.ctx.poseidon_tree_create_blank(tree.sponge.h, height, leaf_len)


@pytest.mark.parametrize("count", [1, 65])
def test_paths(HASH, sponge, model_tree, count):
    from simpleworks_amd._lib import SwmError
    leaves, want = model_tree(72, 128)
    tree = HASH.PoseidonMerkleTree.new(sponge, leaves)
    try:
        indices = [(37 * j + 127) % 128 for j in range(count)]
        got = tree.generate_proofs(indices)
        assert got.shape == (count, 7, 32)
        for p, i in enumerate(indices):
            assert ints(got[p]) == T.path(want, i)
        assert tree.generate_proof(indices[0]) == T.path(want, indices[0])
        with pytest.raises(SwmError) as e:
            tree.generate_proofs([0, 128])
        assert e.value.code == -1
    finally:
        tree.free()


def test_verify_paths(HASH, ref, sponge, model_tree):
    count, n, height = 65, 128, 8
    leaves, want = model_tree(72, n)
    root = want[-1][0]
    indices = [(37 * j + 127) % n for j in range(count)]
    sib = np.stack([rows(T.path(want, i)) for i in indices])
    mine = [leaves[i] for i in indices]

    def run(roots, lv=mine, idx=indices, s=sib):
        ok, status = HASH.verify_poseidon_paths(sponge, height, roots, lv, idx, s, with_status=True)
        return [bool(v) for v in ok], [int(v) for v in status]
    assert run(root) == ([True] * count, [0] * count)
    assert run([root] * count) == ([True] * count, [0] * count)
    # per-path roots of which one is another tree's
    other = T.root_of(ref, b"x" * 72, 0, T.path(want, 0))
    assert run([other if p == 64 else root for p in range(count)])[0] == [p != 64 for p in range(count)]
    # one flipped sibling byte, a wrong index, a wrong leaf: that path alone
    s = sib.copy()
    s[3, 5, 0] ^= 1
    assert run(root, s=s) == ([p != 3 for p in range(count)], [0] * count)
    idx = list(indices)
    idx[64] ^= 2
    assert run(root, idx=idx)[0] == [p != 64 for p in range(count)]
    lv = list(mine)
    lv[0] = b"\x00" * 72
    assert run(root, lv=lv)[0] == [p != 0 for p in range(count)]
    assert run((root + 1) % R) == ([False] * count, [0] * count)
    # status 1: a sibling = r, a root = r; status 2: an index = 2^L; the rest of the batch unaffected
    s = sib.copy()
    s[7, 6] = rows([R])[0]
    idx = list(indices)
    idx[9] = n
    roots = [R if p == 11 else root for p in range(count)]
    ok, status = run(roots, idx=idx, s=s)
    assert status == [1 if p in (7, 11) else 2 if p == 9 else 0 for p in range(count)]
    assert ok == [p not in (7, 9, 11) for p in range(count)]
    assert HASH.verify_poseidon_paths(sponge, height, root, [], [], np.zeros((0, 7, 32), dtype=np.uint8)).shape == (0,)


# ---- the membership circuit's witness
@pytest.fixture(scope="module")
def circuits(HASH, sponge):
    made = {}

    def get(height, leaf_len):
        if (height, leaf_len) not in made:
            made[(height, leaf_len)] = HASH.PoseidonMembershipCircuit(sponge, height, leaf_len)
        return made[(height, leaf_len)]
    yield get
    for c in made.values():
        c.free()


@pytest.fixture(scope="module")
def oracle(M, W, ref_params):
    """(leaf, index, siblings) -> (the builder's witness as Montgomery limbs, its public inputs); built once per path."""
    seen = {}

    def get(leaf, index, siblings):
        k = (bytes(leaf), index, tuple(siblings))
        if k not in seen:
            cs = _WitnessOnly()
            public = W.build_poseidon_membership(cs, ref_params, leaf, index, siblings)
            assert public == cs.public
            seen[k] = (M._to_mont_limbs(cs.witness), public)
        return seen[k]
    return get


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: %d witnesses differ, the first at %d" % (what, bad.size, bad[0])


@pytest.fixture(scope="module")
def device_trees(HASH, sponge, model_tree):
    made = {}

    def get(leaf_len, n):
        if (leaf_len, n) not in made:
            made[(leaf_len, n)] = HASH.PoseidonMerkleTree.new(sponge, model_tree(leaf_len, n)[0])
        return made[(leaf_len, n)]
    yield get
    for t in made.values():
        t.free()


@pytest.mark.parametrize("leaf_len", [1, 55, 72])
@pytest.mark.parametrize("height", [2, 6])
@pytest.mark.parametrize("count", [1, 64, 65])
def test_witness_treeless_and_at(oracle, circuits, model_tree, device_trees, count, height, leaf_len):
    """The whole witness of every path equals the builder's assignment, the roots the model's, and the two forms agree word for
    word.  Path p of a batch is path p of every batch of this (height, leaf_len): the builder runs once per path."""
    n = 1 << (height - 1)
    leaves, want = model_tree(leaf_len, n)
    indices = [(11 * p + n - 1) % n for p in range(count)]
    sib = [T.path(want, i) for i in indices]
    mine = [leaves[i] for i in indices]
    c = circuits(height, leaf_len)
    witness, roots = c.witness_many(mine, indices, sib)
    assert witness.shape == (count, c.shape()[1], 4)
    assert roots == [want[-1][0]] * count
    for p in range(count):
        w, public = oracle(mine[p], indices[p], sib[p])
        _same(witness[p], w, "path %d" % p)
        assert public[0] == want[-1][0]
    at = c.witness_at(device_trees(leaf_len, n), mine, indices)
    assert np.array_equal(at, witness)


@pytest.mark.parametrize("count,chunk", [(7, 3), (3, 1)])
def test_witness_across_a_chunk_seam(oracle, circuits, model_tree, device_trees, count, chunk):
    """Both host forms with their stage cap moved (swm_selftest_witness_stage): 7 paths at a cap of 3 paths' witness bytes + 5 go in
    chunks of 3, 3 and 1, 3 paths at a cap one byte short of a path one by one.  Height 2, one-byte leaves; every witness the
    builder's, every root the model's, the resident tree's form the same words."""
    height, leaf_len, n = 2, 1, 2
    leaves, want = model_tree(leaf_len, n)
    indices = [(11 * p + n - 1) % n for p in range(count)]
    sib = [T.path(want, i) for i in indices]
    mine = [leaves[i] for i in indices]
    c = circuits(height, leaf_len)
    item = 32 * c.shape()[1]
    with c.ctx.selftest_witness_stage(3 * item + 5 if chunk == 3 else item - 1):
        witness, roots = c.witness_many(mine, indices, sib)
        at = c.witness_at(device_trees(leaf_len, n), mine, indices)
    assert witness.shape == (count, c.shape()[1], 4) and roots == [want[-1][0]] * count
    for p in range(count):
        _same(witness[p], oracle(mine[p], indices[p], sib[p])[0], "path %d" % p)
    assert np.array_equal(at, witness)


def test_witness_refusals(HASH, sponge, circuits, model_tree, device_trees):
    from simpleworks_amd._lib import SwmError
    leaves, want = model_tree(55, 32)
    c = circuits(6, 55)
    sib = [T.path(want, 3), T.path(want, 4)]
    sib[1][2] = R
    with pytest.raises(SwmError) as e:
        c.witness_many([leaves[3], leaves[4]], [3, 4], sib)
    assert e.value.code == -1 and "path 1" in str(e.value)
    with pytest.raises(SwmError) as e:
        c.witness_many([leaves[3]], [32], [T.path(want, 3)])
    assert e.value.code == -1
    with pytest.raises(SwmError) as e:
        c.witness_at(device_trees(55, 32), [leaves[3]], [32])
    assert e.value.code == -1
    with pytest.raises(SwmError) as e:          # a tree of another height
        c.witness_at(device_trees(55, 2), [leaves[0]], [0])
    assert e.value.code == -1
    for height, leaf_len in ((1, 1), (32, 1), (4, 0), (4, 257)):
        with pytest.raises(SwmError):
            HASH.PoseidonMembershipCircuit(sponge, height, leaf_len)
    lib, ctx = c.ctx.lib, c.ctx
    assert lib.swm_poseidon_tree_witness(ctx.h, c.h, None, None, None, 0, None, None) == 0
    assert lib.swm_poseidon_tree_witness_at(ctx.h, c.h, device_trees(55, 32).h, None, None, 0, None) == 0


@pytest.mark.parametrize("height,leaf_len", [(4, 1), (6, 72)])
def test_proof_equals_the_builders(M, W, ref_params, circuits, model_tree, device_trees, height, leaf_len):
    """Both prove entries are byte-identical to generate_proof on the builder's system with the same rng state; the proof verifies
    with [root] + leaf bits and not with one leaf bit flipped; a wrong root, a path that does not lead to the root and (_at)
    another leaf are SWM_ERR_UNSATISFIED (-5)."""
    from simpleworks_amd import serialization as Ser
    n = 1 << (height - 1)
    leaves, want = model_tree(leaf_len, n)
    index = n - 3
    leaf, sib, root = leaves[index], T.path(want, index), want[-1][0]
    cs = M.MarlinInst._synthesize(W.PoseidonMerkleTreeVerification(ref_params, root, leaf, index, sib))
    public = cs.instance[1:]
    assert public[0] == root and (height, leaf_len) != (4, 1) or cs.num_constraints == 1075
    packed = cs.pack()
    nnz = max(int(m[0][-1]) for m in packed.mats)
    srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, M.generate_rand())
    pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
    c, tree = circuits(height, leaf_len), device_trees(leaf_len, n)
    try:
        want_proof = Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand()))
        got = M.generate_poseidon_membership_proof(pk, c, root, leaf, index, sib, M.generate_rand())
        assert got == want_proof
        got_at = M.generate_poseidon_membership_proof(pk, c, None, leaf, index, None, M.generate_rand(), tree=tree)
        assert got_at == want_proof
        assert M.verify_proof(vk, public, M.MarlinProof(got), M.generate_rand())
        flipped = list(public)
        flipped[1 + 2] ^= 1
        assert not M.verify_proof(vk, flipped, M.MarlinProof(got), M.generate_rand())
        with pytest.raises(M.MarlinError) as e:
            M.generate_poseidon_membership_proof(pk, c, (root + 1) % R, leaf, index, sib, M.generate_rand())
        assert e.value.code == -5
        with pytest.raises(M.MarlinError) as e:
            M.generate_poseidon_membership_proof(pk, c, root, leaf, index ^ 1, sib, M.generate_rand())
        assert e.value.code == -5
        with pytest.raises(M.MarlinError) as e:
            M.generate_poseidon_membership_proof(pk, c, None, leaves[index ^ 1], index, None, M.generate_rand(), tree=tree)
        assert e.value.code == -5
        # the prover is as it was for the next caller: the device source does not outlive the call
        assert Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand())) == got
    finally:
        pk.free()
        srs.free()


def test_a_pedersen_membership_key_does_not_match(M, W, circuits, model_tree):
    cs, _, _ = W.merkle_membership_circuit(height=2, gadget_byte_ops=0)
    packed = cs.pack()
    nnz = max(int(m[0][-1]) for m in packed.mats)
    srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, M.generate_rand())
    pk, _ = M.MarlinInst.index_from_constraint_system(srs, packed)
    srs.free()
    leaves, want = model_tree(1, 8)
    try:
        with pytest.raises(M.MarlinError) as e:
            M.generate_poseidon_membership_proof(pk, circuits(4, 1), want[-1][0], leaves[5], 5, T.path(want, 5), M.generate_rand())
        assert e.value.code == -8
    finally:
        pk.free()

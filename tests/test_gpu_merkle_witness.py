"""The membership circuit's witness synthesised on the GPU (csrc/merkle_witness.hip: swm_merkle_witness, swm_merkle_witness_dev,
swm_merkle_prove) against its specification, workloads.build_merkle_membership run on the CPU into a ConstraintSystem: exact
integer equality of the whole witness vector, of the instance and of the root; then SimpleMerkleTree.prove_on_gpu / prove_many
against SimpleMerkleTree.prove, byte for byte."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001


@pytest.fixture(scope="module")
def M():
    from simpleworks_amd import marlin
    return marlin


@pytest.fixture(scope="module")
def W():
    from simpleworks_amd import workloads
    return workloads


@pytest.fixture(scope="module")
def H():
    from simpleworks_amd import hash
    return hash


@pytest.fixture(scope="module")
def params(W):
    """The reference's configuration (256-bit digests, 144 / 128 windows of 4) with the committed fixtures' generators."""
    p = W.MerkleParams()
    p.crh()
    return p


@pytest.fixture(scope="module")
def circuits(H, params):
    made = {}

    def get(height, ops):
        if (height, ops) not in made:
            made[height, ops] = H.MerkleCircuit(*params.crh(), height, ops)
        return made[height, ops]
    yield get
    for c in made.values():
        c.free()


def _oracle(M, W, params, leaf, index, siblings, ops):
    """(witness as Montgomery limbs, instance ints, root) of the builder."""
    cs = M.ConstraintSystem()
    public = W.build_merkle_membership(cs, params, leaf, index, list(siblings), gadget_byte_ops=ops)
    return M._to_mont_limbs(cs.witness), cs.instance, public[0]


def _check_batch(M, W, params, circuit, leaves, indices, paths, ops):
    witness, roots = circuit.witness_many(leaves, indices, paths)
    ni, nw, nc = circuit.shape()
    assert witness.shape == (len(leaves), nw, 4)
    for i, (leaf, index, path) in enumerate(zip(leaves, indices, paths)):
        want, instance, root = _oracle(M, W, params, leaf, index, path, ops)
        assert len(instance) == ni
        bad = np.nonzero((witness[i] != want).any(axis=1))[0]
        assert bad.size == 0, "path %d: %d witnesses differ, the first at %d" % (i, bad.size, bad[0])
        assert roots[i] == root == instance[1], i
    return witness, roots


@pytest.mark.parametrize("ops", [0, 16])
def test_height2_edge_paths(M, W, H, params, circuits, ops):
    """One level: a leaf chain, a direction select, both decompositions and one full 512-bit scan.  Leaf 0x00 keeps the leaf
    hash's running sum at the identity (every t is 0), 0xFF sets every bit; sibling 0 is the blank tree's path, r - 1 the
    largest canonical digest; the last two paths are those of a real two-leaf tree.  16 operations: all three kinds, shifts
    1..7, and operation 10 reads pool[70] of 74 entries, an earlier result."""
    a, b = 0xA7, 0x3C
    tree = H.MerkleTree.new(*params.crh(), [a, b])
    leaves = [0x00, 0xFF, 0x00, 0xFF, a, b]
    indices = [0, 1, 1, 0, 0, 1]
    paths = [[0], [R - 1], [R - 1], [0], [tree.node(0, 1)], [tree.node(0, 0)]]
    _, roots = _check_batch(M, W, params, circuits(2, ops), leaves, indices, paths, ops)
    assert roots[4] == roots[5] == tree.root()


@pytest.mark.parametrize("height,ops", [(3, 5), (5, 0)])
def test_real_trees_every_leaf(M, W, H, params, circuits, height, ops):
    n = 1 << (height - 1)
    leaves = [(37 * i + 11) & 0xFF for i in range(n)]
    tree = H.MerkleTree.new(*params.crh(), leaves)
    assert tree.height() == height
    paths = [tree.generate_proof(i) for i in range(n)]
    _, roots = _check_batch(M, W, params, circuits(height, ops), leaves, list(range(n)), paths, ops)
    assert roots == [tree.root()] * n


def test_batch_shapes(M, W, params, circuits):
    """count = 1, and count = 65 (no multiple of any packing factor): path i of the batch is that path computed alone."""
    g = W._SplitMix(65)
    leaves = [(29 * i + 3) & 0xFF for i in range(65)]
    indices = [i & 1 for i in range(65)]
    paths = [[g.fr()] for _ in range(65)]
    c = circuits(2, 0)
    _check_batch(M, W, params, c, leaves[:1], indices[:1], paths[:1], 0)
    witness, roots = c.witness_many(leaves, indices, paths)
    for i in range(65):
        w1, r1 = c.witness_many(leaves[i:i + 1], indices[i:i + 1], paths[i:i + 1])
        assert np.array_equal(w1[0], witness[i]), i
        assert r1[0] == roots[i]
    w0, r0 = c.witness_many([], [], [])   # nothing to launch
    assert w0.shape[0] == 0 and r0 == []


def test_full_size(M, W, params, circuits):
    """Height 19 with the 2400 byte operations of `--circuit merkle`, random canonical siblings: the builder's witness, and the
    GPU's witness satisfies the circuit's matrices."""
    g = W._SplitMix(7)
    siblings = [g.fr() for _ in range(18)]
    index = g.next_u64() % (1 << 18)
    cs, public, _ = W.merkle_membership_circuit(height=19, leaf_u8=0xA7, leaf_index=index, gadget_byte_ops=2400, params=params,
                                                siblings=siblings)
    c = circuits(19, 2400)
    assert c.shape() == (len(cs.instance), len(cs.witness), cs.num_constraints)
    witness, roots = c.witness_many([0xA7], [index], [siblings])
    want = M._to_mont_limbs(cs.witness)
    bad = np.nonzero((witness[0] != want).any(axis=1))[0]
    assert bad.size == 0, "%d witnesses differ, the first at %d" % (bad.size, bad[0])
    assert roots[0] == public[0]
    packed = cs.pack()
    assert M.PackedR1cs(M._to_mont_limbs([1] + public), witness[0], *packed.mats).is_satisfied()


def test_device_form_and_refusals(M, W, params, circuits):
    from simpleworks_amd._lib import DeviceBuffer, SwmError
    c = circuits(2, 16)
    ctx = c.ctx
    nw = c.shape()[1]
    g = W._SplitMix(5)
    leaves, indices = [0x11, 0x22, 0x33], [0, 1, 1]
    good = [[g.fr()], [g.fr()], [g.fr()]]
    want, want_roots = c.witness_many(leaves, indices, good)

    def run_dev(idx, paths):
        sib = np.frombuffer(b"".join(int(s).to_bytes(32, "little") for p in paths for s in p), dtype=np.uint8)
        bufs = [DeviceBuffer(ctx, 256).upload(np.array(leaves, dtype=np.uint8)), DeviceBuffer(ctx, 256).upload(np.array(idx, dtype=np.uint64)),
                DeviceBuffer(ctx, 256).upload(sib), DeviceBuffer(ctx, 3 * nw * 32), DeviceBuffer(ctx, 256), DeviceBuffer(ctx, 256)]
        ctx.merkle_witness_dev(c.h, bufs[0], bufs[1], bufs[2], 3, bufs[3], bufs[4], bufs[5])
        out = (bufs[3].download((3, nw, 4)), bufs[4].download((3, 32), np.uint8), bufs[5].download((3,), np.uint32))
        for b in bufs:
            b.free()
        return out

    w, roots, status = run_dev(indices, good)
    assert status.tolist() == [0, 0, 0]
    assert np.array_equal(w, want)
    assert [int.from_bytes(r.tobytes(), "little") for r in roots] == want_roots
    # a sibling >= r: that path's status, witness and root say so, its neighbours are untouched; the host form refuses the call
    for s in (R, (1 << 256) - 1):
        paths = [good[0], [s], good[2]]
        w, roots, status = run_dev(indices, paths)
        assert status.tolist() == [0, 1, 0]
        assert not w[1].any() and not roots[1].any()
        assert np.array_equal(w[0], want[0]) and np.array_equal(w[2], want[2])
        with pytest.raises(SwmError) as e:
            ctx.merkle_witness(c.h, nw, np.array(leaves, dtype=np.uint8), np.array(indices, dtype=np.uint64),
                               np.frombuffer(b"".join(int(x).to_bytes(32, "little") for p in paths for x in p), dtype=np.uint8).reshape(3, 1, 32))
        assert e.value.code == -1 and "canonical" in str(e.value)
    # a leaf index beyond the 2^L leaves
    w, roots, status = run_dev([0, 1, 2], good)
    assert status.tolist() == [0, 0, 2] and not w[2].any()
    assert np.array_equal(w[:2], want[:2])
    with pytest.raises(SwmError) as e:
        c.witness_many(leaves, [0, 1, 2], good)
    assert e.value.code == -1 and "leaf index" in str(e.value)


def test_create_refusals(H, W, params):
    from simpleworks_amd._lib import SwmError
    leaf, inner = params.crh()
    for height in (0, 1, 65):
        with pytest.raises(SwmError) as e:
            H.MerkleCircuit(leaf, inner, height)
        assert e.value.code == -1
    gens = params.inner_gens
    narrow = H.PedersenCRH([row[:2] for row in gens[:128]])       # windows of 2 bits
    one_window = H.PedersenCRH(gens[:1])                             # a leaf set of fewer than 2 windows
    short = H.PedersenCRH(gens[:127])                                # a two-to-one set of fewer than 128
    try:
        for a, b in ((narrow, inner), (leaf, narrow), (one_window, inner), (leaf, short)):
            with pytest.raises(SwmError) as e:
                H.MerkleCircuit(a, b, 5)
            assert e.value.code == -1
    finally:
        for p in (narrow, one_window, short):
            p.free()


@pytest.fixture(scope="module")
def trees(M, W, params):
    """SimpleMerkleTree over 16 leaves, the universal SRS just large enough for the circuit (as test_merkle_real_tree_height5
    sizes it), with and without the byte-operation block."""
    leaves = [(37 * i + 11) & 0xFF for i in range(16)]
    made = {}

    def get(ops):
        if ops not in made:
            cs = M.ConstraintSystem()
            W.build_merkle_membership(cs, params, 0, 0, [0] * 4, gadget_byte_ops=ops)
            packed = cs.pack()
            nnz = max(int(m[0][-1]) for m in packed.mats)
            sizes = (cs.num_constraints, len(cs.instance) + len(cs.witness), nnz)
            made[ops] = W.SimpleMerkleTree(leaves, params=params, srs_sizes=sizes, gadget_byte_ops=ops)
        return made[ops]
    yield leaves, get
    for t in made.values():
        t.free()


@pytest.mark.parametrize("ops", [0, 16])
def test_prove_on_gpu_equals_prove(trees, ops):
    leaves, get = trees
    tree = get(ops)
    idx = 9
    path = tree.get_merkle_path(idx)
    want = tree.prove(leaves[idx], path)
    got = tree.prove_on_gpu(leaves[idx], path)
    assert got == want
    assert tree.verify(got, leaves[idx])
    assert not tree.verify(got, leaves[idx] ^ 1)


def test_prove_many_and_errors(M, W, H, params, trees):
    from simpleworks_amd import serialization as S
    leaves, get = trees
    tree = get(16)
    picks = [0, 5, 10, 15]
    paths = [tree.get_merkle_path(i) for i in picks]
    singles = [tree.prove_on_gpu(leaves[i], p) for i, p in zip(picks, paths)]
    assert tree.prove_many([leaves[i] for i in picks], paths) == singles
    assert all(tree.verify(pr, leaves[i]) for pr, i in zip(singles, picks))
    # the public root is an input: a wrong one fails the prover's own check
    circuit = tree._merkle_circuit()
    index, siblings = paths[1]
    with pytest.raises(M.MarlinError) as e:
        M.generate_merkle_proof(tree.proving_key, circuit, (tree.root() + 1) % R, leaves[5], index, siblings, M.generate_rand())
    assert e.value.code == -5
    with pytest.raises(M.MarlinError) as e:   # the right root, another leaf
        M.generate_merkle_proof(tree.proving_key, circuit, tree.root(), leaves[5] ^ 1, index, siblings, M.generate_rand())
    assert e.value.code == -5
    # a circuit of another height against this key
    other = H.MerkleCircuit(*params.crh(), 3, 16)
    with pytest.raises(M.MarlinError) as e:
        M.generate_merkle_proof(tree.proving_key, other, tree.root(), leaves[5], index & 3, siblings[:2], M.generate_rand())
    assert e.value.code == -8
    other.free()
    # the uncompressed form recodes to the compressed bytes
    raw = M.generate_merkle_proof(tree.proving_key, circuit, tree.root(), leaves[5], index, siblings, M.generate_rand(), uncompressed=True)
    assert len(raw) > len(singles[1])
    assert S.proof_recode(raw, False) == singles[1]
    # the prover is as it was for the next caller: the device source does not outlive the call
    assert tree.prove(leaves[5], paths[1]) == singles[1]


def test_toy_digests_stay_on_the_builder(W):
    """digest_bits < 256 exists in the Python builder only: the GPU entry points say so before touching the GPU."""
    tree = W.SimpleMerkleTree.__new__(W.SimpleMerkleTree)
    tree.params = type("P", (), {"digest_bits": 16})()
    tree._circuit = None
    with pytest.raises(ValueError):
        tree.prove_on_gpu(0, (0, []))
    with pytest.raises(ValueError):
        tree.prove_many([0], [(0, [])])

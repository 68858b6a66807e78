"""The Merkle tree that stays on the GPU (csrc/merkle_tree.hip: swm_merkle_tree_*, swm_merkle_verify_paths; hash.DeviceMerkleTree,
hash.verify_paths) — what examples/simple-payments/ledger.rs:106-173 and transaction.rs:163-173 do to the account tree.
Three references, none of them the code under test:
  * hash.MerkleTree.new on the modified leaf list (swm_merkle_tree_build, held to the oracle by test_gpu_pedersen.py);
  * PedersenCRH.evaluate / evaluate_many;
  * root_from_path of the pure-Python model (oracle/pyref/pedersen.py) and the tree and path of tests/golden/pedersen.json.
Every tree comparison is byte equality over all 2 n - 1 nodes.  Leaves are 1 byte (u8) and 72 bytes (the ledger's account)."""
import numpy as np
import pytest

from oracle_lib import golden, h2i

pytestmark = pytest.mark.gpu

R = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001
LEAF_LENS = (1, 72)


@pytest.fixture(scope="module")
def H():
    from simpleworks_amd import hash
    return hash


@pytest.fixture(scope="module")
def M():
    from simpleworks_amd import marlin
    return marlin


@pytest.fixture(scope="module")
def params(H, M):
    """LeafHash::setup then TwoToOneHash::setup from a fresh test_rng, as in test_gpu_pedersen.py."""
    rng = M.generate_rand()
    leaf = H.PedersenCRH.setup(rng, H.LEAF_WINDOWS)
    inner = H.PedersenCRH.setup(rng, H.TWO_TO_ONE_WINDOWS)
    return leaf, inner


@pytest.fixture(scope="module")
def rebuilt(H, params):
    """leaves uint8 [n, leaf_len] -> all nodes of MerkleTree.new over them, uint8 [2 n - 1, 32]; built once per leaf list."""
    seen = {}

    def get(leaves):
        key = (leaves.shape, leaves.tobytes())
        if key not in seen:
            seen[key] = np.concatenate(H.MerkleTree.new(params[0], params[1], _rows(leaves)).levels)
            seen[key].setflags(write=False)
        return seen[key]
    return get


def _rows(leaves):
    return [int(r[0]) for r in leaves] if leaves.shape[1] == 1 else [bytes(r) for r in leaves]


def _leaves(seed, n, leaf_len):
    return np.random.default_rng(seed).integers(0, 256, size=(n, leaf_len), dtype=np.uint8)


def _nodes(tree):
    return tree.ctx.merkle_tree_nodes(tree.h)


def _levels(nodes):
    out, off, cnt = [], 0, (len(nodes) + 1) // 2
    while cnt >= 1:
        out.append(nodes[off:off + cnt])
        off += cnt
        cnt >>= 1
    return out


def _apply(leaves, indices, new):
    """The leaf list after tree.update(indices[i], new[i]) in order."""
    out = leaves.copy()
    for i, row in zip(indices, new):
        out[i] = row
    return out


def _ints(rows):
    return [int.from_bytes(r.tobytes(), "little") for r in rows]


# ---------------------------------------------------------------------------------------------- blank, from leaves

@pytest.mark.parametrize("height", [2, 3, 7])
@pytest.mark.parametrize("leaf_len", LEAF_LENS)
def test_blank(H, params, height, leaf_len):
    """MerkleTree::blank: leaf digests are 32 zero bytes (not the hash of anything), every level is uniform, and a node of level
    l + 1 is the two-to-one hash of two equal nodes of level l."""
    leaf, inner = params
    tree = H.DeviceMerkleTree.blank(leaf, inner, height, leaf_len)
    levels = _levels(_nodes(tree))
    assert tree.height() == height == len(levels) and [len(l) for l in levels] == [1 << (height - 1 - l) for l in range(height)]
    assert not levels[0].any()
    for l in range(height):
        assert (levels[l] == levels[l][0]).all(), l
    for l in range(height - 1):
        assert int.from_bytes(levels[l + 1][0].tobytes(), "little") == inner.evaluate(levels[l][0].tobytes() * 2), l
    assert tree.root() == int.from_bytes(levels[-1][0].tobytes(), "little")
    tree.free()


@pytest.mark.parametrize("n", [2, 4, 64])
@pytest.mark.parametrize("leaf_len", LEAF_LENS)
def test_from_leaves_equals_merkle_tree_new(H, params, rebuilt, n, leaf_len):
    leaf, inner = params
    leaves = _leaves(n, n, leaf_len)
    tree = H.DeviceMerkleTree.new(leaf, inner, _rows(leaves))
    assert np.array_equal(_nodes(tree), rebuilt(leaves))
    assert tree.height() == n.bit_length()
    down = tree.to_merkle_tree()
    assert down.height() == tree.height() and down.root() == tree.root()
    # the device form, and the buffer the handle owns
    d_leaves = tree.ctx.to_device(leaves)
    h2 = tree.ctx.merkle_tree_create_from_leaves_dev(leaf.h, inner.h, d_leaves, leaf_len, n)
    assert np.array_equal(tree.ctx.merkle_tree_nodes(h2), rebuilt(leaves))
    ptr, count = tree.ctx.merkle_tree_dev_nodes(h2)
    assert ptr and count == 2 * n - 1
    tree.ctx.merkle_tree_destroy(h2)
    d_leaves.free()
    tree.free()


def test_from_leaves_fixture_tree(H, params):
    leaf, inner = params
    t = golden("pedersen.json")["tree"]
    tree = H.DeviceMerkleTree.new(leaf, inner, t["leaves"])
    assert tree.to_merkle_tree().int_levels() == [[h2i(v) for v in lvl] for lvl in t["levels"]]
    assert tree.root() == h2i(t["root"]) and tree.height() == 4
    assert tree.generate_proof(t["index"]) == [h2i(v) for v in t["path"]]
    tree.free()


# ---------------------------------------------------------------------------------------------- updates

@pytest.mark.parametrize("height,indices", [(2, [0, 1]), (4, list(range(8))), (7, [0, 21, 42, 63])])
@pytest.mark.parametrize("leaf_len", LEAF_LENS)
def test_single_update_equals_a_rebuild(H, params, rebuilt, height, indices, leaf_len):
    """Every index of n = 2 (one two-to-one level: the finishing workgroup is the whole job) and n = 8 pins left and right."""
    leaf, inner = params
    n = 1 << (height - 1)
    leaves = _leaves(100 + height, n, leaf_len)
    tree = H.DeviceMerkleTree.new(leaf, inner, _rows(leaves))
    for i in indices:
        new = _leaves(200 + i, 1, leaf_len)
        tree.update(i, _rows(new)[0])
        leaves = _apply(leaves, [i], new)
        assert np.array_equal(_nodes(tree), rebuilt(leaves)), i
    tree.free()


def _bit_reverse6(i):
    return int("{:06b}".format(i % 64)[::-1], 2)


PATTERNS = {
    "both children of one parent": lambda k: [(10 + i) % 64 for i in range(k)],                # parents merge from level 1 on
    "one 8-leaf subtree": lambda k: [40 + (3 * i) % 8 for i in range(k)],                      # narrows to one node by level 3
    "one per subtree, far apart": lambda k: [_bit_reverse6(i) for i in range(k)],              # k nodes stay dirty for several levels
    "all leaves": lambda k: [(63 - 37 * i) % 64 for i in range(k)],                            # k = 64: the whole tree, unordered
}


@pytest.mark.parametrize("k", list(range(1, 10)) + [16, 17, 64])
@pytest.mark.parametrize("leaf_len", LEAF_LENS)
def test_batches_equal_a_rebuild(H, params, rebuilt, k, leaf_len):
    """n = 64.  k <= 4 goes to the finishing workgroup straight from the leaf launch; k = 5 .. 9 far apart keeps more than four
    nodes dirty for several levels before the hand-over; 16 and 17 take index lists; 64 rewrites the tree."""
    leaf, inner = params
    base = _leaves(64, 64, leaf_len)
    for name, pattern in PATTERNS.items():
        indices = pattern(k)
        assert len(indices) == k and all(0 <= i < 64 for i in indices)
        tree = H.DeviceMerkleTree.new(leaf, inner, _rows(base))
        new = _leaves(1000 + k, k, leaf_len)
        tree.update_many(indices, _rows(new))
        assert np.array_equal(_nodes(tree), rebuilt(_apply(base, indices, new))), name
        tree.free()
    assert sorted(PATTERNS["all leaves"](64)) == list(range(64))


@pytest.mark.parametrize("indices", [[5, 9, 5], [5, 9, 5, 30, 5], [63, 63], [0, 1, 2, 3, 4, 5, 0, 6, 7, 8, 0]])
@pytest.mark.parametrize("leaf_len", LEAF_LENS)
def test_a_repeated_index_keeps_its_last_leaf(H, params, rebuilt, indices, leaf_len):
    leaf, inner = params
    base = _leaves(7, 64, leaf_len)
    tree = H.DeviceMerkleTree.new(leaf, inner, _rows(base))
    new = _leaves(8, len(indices), leaf_len)
    assert len({r.tobytes() for r in new}) == len(indices)
    tree.update_many(indices, _rows(new))
    want = _apply(base, indices, new)
    assert np.array_equal(want[indices[0]], new[len(indices) - 1 - indices[::-1].index(indices[0])])
    assert np.array_equal(_nodes(tree), rebuilt(want))
    tree.free()


@pytest.mark.parametrize("i,j", [(0, 1), (3, 60), (17, 17)])
@pytest.mark.parametrize("leaf_len", LEAF_LENS)
def test_a_batch_equals_the_sequence(H, params, rebuilt, i, j, leaf_len):
    leaf, inner = params
    base = _leaves(9, 64, leaf_len)
    new = _leaves(10, 2, leaf_len)
    a = H.DeviceMerkleTree.new(leaf, inner, _rows(base))
    b = H.DeviceMerkleTree.new(leaf, inner, _rows(base))
    a.update_many([i, j], _rows(new))
    b.update(i, _rows(new)[0])
    b.update(j, _rows(new)[1])
    assert np.array_equal(_nodes(a), _nodes(b))
    assert np.array_equal(_nodes(a), rebuilt(_apply(base, [i, j], new)))
    a.free()
    b.free()


def test_update_with_the_leaves_on_the_device(H, params, rebuilt):
    """swm_merkle_tree_update_dev: indices on the host, leaf bytes on the device; 2 updates (no list goes up) and 20."""
    leaf, inner = params
    base = _leaves(11, 64, 72)
    for indices in ([7, 50], list(range(3, 63, 3))):
        tree = H.DeviceMerkleTree.new(leaf, inner, _rows(base))
        new = _leaves(12, len(indices), 72)
        d_new = tree.ctx.to_device(new)
        tree.ctx.merkle_tree_update_dev(tree.h, indices, d_new, 72)
        assert np.array_equal(_nodes(tree), rebuilt(_apply(base, indices, new)))
        d_new.free()
        tree.free()


@pytest.mark.parametrize("leaf_len", LEAF_LENS)
def test_blank_then_updates(H, params, rebuilt, leaf_len):
    """After some updates the untouched leaf digests are still zero, the touched ones are the leaf hash, and every node above is
    the two-to-one hash of its children; after all leaves have been written the tree is MerkleTree.new(leaves)."""
    leaf, inner = params
    n = 8
    leaves = _leaves(13, n, leaf_len)
    tree = H.DeviceMerkleTree.blank(leaf, inner, 4, leaf_len)
    touched = [6, 1, 3]
    tree.update(6, _rows(leaves)[6])
    tree.update_many([1, 3], [_rows(leaves)[1], _rows(leaves)[3]])
    levels = _levels(_nodes(tree))
    for i in range(n):
        want = leaf.evaluate_many(leaves[i:i + 1])[0] if i in touched else np.zeros(32, np.uint8)
        assert np.array_equal(levels[0][i], want), i
    for l in range(3):
        pairs = levels[l].reshape(-1, 64)
        assert np.array_equal(levels[l + 1], inner.evaluate_many(pairs)), l
    rest = [i for i in range(n) if i not in touched]
    tree.update_many(rest, [_rows(leaves)[i] for i in rest])
    assert np.array_equal(_nodes(tree), rebuilt(leaves))
    tree.update_many([], [])   # nothing to launch
    assert np.array_equal(_nodes(tree), rebuilt(leaves))
    tree.free()


# ---------------------------------------------------------------------------------------------- paths

@pytest.mark.parametrize("height", [2, 5])
@pytest.mark.parametrize("leaf_len", LEAF_LENS)
def test_paths_equal_generate_proof_of_the_downloaded_tree(H, params, height, leaf_len):
    leaf, inner = params
    n = 1 << (height - 1)
    tree = H.DeviceMerkleTree.new(leaf, inner, _rows(_leaves(14, n, leaf_len)))
    down = tree.to_merkle_tree()
    indices = [0, n - 1, n // 2, n // 2]
    got = tree.generate_proofs(indices)
    assert got.shape == (4, height - 1, 32)
    for row, i in zip(got, indices):
        assert _ints(row) == down.generate_proof(i), i
        assert tree.generate_proof(i) == down.generate_proof(i)
    assert tree.generate_proofs([]).shape == (0, height - 1, 32)
    with pytest.raises(IndexError):
        tree.generate_proof(n)
    from simpleworks_amd._lib import SwmError
    with pytest.raises(SwmError) as e:
        tree.generate_proofs([0, n])
    assert e.value.code == -1
    tree.free()


def test_device_paths_feed_the_membership_witness(H, params):
    """swm_merkle_tree_paths_dev writes what swm_merkle_witness_dev reads, with no host copy between them: the roots the circuit
    arrives at are the tree's (u8 leaves, height 5).  An index beyond the leaves reads as a zero path and is status 2 there."""
    leaf, inner = params
    leaves = _leaves(15, 16, 1)
    tree = H.DeviceMerkleTree.new(leaf, inner, _rows(leaves))
    circuit = H.MerkleCircuit(leaf, inner, 5)
    ctx, nw = tree.ctx, circuit.shape()[1]
    indices = np.array([0, 15, 6, 6, 16], dtype=np.uint64)
    picked = np.array([leaves[int(i) % 16, 0] for i in indices], dtype=np.uint8)
    d_idx, d_leaf = ctx.to_device(indices), ctx.to_device(picked)
    d_sib, d_w, d_roots, d_status = ctx.alloc(5 * 4 * 32), ctx.alloc(5 * nw * 32), ctx.alloc(5 * 32), ctx.alloc(64)
    ctx.merkle_tree_paths_dev(tree.h, d_idx, 5, d_sib)
    ctx.merkle_witness_dev(circuit.h, d_leaf, d_idx, d_sib, 5, d_w, d_roots, d_status)
    sib = d_sib.download((5, 4, 32), np.uint8)
    roots = d_roots.download((5, 32), np.uint8)
    status = d_status.download((5,), np.uint32)
    down = tree.to_merkle_tree()
    for p in range(4):
        assert _ints(sib[p]) == down.generate_proof(int(indices[p])), p
    assert not sib[4].any()
    assert status.tolist() == [0, 0, 0, 0, 2]
    assert _ints(roots[:4]) == [tree.root()] * 4
    _, host_roots = circuit.witness_many(picked[:4], indices[:4], sib[:4])
    assert host_roots == [tree.root()] * 4
    for b in (d_idx, d_leaf, d_sib, d_w, d_roots, d_status):
        b.free()
    circuit.free()
    tree.free()


# ---------------------------------------------------------------------------------------------- path check

@pytest.fixture(scope="module")
def checked_trees(H, params):
    """(height, leaf_len) -> (leaves, the downloaded MerkleTree, all paths uint8 [n, L, 32]) of one tree per shape."""
    made = {}

    def get(height, leaf_len):
        if (height, leaf_len) not in made:
            n = 1 << (height - 1)
            leaves = _leaves(16 + height, n, leaf_len)
            tree = H.DeviceMerkleTree.new(params[0], params[1], _rows(leaves))
            made[height, leaf_len] = (leaves, tree.to_merkle_tree(), tree.generate_proofs(range(n)))
            tree.free()
        return made[height, leaf_len]
    return get


def _verify(params, height, roots, leaves, indices, siblings):
    leaf, inner = params
    ok, status = leaf.ctx.merkle_verify_paths(leaf.h, inner.h, height, roots, leaves, np.asarray(indices, dtype=np.uint64), siblings)
    return ok.tolist(), status.tolist()


# 1 .. 257: 64 lanes per path, ragged last workgroups; 4097, 20000 and 131073: 32, 8 and 1 lanes per path (lanes_for)
@pytest.mark.parametrize("height,count", [(2, 1), (2, 3), (2, 4), (2, 5), (2, 257), (7, 1), (7, 3), (7, 4), (7, 5), (7, 257), (7, 4097),
                                          (7, 20000), (3, 131073)])
@pytest.mark.parametrize("leaf_len", LEAF_LENS)
def test_valid_paths_verify_and_tampered_ones_do_not(H, params, checked_trees, height, count, leaf_len):
    leaves, down, paths = checked_trees(height, leaf_len)
    n, L = len(leaves), height - 1
    root = down.levels[-1][0]
    idx = (np.arange(count) * 7 + 3) % n
    lv, sib = leaves[idx], paths[idx]
    # one root for all, then one root per path
    assert _verify(params, height, root, lv, idx, sib) == ([1] * count, [0] * count)
    assert _verify(params, height, np.tile(root, (count, 1)), lv, idx, sib) == ([1] * count, [0] * count)
    assert H.verify_paths(params[0], params[1], height, down.root(), _rows(lv), idx, sib).all()
    # one tamper per call, at the last path (the ragged end of the launch) and in the middle; its neighbours still verify
    for at in sorted({count - 1, count // 2}):
        want = [1] * count
        want[at] = 0

        def tampered(what, level=0):
            l2, i2, s2, r2 = lv.copy(), idx.copy(), sib.copy(), np.tile(root, (count, 1))
            if what == "leaf":
                l2[at, -1] ^= 0x10
            elif what == "sibling":
                s2[at, level, 0] ^= 1
            elif what == "index":
                i2[at] ^= 1 << level
            else:
                r2[at, 3] ^= 4
            return _verify(params, height, r2, l2, i2, s2)
        for level in sorted({0, L // 2, L - 1}):
            assert tampered("sibling", level) == (want, [0] * count), ("sibling", level)
            assert tampered("index", level) == (want, [0] * count), ("index", level)
        assert tampered("leaf") == (want, [0] * count)
        assert tampered("root") == (want, [0] * count)
        if count == 1:   # one root for all paths, wrong
            wrong = root.copy()
            wrong[31] ^= 1
            assert _verify(params, height, wrong, lv, idx, sib) == ([0], [0])
    # what the witness kernel reports per path: a sibling or root >= r is 1, an index >= 2^L is 2; the neighbours are unaffected
    if count >= 3:
        s2, i2, r2 = sib.copy(), idx.copy().astype(np.uint64), np.tile(root, (count, 1))
        s2[0, L - 1] = np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint8)
        i2[count - 1] += n
        ok, status = _verify(params, height, r2, lv, i2, s2)
        assert ok == [0] + [1] * (count - 2) + [0] and status == [1] + [0] * (count - 2) + [2]
        r2[1] = 0xFF
        i2[count - 1] = 1 << 63
        ok, status = _verify(params, height, r2, lv, i2, s2)
        assert ok == [0, 0] + [1] * (count - 3) + [0] and status == [1, 1] + [0] * (count - 3) + [2]


@pytest.mark.parametrize("height", [2, 7])
def test_path_check_against_the_python_model(H, params, height):
    """Two paths that no GPU tree produced: random canonical siblings, the root folded by root_from_path of the pure-Python model."""
    from pyref.pedersen import root_from_path
    leaf, inner = params
    rng = np.random.default_rng(height)
    L = height - 1
    lv = rng.integers(0, 256, size=(2, 72), dtype=np.uint8)
    idx = [int(rng.integers(0, 1 << L)), (1 << L) - 1]
    sib = [[int.from_bytes(rng.bytes(32), "little") % R for _ in range(L)] for _ in range(2)]
    roots = [root_from_path(leaf.generators, inner.generators, bytes(lv[p]), idx[p], sib[p]) for p in range(2)]
    assert H.verify_paths(leaf, inner, height, roots, [bytes(r) for r in lv], idx, sib).tolist() == [True, True]
    assert H.verify_paths(leaf, inner, height, roots[::-1], [bytes(r) for r in lv], idx, sib).tolist() == [False, False]
    assert H.verify_paths(leaf, inner, height, roots[0], [bytes(r) for r in lv], idx, sib).tolist() == [True, False]
    assert H.verify_paths(leaf, inner, height, roots, [], [], []).shape == (0,)


def test_path_check_on_device_buffers(H, params, checked_trees):
    leaves, down, paths = checked_trees(7, 72)
    leaf, inner = params
    ctx = leaf.ctx
    idx = np.array([5, 40, 63], dtype=np.uint64)
    lv = leaves[idx.astype(np.int64)].copy()
    lv[1, 0] ^= 1
    bufs = [ctx.to_device(down.levels[-1][0]), ctx.to_device(lv), ctx.to_device(idx), ctx.to_device(paths[idx.astype(np.int64)]), ctx.alloc(64),
            ctx.alloc(64)]
    ctx.merkle_verify_paths_dev(leaf.h, inner.h, 7, bufs[0], 0, bufs[1], 72, bufs[2], bufs[3], 3, bufs[4], bufs[5])
    assert bufs[4].download((3,), np.uint8).tolist() == [1, 0, 1] and bufs[5].download((3,), np.uint32).tolist() == [0, 0, 0]
    ctx.merkle_verify_paths_dev(leaf.h, inner.h, 7, bufs[0], 0, bufs[1], 72, bufs[2], bufs[3], 2, bufs[4])   # no status wanted
    assert bufs[4].download((3,), np.uint8).tolist() == [1, 0, 1]
    for b in bufs:
        b.free()


# ---------------------------------------------------------------------------------------------- refusals

def test_refusals_leave_the_tree_as_it_was(H, params):
    from simpleworks_amd._lib import SwmError
    leaf, inner = params
    for height, leaf_len in ((1, 72), (32, 72), (0, 1), (4, 73), (4, 0)):
        with pytest.raises(SwmError) as e:
            H.DeviceMerkleTree.blank(leaf, inner, height, leaf_len)
        assert e.value.code == -1, (height, leaf_len)
    short = H.PedersenCRH(inner.generators[:100])   # a two-to-one set that cannot take two digests
    with pytest.raises(SwmError) as e:
        H.DeviceMerkleTree.blank(leaf, short, 4, 72)
    assert e.value.code == -1
    short.free()
    for bad_n in (1, 3, 6):
        with pytest.raises(SwmError) as e:
            H.DeviceMerkleTree.new(leaf, inner, list(range(bad_n)))
        assert e.value.code == -1
    with pytest.raises(SwmError) as e:
        leaf.ctx.merkle_verify_paths(leaf.h, inner.h, 1, np.zeros(32, np.uint8), np.zeros((1, 1), np.uint8), np.zeros(1, np.uint64),
                                     np.zeros((1, 0, 32), np.uint8))
    assert e.value.code == -1
    for start in ("blank", "leaves"):
        base = _leaves(17, 8, 72)
        tree = H.DeviceMerkleTree.blank(leaf, inner, 4, 72) if start == "blank" else H.DeviceMerkleTree.new(leaf, inner, _rows(base))
        before = _nodes(tree)
        new = _leaves(18, 3, 72)
        for indices in ([1, 8, 2], [1, 2, 1 << 40]):      # an index >= n in a batch
            with pytest.raises(SwmError) as e:
                tree.update_many(indices, _rows(new))
            assert e.value.code == -1 and "update %d" % [i >= 8 for i in indices].index(True) in str(e.value)
            assert np.array_equal(_nodes(tree), before)
        with pytest.raises(SwmError) as e:                # a leaf_len that differs from the tree's
            tree.update_many([1, 2, 3], [bytes(r[:71]) for r in new])
        assert e.value.code == -1
        assert np.array_equal(_nodes(tree), before)
        with pytest.raises(SwmError) as e:
            tree.update(0, 5)
        assert e.value.code == -1
        assert np.array_equal(_nodes(tree), before)
        tree.free()

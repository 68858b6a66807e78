"""CPU tests of the Poseidon Merkle tree's model and of the membership circuit over it: the model (tests/poseidon_tree_model.py)
against its fixture, the circuit's specification workloads.build_poseidon_membership evaluated row by row in Python integers on
honest and tampered assignments, and its SHAPE as the library states it without a GPU (swm_poseidon_tree_circuit_shape,
csrc/host/poseidon_tree_shape.h): the GPU witness synthesis (csrc/poseidon_tree_witness.hip) lays its output out by these counts and
offsets."""
import ctypes
import os
import shutil
import subprocess

import pytest

import poseidon_model as P
import poseidon_tree_model as T
from oracle_lib import golden
from simpleworks_amd import hash as H, marlin as M, workloads as W
from simpleworks_amd._lib import load_library

R = W.R_MODULUS
PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")
HEIGHTS = (2, 3, 6)
LEAF_LENS = (1, 23, 24, 54, 55, 72)   # 8 + n: one | two | three absorbed elements at 23|24 and 54|55, where P_leaf goes 1 -> 2 as well


def le(h):
    return int.from_bytes(bytes.fromhex(h), "little")


@pytest.fixture(scope="module")
def G():
    return golden("poseidon_tree.json")


@pytest.fixture(scope="module")
def ref():
    return P.load_params(PARAMS)


@pytest.fixture(scope="module")
def params():
    return H.PoseidonParameters.from_json(PARAMS)


def _failing_rows(cs, instance=None, witness=None):
    """The row evaluator: every row a z * b z == c z in Python integers; returns the indices of the rows that fail."""
    z = {("i", k): v for k, v in enumerate(cs.instance if instance is None else instance)}
    z.update({("w", k): v for k, v in enumerate(cs.witness if witness is None else witness)})

    def ev(lc):
        return sum(c * z[v] for c, v in lc) % R
    return [i for i, (a, b, c) in enumerate(zip(*cs.rows)) if ev(a) * ev(b) % R != ev(c)]


def _shape(full, partial, alpha, height, leaf_len):
    ni, nw, nc = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = load_library().swm_poseidon_tree_circuit_shape(full, partial, alpha, height, leaf_len, ctypes.byref(ni), ctypes.byref(nw),
                                                        ctypes.byref(nc))
    return rc, (ni.value, nw.value, nc.value)


def _case(ref, height, leaf_len):
    """A leaf, an index with both kinds of bits and a path of random digests; the root by the model."""
    leaf = T.leaf(leaf_len, 0, height)
    levels = height - 1
    index = 0b10110 & ((1 << levels) - 1) if levels > 1 else 1
    siblings = [P.fr("poseidon tree host sibling %d %d %d" % (height, leaf_len, l)) for l in range(levels)]
    return leaf, index, siblings, T.root_of(ref, leaf, index, siblings)


@pytest.fixture(scope="module")
def small(ref, params):
    """height 4, one byte: the 1075-row circuit"""
    leaf, index, siblings, root = _case(ref, 4, 1)
    cs, public = W.poseidon_membership_circuit(params, 4, leaf, index, siblings)
    return cs, public, (leaf, index, siblings, root)


def test_model_against_fixture(G, ref):
    for t in G["trees"]:
        levels = T.build(ref, [T.leaf(t["leaf_len"], i) for i in range(t["n"])])
        assert T.nodes(levels) == [le(h) for h in t["nodes"]], (t["leaf_len"], t["n"])
        assert len(levels) == t["n"].bit_length() and len(levels[-1]) == 1
    for h, chain in G["blank"].items():
        levels = T.blank(ref, int(h))
        assert [level[0] for level in levels] == [le(c) for c in chain] and levels[0][0] == 0
        assert all(len(set(level)) == 1 and len(level) == 1 << (int(h) - 1 - l) for l, level in enumerate(levels))
    for p in G["paths"]:
        t = next(t for t in G["trees"] if (t["leaf_len"], t["n"]) == (p["leaf_len"], p["n"]))
        levels = T.build(ref, [T.leaf(p["leaf_len"], i) for i in range(p["n"])])
        sib = [le(h) for h in p["siblings"]]
        assert T.path(levels, p["index"]) == sib
        root = le(t["nodes"][-1])
        assert T.verify(ref, root, T.leaf(p["leaf_len"], p["index"]), p["index"], sib)
        assert not T.verify(ref, root, T.leaf(p["leaf_len"], p["index"] ^ 1), p["index"], sib)
        assert not T.verify(ref, root, T.leaf(p["leaf_len"], p["index"]), p["index"] ^ 1, sib)


def test_model_update_equals_rebuild(ref):
    leaves = [T.leaf(1, i) for i in range(8)]
    levels = T.build(ref, leaves)
    T.update(ref, levels, [3, 7, 3], [b"a", b"b", b"c"])
    leaves[3], leaves[7] = b"c", b"b"
    assert levels == T.build(ref, leaves)
    first = T.update(ref, T.blank(ref, 3), [0, 1, 2, 3], leaves[:4])
    assert first == T.build(ref, leaves[:4])


@pytest.mark.parametrize("leaf_len", LEAF_LENS)
@pytest.mark.parametrize("height", HEIGHTS)
def test_every_row_holds_and_the_counts_agree(ref, params, height, leaf_len):
    leaf, index, siblings, root = _case(ref, height, leaf_len)
    cs, public = W.poseidon_membership_circuit(params, height, leaf, index, siblings)
    bits = [(byte >> k) & 1 for byte in leaf for k in range(8)]
    assert public == [root] + bits and cs.instance == [1] + public
    assert _failing_rows(cs) == []
    rc, got = _shape(8, 29, 17, height, leaf_len)
    lay = W.poseidon_membership_layout(params, height, leaf_len)
    assert rc == 0 and got == (len(cs.instance), len(cs.witness), cs.num_constraints)
    assert got == (lay["num_instance"], lay["num_witness"], lay["num_constraints"]) == M.poseidon_membership_circuit_shape(params, height, leaf_len)
    levels, c = height - 1, 265
    elems = (8 + leaf_len + 30) // 31
    assert lay["leaf_permutations"] == (elems + 1) // 2 == (1 if leaf_len <= 54 else 2) and lay["permutation_values"] == c
    assert got == (2 + 8 * leaf_len, 3 * levels + (lay["leaf_permutations"] + levels) * c,
                   8 * leaf_len + lay["leaf_permutations"] * c + levels * (2 + c) + 1)
    # the five offsets: index bits, siblings, deltas, then the chains
    w = cs.witness
    assert w[lay["bits"]:lay["bits"] + levels] == [(index >> l) & 1 for l in range(levels)]
    assert w[lay["siblings"]:lay["siblings"] + levels] == siblings
    cur, curs = T.HL(ref, leaf), []
    for l, s in enumerate(siblings):
        curs.append(cur)
        cur = T.H2(ref, s, cur) if (index >> l) & 1 else T.H2(ref, cur, s)
    assert w[lay["deltas"]:lay["deltas"] + levels] == [((index >> l) & 1) * (siblings[l] - curs[l]) % R for l in range(levels)]
    assert lay["leaf"] == 3 * levels and lay["level0"] == lay["leaf"] + lay["leaf_permutations"] * c
    # the first chain value of a level is the square of its state[0] + ark[0][0]
    for l in range(levels):
        x = ((siblings[l] if (index >> l) & 1 else curs[l]) + ref[4][0][0]) % R
        assert w[lay["level0"] + l * c] == x * x % R


def test_the_counts_the_issue_states(G, params):
    assert M.poseidon_membership_circuit_shape(params, 4, 1) == (10, 1069, 1075)
    assert M.poseidon_membership_circuit_shape(params, 19, 72) == (578, 5354, 5913)
    for c in G["counts"]:
        assert list(M.poseidon_membership_circuit_shape(params, c["height"], c["leaf_len"])) == c["counts"]


def test_tampering_makes_a_row_fail(params, small):
    cs, public, (leaf, index, siblings, root) = small
    lay = W.poseidon_membership_layout(params, 4, 1)
    assert _failing_rows(cs) == []
    first_level_row = 8 + 265   # leaf bit rows, leaf chain rows

    def tampered(at, value):
        w = list(cs.witness)
        w[at] = value % R
        return _failing_rows(cs, witness=w)
    for l in range(3):
        # a flipped index bit stays boolean: the row of d_l fails
        bad = tampered(lay["bits"] + l, 1 - cs.witness[lay["bits"] + l])
        assert bad and bad[0] == first_level_row + l * 267 + 1, l
        # a changed sibling
        assert tampered(lay["siblings"] + l, cs.witness[lay["siblings"] + l] + 1), l
        # a changed d_l: its own row
        bad = tampered(lay["deltas"] + l, cs.witness[lay["deltas"] + l] + 1)
        assert bad and bad[0] == first_level_row + l * 267 + 1, l
    # an index bit of two fails its booleanity row
    assert tampered(lay["bits"], 2)[0] == first_level_row
    # a changed chain value: its own row and the next, in the leaf sponge and in a level
    at = lay["leaf"] + 7
    assert tampered(at, cs.witness[at] + 1) == [8 + 7, 8 + 8]
    at = lay["level0"] + 265 + 11
    assert tampered(at, cs.witness[at] + 1) == [first_level_row + 267 + 2 + 11, first_level_row + 267 + 2 + 12]
    # a wrong root: the last row only
    assert _failing_rows(cs, instance=[1, (root + 1) % R] + public[1:]) == [cs.num_constraints - 1]
    wrong, _ = W.poseidon_membership_circuit(params, 4, leaf, index, siblings, root=root + 1)
    assert _failing_rows(wrong) == [wrong.num_constraints - 1]
    # one flipped leaf bit: boolean still, the leaf sponge's first rows fail
    inst = list(cs.instance)
    inst[2 + 3] ^= 1
    bad = _failing_rows(cs, instance=inst)
    assert bad and bad[0] == 8
    inst[2 + 3] = 2
    assert 3 in _failing_rows(cs, instance=inst)


def test_another_leaf_against_the_same_path_is_unsatisfied(ref, params, small):
    """What swm_poseidon_tree_prove_at meets when the leaf is not the tree's: the leaf sponge of the other leaf with the tree's
    running digests."""
    cs, public, (leaf, index, siblings, root) = small
    other, _ = W.poseidon_membership_circuit(params, 4, b"\x00", index, siblings)
    lay = W.poseidon_membership_layout(params, 4, 1)
    w = list(cs.witness)
    w[lay["leaf"]:lay["level0"]] = other.witness[lay["leaf"]:lay["level0"]]
    assert _failing_rows(cs, instance=[1, root] + [0] * 8, witness=w)


def test_synthesizer_class(params, small):
    cs, public, (leaf, index, siblings, root) = small
    again = M.MarlinInst._synthesize(W.PoseidonMerkleTreeVerification(params, root, leaf, index, siblings))
    assert again.witness == cs.witness and again.rows == cs.rows and again.instance == [1] + public


def test_builder_refusals(params):
    for height, leaf_len in ((1, 1), (32, 1), (4, 0), (4, 257)):
        with pytest.raises(ValueError):
            W.poseidon_membership_layout(params, height, leaf_len)
    with pytest.raises(ValueError):
        W.build_poseidon_membership(M.ConstraintSystem(), params, b"", 0, [1, 2])


def test_shape_call_without_a_gpu_and_its_refusals(params):
    lib = load_library()
    n = ctypes.c_size_t(0)
    for args in ((8, 29, 17, 1, 1), (8, 29, 17, 32, 1), (8, 29, 17, 4, 0), (8, 29, 17, 4, 257), (7, 29, 17, 4, 1), (0, 29, 17, 4, 1),
                 (8, 248, 17, 4, 1), (8, 29, 1, 4, 1), (8, 29, 65536, 4, 1), (8, 29, 17, 1 << 62, 1), (8, 29, 17, 4, 1 << 62),
                 (1 << 63, 29, 17, 4, 1), (8, (1 << 64) - 8, 17, 4, 1)):
        assert _shape(*args)[0] == -1, args
    assert lib.swm_last_error(None).decode().startswith("poseidon_tree_circuit_shape")
    assert _shape(8, 29, 17, 31, 256)[0] == 0 and _shape(8, 29, 17, 2, 1)[0] == 0
    assert lib.swm_poseidon_tree_circuit_shape(8, 29, 17, 4, 1, None, ctypes.byref(n), ctypes.byref(n)) == -1
    assert lib.swm_poseidon_tree_circuit_shape(8, 29, 17, 4, 1, ctypes.byref(n), None, ctypes.byref(n)) == -1
    assert lib.swm_poseidon_tree_circuit_shape(8, 29, 17, 4, 1, ctypes.byref(n), ctypes.byref(n), None) == -1
    with pytest.raises(M.MarlinError) as e:
        M.poseidon_membership_circuit_shape(params, 4, 257)
    assert e.value.code == -1


def test_ffi_declares_the_new_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ffi = open(os.path.join(root, "swmarlin-sys", "src", "ffi.rs")).read()
    hdr = open(os.path.join(root, "include", "swmarlin.h")).read()
    names = ("swm_poseidon_tree_create_blank", "swm_poseidon_tree_create_from_leaves", "swm_poseidon_tree_destroy", "swm_poseidon_tree_update",
             "swm_poseidon_tree_root", "swm_poseidon_tree_paths", "swm_poseidon_tree_nodes", "swm_poseidon_tree_dev_nodes",
             "swm_poseidon_verify_paths", "swm_poseidon_tree_circuit_shape", "swm_poseidon_tree_circuit_create",
             "swm_poseidon_tree_circuit_destroy", "swm_poseidon_tree_witness", "swm_poseidon_tree_witness_at", "swm_poseidon_tree_prove",
             "swm_poseidon_tree_prove_at")
    for name in names:
        assert "pub fn %s(" % name in ffi and "%s(" % name in hdr
        assert hasattr(load_library(), name)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shape_under_asan_ubsan(tmp_path):
    """csrc/host/poseidon_tree_shape.h — the counts and offsets the kernel writes witnesses by — against a brute-force walk of what
    the builder allocates, in a stand-alone program (tests/native/poseidon_tree_shape_check.cpp) built with
    -fsanitize=address,undefined."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "poseidon_tree_shape_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(root, "simpleworks_amd", "csrc"), os.path.join(root, "tests", "native", "poseidon_tree_shape_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and ("asan" in out.stderr.lower() or "ubsan" in out.stderr.lower()) and "error:" not in out.stderr:
        pytest.skip("this g++ has no ASan / UBSan runtime")
    assert out.returncode == 0, out.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) >= 256 + 60 + 40 + 2 + 21

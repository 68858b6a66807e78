"""CPU tests of the account-update circuit over a Pedersen account tree (State::register and State::update_balance as one
statement over the reference's own tree): the model of a block of operations applied in order
(tests/pedersen_account_update_model.py), the circuit's specification workloads.build_pedersen_account_update evaluated row by row
in Python integers at heights 2 and 3 — honest registrations (id 0 and id 2^L - 1 included), balances raised and lowered, a wrong
new_root, a wrong old_root, fresh = 1 on an occupied leaf, fresh = 0 on a blank one, a registration that claims an old balance,
fresh = 2, each of the 1160 loose witnesses and the ends of every section group tampered one at a time — its layout and counts also
at heights 4 and 9, and its SHAPE as the library states it without a GPU (swm_pedersen_account_update_circuit_shape,
csrc/host/pedersen_account_update_shape.h): the GPU witness synthesis (csrc/pedersen_account_update_witness.hip) lays its output out
by these counts and offsets."""
import ctypes
import os
import shutil
import subprocess

import pytest

import pedersen_account_update_model as AM
import pedersen_payment_model as PM
from simpleworks_amd import marlin as M, workloads as W
from simpleworks_amd._lib import load_library

R = W.R_MODULUS


@pytest.fixture(scope="module")
def params():
    return W.MerkleParams()


@pytest.fixture(scope="module")
def blocks(params):
    """height -> pedersen_account_update_model.apply of the dependence block from the blank tree, made once."""
    seen = {}

    def get(height):
        if height not in seen:
            table, levels = AM.blank(params, height)
            seen[height] = AM.apply(params, height, table, levels, AM.dependences(height))
        return seen[height]
    return get


@pytest.fixture(scope="module")
def built(params, blocks):
    """(height, index into the dependence block) -> (cs, public inputs) of the honest operation, built once."""
    seen = {}

    def get(height, k):
        if (height, k) not in seen:
            seen[(height, k)] = AM.build(params, height, blocks(height)[0][k])
        return seen[(height, k)]
    return get


def _rows_of(cs):
    return list(zip(*cs.rows))


def _failing_rows(cs, instance=None, witness=None):
    """The row evaluator: every row a z * b z == c z in Python integers; returns the indices of the rows that fail."""
    z = {("i", k): v for k, v in enumerate(cs.instance if instance is None else instance)}
    z.update({("w", k): v for k, v in enumerate(cs.witness if witness is None else witness)})

    def ev(lc):
        return sum(c * z[v] for c, v in lc) % R
    return [i for i, (a, b, c) in enumerate(zip(*cs.rows)) if ev(a) * ev(b) % R != ev(c)]


def _first(ops, fresh, odd=False):
    return next(k for k, t in enumerate(ops) if t["fresh"] == fresh and (not odd or t["id"] & 1))


@pytest.mark.parametrize("height", [2, 3])
def test_model_block(params, blocks, height):
    """The model against itself: the roots chain from the blank root, every old walk is the tree's path to old_root and every new
    walk the path of the new leaf to new_root, and the tree after the block is the tree of the table after the block."""
    ops, table, levels = blocks(height)
    root = PM.tree(params, height, {})[-1][0]
    assert PM.leaf_digest(params, bytes(72)) == 0
    for t in ops:
        assert t["applied"] and t["flag"] == 1 and t["status"] == 0 and t["old_root"] == root
        m = t["id"]
        assert W.pedersen_payment_root(params, t["old_leaf"], m, t["path"]) == t["old_root"] == t["walks"]["old"][-1]
        assert W.pedersen_payment_root(params, t["new_leaf"], m, t["path"]) == t["new_root"] == t["walks"]["new"][-1]
        assert (t["old_leaf"] == bytes(72)) == (t["fresh"] == 1) and t["table"][m] == t["new_leaf"]
        root = t["new_root"]
    assert root == levels[-1][0]
    assert levels == PM.tree(params, height, {i: leaf for i, leaf in enumerate(table) if any(leaf)})
    # the refusals: the status words, and a refused operation moves nothing
    held, cases = AM.refusals(max(height, 3))
    first = AM.apply(params, max(height, 3), *AM.blank(params, max(height, 3)), [(held, AM.REGISTER, AM.key(held), 0)])
    for name, op, st in cases:
        (t,), after, after_levels = AM.apply(params, max(height, 3), first[1], first[2], [op])
        assert (t["status"], t["flag"], t["applied"]) == (st, 0, False), name
        assert t["old_root"] == t["new_root"] and after == first[1] and after_levels == first[2] and t["walks"]["new"] == t["walks"]["old"]


@pytest.mark.parametrize("height", [2, 3])
def test_rows_of_honest_operations(params, blocks, built, height):
    """Every operation of the dependence block: the public inputs are the model's, the counts the layout's, no row fails.  The block
    registers id 0 and id 2^L - 1, raises balances and lowers them (to zero too: the leaf keeps its key and is not blank)."""
    ops, _, _ = blocks(height)
    lay = W.pedersen_account_update_circuit_layout(height)
    last = (1 << (height - 1)) - 1
    assert {(t["id"], t["fresh"]) for t in ops} >= {(0, 1), (last, 1), (0, 0), (last, 0)}
    assert any(t["fresh"] == 0 and t["new_balance"] > t["old_balance"] for t in ops)
    assert any(t["fresh"] == 0 and t["new_balance"] < t["old_balance"] for t in ops)
    leaf_w, lvl_w, upd_w = W.PEDERSEN_PAYMENT_LEAF_WITNESSES, W.PEDERSEN_PAYMENT_LEVEL_WITNESSES, W.PEDERSEN_TRANSFER_LEVEL_WITNESSES
    bits = lambda v, n: [(v >> i) & 1 for i in range(n)]
    for k, t in enumerate(ops):
        cs, public = built(height, k)
        x, y = t["key"]
        assert public == W.account_update_public_inputs(t["old_root"], t["new_root"], t["id"], (x, y), t["old_balance"], t["new_balance"],
                                                        t["fresh"])
        assert cs.instance == [1] + public
        assert (len(cs.instance), len(cs.witness), cs.num_constraints) == (lay["num_instance"], lay["num_witness"], lay["num_constraints"])
        assert _failing_rows(cs) == []
        # the witness groups sit where the layout says
        assert cs.witness[lay["key_bits"]:lay["old_balance"]] == bits(x, 256) + bits(y, 256)
        assert cs.witness[lay["old_balance"]:lay["new_balance"]] == bits(t["old_balance"], 64)
        assert cs.witness[lay["new_balance"]:lay["id_bits"]] == bits(t["new_balance"], 64)
        assert cs.witness[lay["id_bits"]:lay["masked_bits"]] == bits(t["id"], 8)
        assert cs.witness[lay["masked_bits"]:lay["old"]] == ([0] * 512 if t["fresh"] else bits(x, 256) + bits(y, 256))
        m, sibs, old, new = t["id"], t["path"], t["walks"]["old"], t["walks"]["new"]
        assert cs.witness[lay["old"] + leaf_w - 2] == old[0] and cs.witness[lay["new"] + leaf_w - 2] == new[0]
        for l in range(lay["levels"]):
            at = lay["old"] + leaf_w + lvl_w * l
            assert cs.witness[at:at + 3] == [(m >> l) & 1, sibs[l], sibs[l] if (m >> l) & 1 else old[l]]
            assert cs.witness[at + lvl_w - 2] == old[l + 1]
            at = lay["new"] + lay["update"]["level0"] + upd_w * l
            left, right = (sibs[l], new[l]) if (m >> l) & 1 else (new[l], sibs[l])
            assert cs.witness[at] == left
            assert cs.witness[at + 1:at + 513] == bits(left, 256) + bits(right, 256)
            assert cs.witness[at + upd_w - 2] == new[l + 1]


@pytest.mark.parametrize("height", [2, 3])
def test_rows_of_what_can_be_wrong(params, blocks, built, height):
    """A wrong new_root: the last row only.  A wrong old_root: the membership section's root row only.  fresh = 1 on an occupied
    leaf and fresh = 0 on a blank one: the membership section's root row.  fresh = 1 with an old balance: its own row only.
    fresh = 2: the booleanity row, and the mask rows stay satisfied because o is computed honestly."""
    ops, _, _ = blocks(height)
    lay = W.pedersen_account_update_circuit_layout(height)
    assert lay["new_root_row"] == lay["num_constraints"] - 1 and lay["old_root_row"] == lay["new_rows"] - 1
    reg_k, upd_k = _first(ops, 1), _first(ops, 0)
    reg, upd = ops[reg_k], ops[upd_k]
    for k in (reg_k, upd_k):
        cs, public = built(height, k)
        inst = [1] + public
        inst[2] = (inst[2] + 1) % R
        assert _failing_rows(cs, instance=inst) == [lay["new_root_row"]]
        inst = [1] + public
        inst[1] = (inst[1] + 1) % R
        assert _failing_rows(cs, instance=inst) == [lay["old_root_row"]]
    # the same through the builder's own overrides
    wrong, wrong_public = AM.build(params, height, upd, new_root=(upd["new_root"] + 1) % R)
    assert wrong_public[1] == (upd["new_root"] + 1) % R and _failing_rows(wrong) == [lay["new_root_row"]]
    wrong, _ = AM.build(params, height, upd, old_root=(upd["old_root"] + 1) % R)
    assert _failing_rows(wrong) == [lay["old_root_row"]]
    # an occupied leaf registered again: the blank leaf's walk leads elsewhere than the tree's root
    again, _ = AM.build(params, height, upd, fresh=1, old_balance=0, old_root=upd["old_root"])
    assert _failing_rows(again) == [lay["old_root_row"]]
    # a balance update of a blank leaf: the walk from the key's leaf leads elsewhere
    ghost, _ = AM.build(params, height, reg, fresh=0, old_root=reg["old_root"])
    assert _failing_rows(ghost) == [lay["old_root_row"]]
    # a registration cannot claim an old balance: against the tree's root the membership fails too, against the walked one its own row alone
    claim, _ = AM.build(params, height, reg, old_balance=5)
    assert _failing_rows(claim) == [lay["fresh_balance_row"]]
    claim, _ = AM.build(params, height, reg, old_balance=5, old_root=reg["old_root"])
    assert _failing_rows(claim) == [lay["fresh_balance_row"], lay["old_root_row"]]
    # fresh is a bit
    two, public = AM.build(params, height, reg, fresh=2)
    failing = _failing_rows(two)
    assert public[7] == 2 and lay["fresh_row"] in failing
    assert not set(failing) & set(range(lay["mask_rows"], lay["old_rows"]))
    assert two.witness[lay["masked_bits"]:lay["old"]] == [(R - v) % R for v in two.witness[lay["key_bits"]:lay["old_balance"]]]
    # an id at or above 2^L walks the path of its low bits and fails an index row
    high, _ = AM.build(params, height, reg, index=reg["id"] + (1 << (height - 1)))
    assert _failing_rows(high) == [lay["old_root_row"] - 8 + height - 1]


@pytest.mark.parametrize("height", [2, 3])
def test_a_tampered_witness_fails_some_row(params, blocks, built, height):
    """Each of the 1160 loose witnesses changed by one, one at a time, and the first and the last witness of every group of the two
    sections (the leaf hash, and per level dir | sibling | left, the bits, the additions): some row that names it fails.  Only rows
    that name the witness can change, so only those are evaluated."""
    ops, _, _ = blocks(height)
    lay = W.pedersen_account_update_circuit_layout(height)
    leaf_w, lvl_w, upd_w = W.PEDERSEN_PAYMENT_LEAF_WITNESSES, W.PEDERSEN_PAYMENT_LEVEL_WITNESSES, W.PEDERSEN_TRANSFER_LEVEL_WITNESSES
    picks = list(range(W.PEDERSEN_ACCOUNT_UPDATE_LOOSE))
    groups = [(lay["old"], leaf_w), (lay["new"], leaf_w)]
    for l in range(lay["levels"]):
        at = lay["old"] + leaf_w + lvl_w * l
        groups += [(at, 3), (at + 3, 512), (at + 515, lvl_w - 515)]
        at = lay["new"] + leaf_w + upd_w * l
        groups += [(at, 1), (at + 1, 512), (at + 513, upd_w - 513)]
    assert sum(n for _, n in groups) == lay["num_witness"] - W.PEDERSEN_ACCOUNT_UPDATE_LOOSE
    assert groups[-1][0] + groups[-1][1] == lay["num_witness"]
    for at, n in groups:
        picks += [at, at + n - 1]
    for k in (_first(ops, 1), _first(ops, 0, odd=True)):
        cs, _ = built(height, k)
        named = {}
        rows = _rows_of(cs)
        for i, row in enumerate(rows):
            for lc in row:
                for _, v in lc:
                    if v[0] == "w":
                        named.setdefault(v[1], set()).add(i)
        assert sorted(named) == list(range(len(cs.witness)))
        z = {("i", j): v for j, v in enumerate(cs.instance)}
        z.update({("w", j): v for j, v in enumerate(cs.witness)})
        ev = lambda lc: sum(c * z[v] for c, v in lc) % R
        for j in picks:
            z[("w", j)] = (cs.witness[j] + 1) % R
            assert any(ev(rows[i][0]) * ev(rows[i][1]) % R != ev(rows[i][2]) for i in named[j]), (height, ops[k]["fresh"], j)
            z[("w", j)] = cs.witness[j]


class _CountingSystem:
    """The builder's vocabulary, counting and keeping nothing."""

    def __init__(self):
        self.instance, self.witness, self.num_constraints = 1, 0, 0

    @staticmethod
    def one():
        return ("i", 0)

    def new_input_variable(self, value):
        self.instance += 1
        return ("i", self.instance - 1)

    def new_witness_variable(self, value):
        self.witness += 1
        return ("w", self.witness - 1)

    def enforce_constraint(self, a, b, c):
        self.num_constraints += 1


def _shape(height):
    ni, nw, nc = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = load_library().swm_pedersen_account_update_circuit_shape(height, ctypes.byref(ni), ctypes.byref(nw), ctypes.byref(nc))
    return rc, (ni.value, nw.value, nc.value)


def test_layout_equals_the_c_shape_at_every_height_and_the_built_counts(params):
    for height in range(2, 10):
        lay = W.pedersen_account_update_circuit_layout(height)
        got = (lay["num_instance"], lay["num_witness"], lay["num_constraints"])
        assert _shape(height) == (0, got) and M.pedersen_account_update_circuit_shape(height) == got
        levels = height - 1
        assert got == (9, 1160 + (3450 + 3581 * levels) + (3450 + 3579 * levels), 1167 + (3459 + 3588 * levels) + (3451 + 3587 * levels))
    # the built system's counts: the shape does not depend on the values, a registration at id 0 with zero siblings and the roots given
    # serves every height
    for height in (2, 3, 4, 9):
        cs = _CountingSystem()
        W.build_pedersen_account_update(cs, params, height, 0, (3, 5), 0, 7, 1, [0] * (height - 1), old_root=0, new_root=0)
        lay = W.pedersen_account_update_circuit_layout(height)
        assert (cs.instance, cs.witness, cs.num_constraints) == (lay["num_instance"], lay["num_witness"], lay["num_constraints"])
    assert (cs.instance, cs.witness, cs.num_constraints) == (9, 65340, 65477)      # the worked numbers at height 9: |H| = 2^16, 59 rows to spare
    for height in (1, 10):
        with pytest.raises(ValueError):
            W.pedersen_account_update_circuit_layout(height)
        assert _shape(height)[0] == -1
        with pytest.raises(M.MarlinError) as e:
            M.pedersen_account_update_circuit_shape(height)
        assert e.value.code == -1


def test_synthesizer_class_and_builder_refusals(params, blocks, built):
    t = blocks(2)[0][1]
    cs, public = built(2, 1)
    again = M.MarlinInst._synthesize(W.PedersenAccountUpdate(params, 2, public[0], public[1], t["id"], t["key"], t["old_balance"],
                                                             t["new_balance"], t["fresh"], t["path"]))
    assert again.witness == cs.witness and again.rows == cs.rows and again.instance == [1] + public
    for kw in (dict(index=256), dict(index=-1), dict(key=(1 << 256, 0)), dict(key=(0, -1)), dict(old_balance=1 << 64), dict(new_balance=-1),
               dict(siblings=t["path"] + [0]), dict(siblings=[])):
        with pytest.raises(ValueError):
            AM.build(params, 2, t, **kw)
    for height in (1, 10):
        with pytest.raises(ValueError):
            AM.build(params, height, t, siblings=[0] * (height - 1))
    with pytest.raises(ValueError):       # a leaf CRH that does not hold 72 bytes
        AM.build(W.MerkleParams(generators=(params.leaf_gens[:143], params.inner_gens)), 2, t)
    with pytest.raises(ValueError):       # a two-to-one CRH that does not hold two digests
        AM.build(W.MerkleParams(generators=(params.leaf_gens, params.inner_gens[:127])), 2, t)
    # the key is packed unreduced: a coordinate of r + 1 publishes 1
    _, public = AM.build(params, 2, t, key=(R + 1, t["key"][1]))
    assert public[3] == 1


def test_shape_call_refusals():
    lib = load_library()
    n = ctypes.c_size_t(0)
    for height in (0, 1, 10, 31, 1 << 62):
        assert _shape(height)[0] == -1, height
    assert lib.swm_last_error(None).decode().startswith("pedersen_account_update_circuit_shape")
    assert lib.swm_pedersen_account_update_circuit_shape(4, None, ctypes.byref(n), ctypes.byref(n)) == -1
    assert lib.swm_pedersen_account_update_circuit_shape(4, ctypes.byref(n), None, ctypes.byref(n)) == -1
    assert lib.swm_pedersen_account_update_circuit_shape(4, ctypes.byref(n), ctypes.byref(n), None) == -1


def test_header_and_ffi_declare_the_new_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ffi = open(os.path.join(root, "swmarlin-sys", "src", "ffi.rs")).read()
    hdr = open(os.path.join(root, "include", "swmarlin.h")).read()
    names = ("swm_pedersen_account_update_circuit_shape", "swm_pedersen_account_update_circuit_create",
             "swm_pedersen_account_update_circuit_destroy", "swm_pedersen_account_update_witness_at",
             "swm_pedersen_account_update_prove_at", "swm_pedersen_account_update_prove_many_at")
    for name in names:
        assert "pub fn %s(" % name in ffi and "%s(" % name in hdr
        assert hasattr(load_library(), name)


LAYOUT_KEYS = ("num_instance", "num_witness", "num_constraints", "key_bits", "old_balance", "new_balance", "id_bits", "masked_bits", "old",
               "new", "membership_witnesses", "update_witnesses", "section_rows", "update_rows", "pack_rows", "fresh_row",
               "fresh_balance_row", "mask_rows", "old_rows", "old_root_row", "new_rows", "new_root_row", "levels")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shape_under_asan_ubsan(tmp_path):
    """csrc/host/pedersen_account_update_shape.h — the counts, offsets and named rows the kernels write witnesses by — in a
    stand-alone program (tests/native/pedersen_account_update_shape_check.cpp) built with -fsanitize=address,undefined: every height
    2 .. 9 against the formulas, a cover of [0, num_witness) by its groups, its refusals, and the numbers of
    pedersen_account_update_circuit_layout() at every height, handed over on the command line."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "pedersen_account_update_shape_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(root, "simpleworks_amd", "csrc"),
           os.path.join(root, "tests", "native", "pedersen_account_update_shape_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and ("asan" in out.stderr.lower() or "ubsan" in out.stderr.lower()) and "error:" not in out.stderr:
        pytest.skip("this g++ has no ASan / UBSan runtime")
    assert out.returncode == 0, out.stderr[-4000:]
    args = []
    for height in range(2, 10):
        lay = W.pedersen_account_update_circuit_layout(height)
        args += [str(height)] + [str(lay[k]) for k in LAYOUT_KEYS]
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) == 8 + 8 + 1 + 5
    # a number that is not the header's is noticed
    lay = W.pedersen_account_update_circuit_layout(4)
    bad = ["4"] + [str(lay[k] + (1 if k == "mask_rows" else 0)) for k in LAYOUT_KEYS]
    assert subprocess.run([exe] + bad, capture_output=True, text=True, timeout=300).returncode != 0

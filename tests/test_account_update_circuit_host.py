"""CPU tests of the account-update circuit (State::register and State::update_balance as one statement over a Poseidon account
tree): the model of a block of operations applied in order (tests/account_update_model.py) against its fixture, the circuit's
specification workloads.build_account_update evaluated row by row in Python integers at heights 2, 4 and 9 — honest registrations
(id 0 and id 2^L - 1 included), balances raised and lowered, a wrong new_root, a wrong old_root, fresh = 1 on an occupied leaf,
fresh = 0 on a blank one, a registration that claims an old balance, fresh = 2, every witness tampered one at a time — and its SHAPE
as the library states it without a GPU (swm_account_update_circuit_shape, csrc/host/account_update_shape.h): the GPU witness
synthesis (csrc/account_update_witness.hip) lays its output out by these counts and offsets."""
import ctypes
import hashlib
import os
import shutil
import subprocess

import pytest

import account_update_model as AM
import poseidon_model as P
from oracle_lib import golden
from simpleworks_amd import hash as H, marlin as M, workloads as W
from simpleworks_amd._lib import load_library

R = W.R_MODULUS
PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")
C = 265     # chain values per permutation of the reference's parameters: (3 * 8 + 29) * 5


def le(h):
    return int.from_bytes(bytes.fromhex(h), "little")


@pytest.fixture(scope="module")
def ref():
    return P.load_params(PARAMS)


@pytest.fixture(scope="module")
def params():
    return H.PoseidonParameters.from_json(PARAMS)


@pytest.fixture(scope="module")
def blocks(ref):
    """height -> account_update_model.apply of the dependence block from the blank tree, made once."""
    seen = {}

    def get(height):
        if height not in seen:
            table, levels = AM.blank(ref, height)
            seen[height] = AM.apply(ref, height, table, levels, AM.dependences(height))
        return seen[height]
    return get


def _rows_of(cs):
    return list(zip(*cs.rows))


def _failing_rows(cs, instance=None, witness=None, only=None):
    """The row evaluator: every row a z * b z == c z in Python integers; returns the indices of the rows that fail (of `only`)."""
    z = {("i", k): v for k, v in enumerate(cs.instance if instance is None else instance)}
    z.update({("w", k): v for k, v in enumerate(cs.witness if witness is None else witness)})

    def ev(lc):
        return sum(c * z[v] for c, v in lc) % R
    rows = _rows_of(cs)
    return [i for i in (range(len(rows)) if only is None else only) if ev(rows[i][0]) * ev(rows[i][1]) % R != ev(rows[i][2])]


def _build(params, height, t, **kw):
    args = dict(index=t["id"], key=t["key"], old_balance=t["old_balance"], new_balance=t["new_balance"], fresh=t["fresh"], siblings=t["path"])
    args.update(kw)
    return W.account_update_circuit(params, height, **args)


def _witness_digest(cs):
    return hashlib.sha256(b"".join(v.to_bytes(32, "little") for v in cs.witness)).hexdigest()


def test_model_and_builder_against_fixture(ref, params, blocks):
    G = golden("account_update.json")
    height = G["height"]
    ops, table, levels = blocks(height)
    assert [[t["op"][0], t["op"][1], t["op"][2].hex(), t["op"][3]] for t in ops] == G["ops"]
    assert levels[-1][0] == le(G["final_root"]) and AM.blank(ref, height)[1][-1][0] == le(G["blank_root"])
    assert {str(i): leaf.hex() for i, leaf in enumerate(table) if any(leaf)} == G["final_accounts"]
    root = le(G["blank_root"])
    for t, g in zip(ops, G["items"]):
        cs, public = _build(params, height, t)
        assert public == [le(v) for v in g["public"]] and t["path"] == [le(v) for v in g["path"]]
        assert (t["status"], t["applied"]) == (g["status"], True) and public[0] == root
        assert (len(cs.witness), cs.num_constraints, _witness_digest(cs)) == (g["num_witness"], g["num_constraints"], g["witness_sha256"])
        root = public[1]
    assert root == le(G["final_root"])
    # the refusals of the fixture's second block: the model's status words
    held, cases = AM.refusals(height)
    assert [[name, op[0], op[1], op[2].hex(), op[3], st] for name, op, st in cases] == G["refusals"]


@pytest.mark.parametrize("height", [2, 4, 9])
def test_rows_of_honest_operations(params, blocks, height):
    """Every operation of the dependence block: the public inputs are the model's, the counts the layout's, no row fails.  The block
    registers id 0 and id 2^L - 1, raises balances and lowers them (to zero too: the leaf keeps its key and is not blank)."""
    ops, _, _ = blocks(height)
    lay = W.account_update_circuit_layout(params, height)
    last = (1 << (height - 1)) - 1
    assert {(t["id"], t["fresh"]) for t in ops} >= {(0, 1), (last, 1), (0, 0), (last, 0)}
    assert any(t["fresh"] == 0 and t["new_balance"] > t["old_balance"] for t in ops)
    assert any(t["fresh"] == 0 and t["new_balance"] < t["old_balance"] for t in ops)
    for t in ops:
        cs, public = _build(params, height, t)
        x, y = t["key"]
        assert public == W.account_update_public_inputs(t["old_root"], t["new_root"], t["id"], (x, y), t["old_balance"], t["new_balance"],
                                                        t["fresh"])
        assert cs.instance == [1] + public and t["applied"]
        assert (len(cs.instance), len(cs.witness), cs.num_constraints) == (lay["num_instance"], lay["num_witness"], lay["num_constraints"])
        assert _failing_rows(cs) == []
        # the witness groups sit where the layout says
        bits = lambda v, n: [(v >> i) & 1 for i in range(n)]
        assert cs.witness[lay["key_bits"]:lay["old_balance"]] == bits(x, 256) + bits(y, 256)
        assert cs.witness[lay["old_balance"]:lay["new_balance"]] == bits(t["old_balance"], 64)
        assert cs.witness[lay["new_balance"]:lay["id_bits"]] == bits(t["new_balance"], 64)
        assert cs.witness[lay["id_bits"]:lay["cur0"]] == bits(t["id"], 8)
        mb, levels = lay["membership"], lay["levels"]
        assert cs.witness[lay["old"] + mb["bits"]:lay["old"] + mb["bits"] + levels] == bits(t["id"], levels)
        assert cs.witness[lay["old"] + mb["siblings"]:lay["old"] + mb["siblings"] + levels] == t["path"]
        assert (cs.witness[lay["cur0"]] == 0) == (t["fresh"] == 1)
    if height == 9:
        assert (len(cs.instance), len(cs.witness), cs.num_constraints) == (9, 5981, 5990)      # the worked numbers


@pytest.mark.parametrize("height", [2, 4, 9])
def test_rows_of_what_can_be_wrong(params, blocks, height):
    """A wrong new_root: the last row only.  A wrong old_root: the membership's root row only.  fresh = 1 on an occupied leaf and
    fresh = 0 on a blank one: the membership's root row.  fresh = 1 with an old balance: its own row only.  fresh = 2: the
    booleanity row."""
    ops, _, _ = blocks(height)
    lay = W.account_update_circuit_layout(params, height)
    assert lay["new_root_row"] == lay["num_constraints"] - 1
    reg = next(t for t in ops if t["fresh"] == 1)
    upd = next(t for t in ops if t["fresh"] == 0)
    for t in (reg, upd):
        cs, public = _build(params, height, t)
        inst = [1] + public
        inst[2] = (inst[2] + 1) % R
        assert _failing_rows(cs, instance=inst) == [lay["new_root_row"]]
        inst = [1] + public
        inst[1] = (inst[1] + 1) % R
        assert _failing_rows(cs, instance=inst) == [lay["old_root_row"]]
    # the same through the builder's own overrides
    wrong, wrong_public = _build(params, height, upd, new_root=(upd["new_root"] + 1) % R)
    assert wrong_public[1] == (upd["new_root"] + 1) % R and _failing_rows(wrong) == [lay["new_root_row"]]
    wrong, _ = _build(params, height, upd, old_root=(upd["old_root"] + 1) % R)
    assert _failing_rows(wrong) == [lay["old_root_row"]]
    # an occupied leaf registered again: the walk from the zero digest leads elsewhere than the tree's root
    again, _ = _build(params, height, upd, fresh=1, old_balance=0, old_root=upd["old_root"])
    assert _failing_rows(again) == [lay["old_root_row"]]
    # a balance update of a blank leaf: the walk from the leaf's hash leads elsewhere
    ghost, _ = _build(params, height, reg, fresh=0, old_root=reg["old_root"])
    assert _failing_rows(ghost) == [lay["old_root_row"]]
    # a registration cannot claim an old balance
    claim, _ = _build(params, height, reg, old_balance=5)
    assert _failing_rows(claim) == [lay["fresh_balance_row"]]
    # fresh is a bit
    two, public = _build(params, height, reg, fresh=2)
    assert public[7] == 2 and lay["fresh_row"] in _failing_rows(two)
    # an id at or above 2^L walks the path of its low bits and fails an index row
    if height < 9:
        high, _ = _build(params, height, reg, index=reg["id"] + (1 << (height - 1)))
        assert _failing_rows(high) == [lay["old_rows"] + height - 1]


@pytest.mark.parametrize("height,stride", [(2, 1), (4, 1), (9, 3)])
def test_a_tampered_witness_fails_some_row(params, blocks, height, stride):
    """Each witness changed by one, one at a time (every third at height 9): some row that names it fails.  Only rows that name the
    witness can change, so only those are evaluated."""
    ops, _, _ = blocks(height)
    for t in (next(t for t in ops if t["fresh"] == 1), next(t for t in ops if t["fresh"] == 0 and t["id"] & 1)):
        cs, _ = _build(params, height, t)
        named = {}
        for i, row in enumerate(_rows_of(cs)):
            for lc in row:
                for _, v in lc:
                    if v[0] == "w":
                        named.setdefault(v[1], set()).add(i)
        assert sorted(named) == list(range(len(cs.witness)))
        rows = _rows_of(cs)
        z = {("i", k): v for k, v in enumerate(cs.instance)}
        z.update({("w", k): v for k, v in enumerate(cs.witness)})
        ev = lambda lc: sum(c * z[v] for c, v in lc) % R
        for k in range(0, len(cs.witness), stride):
            z[("w", k)] = (cs.witness[k] + 1) % R
            assert any(ev(rows[i][0]) * ev(rows[i][1]) % R != ev(rows[i][2]) for i in named[k]), (height, t["fresh"], k)
            z[("w", k)] = cs.witness[k]


def _shape(full, partial, alpha, height):
    ni, nw, nc = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = load_library().swm_account_update_circuit_shape(full, partial, alpha, height, ctypes.byref(ni), ctypes.byref(nw), ctypes.byref(nc))
    return rc, (ni.value, nw.value, nc.value)


def test_layout_equals_the_c_shape_at_every_height(params):
    for height in range(2, 10):
        lay = W.account_update_circuit_layout(params, height)
        got = (lay["num_instance"], lay["num_witness"], lay["num_constraints"])
        assert _shape(8, 29, 17, height) == (0, got) and M.account_update_circuit_shape(params, height) == got
        levels = height - 1
        m = 3 * levels + (2 + levels) * C
        assert got == (9, 649 + 2 * m - 2 * levels, 655 + (8 + 2 * C + 1 + levels * (2 + C) + 1) + (2 * C + levels * (1 + C) + 1))
    for height in (1, 10):
        with pytest.raises(ValueError):
            W.account_update_circuit_layout(params, height)
        assert _shape(8, 29, 17, height)[0] == -1
        with pytest.raises(M.MarlinError) as e:
            M.account_update_circuit_shape(params, height)
        assert e.value.code == -1


def test_synthesizer_class_and_builder_refusals(params, blocks):
    t = blocks(2)[0][1]
    cs, public = _build(params, 2, t)
    again = M.MarlinInst._synthesize(W.AccountUpdate(params, 2, public[0], public[1], t["id"], t["key"], t["old_balance"], t["new_balance"],
                                                     t["fresh"], t["path"]))
    assert again.witness == cs.witness and again.rows == cs.rows and again.instance == [1] + public
    for kw in (dict(index=256), dict(index=-1), dict(key=(1 << 256, 0)), dict(key=(0, -1)), dict(old_balance=1 << 64), dict(new_balance=-1),
               dict(siblings=t["path"] + [0]), dict(siblings=[])):
        with pytest.raises(ValueError):
            _build(params, 2, t, **kw)
    # the key is packed unreduced: a coordinate of r + 1 publishes 1
    _, public = _build(params, 2, t, key=(R + 1, t["key"][1]))
    assert public[3] == 1


def test_shape_call_refusals():
    lib = load_library()
    n = ctypes.c_size_t(0)
    for args in ((8, 29, 17, 1), (8, 29, 17, 10), (8, 29, 17, 31), (7, 29, 17, 4), (0, 29, 17, 4), (8, 248, 17, 4), (8, 29, 1, 4),
                 (8, 29, 65536, 4), (8, 29, 17, 1 << 62), (1 << 63, 29, 17, 4), (8, (1 << 64) - 8, 17, 4)):
        assert _shape(*args)[0] == -1, args
    assert lib.swm_last_error(None).decode().startswith("account_update_circuit_shape")
    assert lib.swm_account_update_circuit_shape(8, 29, 17, 4, None, ctypes.byref(n), ctypes.byref(n)) == -1
    assert lib.swm_account_update_circuit_shape(8, 29, 17, 4, ctypes.byref(n), None, ctypes.byref(n)) == -1
    assert lib.swm_account_update_circuit_shape(8, 29, 17, 4, ctypes.byref(n), ctypes.byref(n), None) == -1


def test_ffi_declares_the_new_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ffi = open(os.path.join(root, "swmarlin-sys", "src", "ffi.rs")).read()
    hdr = open(os.path.join(root, "include", "swmarlin.h")).read()
    names = ("swm_account_update_circuit_shape", "swm_account_update_circuit_create", "swm_account_update_circuit_destroy",
             "swm_account_update_witness_at", "swm_account_update_prove_at", "swm_account_update_prove_many_at")
    for name in names:
        assert "pub fn %s(" % name in ffi and "%s(" % name in hdr
        assert hasattr(load_library(), name)


LAYOUT_KEYS = ("num_instance", "num_witness", "num_constraints", "key_bits", "old_balance", "new_balance", "id_bits", "cur0", "old", "new",
               "membership_witnesses", "update_witnesses", "pack_rows", "fresh_row", "fresh_balance_row", "old_rows", "mask_row", "old_root_row",
               "new_rows", "new_root_row")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shape_under_asan_ubsan(tmp_path, params):
    """csrc/host/account_update_shape.h — the counts, offsets and named rows the kernels write witnesses by — in a stand-alone
    program (tests/native/account_update_shape_check.cpp) built with -fsanitize=address,undefined: against the formulas, a cover of
    [0, num_witness) by its groups, its refusals, and the numbers of account_update_circuit_layout() at heights 2, 4 and 9, handed
    over on the command line."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "account_update_shape_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(root, "simpleworks_amd", "csrc"), os.path.join(root, "tests", "native", "account_update_shape_check.cpp"),
           "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and ("asan" in out.stderr.lower() or "ubsan" in out.stderr.lower()) and "error:" not in out.stderr:
        pytest.skip("this g++ has no ASan / UBSan runtime")
    assert out.returncode == 0, out.stderr[-4000:]
    args = []
    for height in (2, 4, 9):
        lay = W.account_update_circuit_layout(params, height)
        args += [str(height)] + [str(lay[k]) for k in LAYOUT_KEYS]
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) >= 8 * 5 * 6 + 17 + 3
    # a number that is not the header's is noticed
    lay = W.account_update_circuit_layout(params, 4)
    bad = ["4"] + [str(lay[k] + (1 if k == "mask_row" else 0)) for k in LAYOUT_KEYS]
    assert subprocess.run([exe] + bad, capture_output=True, text=True, timeout=300).returncode != 0

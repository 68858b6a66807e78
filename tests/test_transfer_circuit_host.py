"""CPU tests of the transfer circuit: the model of a small ledger and a block of transfers applied in order
(tests/transfer_model.py) against its fixture, the circuit's specification workloads.build_transfer evaluated row by row in Python
integers at heights 2, 4 and 9 — a valid transfer, a wrong new_root, a wrong R1, an overflow, an overdraft, a recipient sibling
taken from the old tree — and its SHAPE as the library states it without a GPU (swm_transfer_circuit_shape,
csrc/host/transfer_shape.h): the GPU witness synthesis (csrc/transfer_witness.hip) lays its output out by these counts and
offsets."""
import ctypes
import os
import shutil
import subprocess

import pytest

import poseidon_model as P
import poseidon_tree_model as T
import schnorr_model as S
import transfer_model as TM
from oracle_lib import golden
from simpleworks_amd import hash as H, marlin as M, workloads as W
from simpleworks_amd._lib import load_library

R = W.R_MODULUS
PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")
SALT = bytes(range(32))
C = 265     # chain values per permutation of the reference's parameters: (3 * 8 + 29) * 5
VALID = {2: "zero to one", 4: "meet at level 0", 9: "meet at level 0"}


def le(h):
    return int.from_bytes(bytes.fromhex(h), "little")


@pytest.fixture(scope="module")
def G():
    return golden("transfer.json")


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


def _build(params, height, t, salt=None, **kw):
    return W.transfer_circuit(params, height, t["message"], t["signature"], t["sender_leaf"], t["sender_path"], t["recipient_leaf"],
                              t["recipient_path"], salt=salt, **kw)


@pytest.fixture(scope="module")
def blocks(ref):
    seen = {}

    def get(height, salt=None):
        if (height, salt) not in seen:
            seen[(height, salt)] = TM.transfers(ref, height, salt)
        return seen[(height, salt)]
    return get


def test_model_against_fixture(G, ref, blocks):
    first, block, table, levels = blocks(G["height"])
    held = lambda tab: {str(i): leaf.hex() for i, leaf in enumerate(tab) if any(leaf)}
    assert held(first) == G["accounts"] and held(table) == G["final_accounts"]
    assert TM.ledger(ref, G["height"])[1][-1][0] == le(G["root"]) and levels[-1][0] == le(G["final_root"])
    assert [t["name"] for t in block] == [g["name"] for g in G["transfers"]] == [t[0] for t in TM.TRANSFERS]
    root = le(G["root"])
    for t, g in zip(block, G["transfers"]):
        for k in ("message", "signature", "sender_leaf", "recipient_leaf"):
            assert t[k].hex() == g[k], (t["name"], k)
        assert t["sender_path"] == [le(h) for h in g["sender_path"]] and t["recipient_path"] == [le(h) for h in g["recipient_path"]]
        assert t["public"] == [le(h) for h in g["public"][:2]] + g["public"][2:] and t["r1"] == le(g["r1"])
        assert (t["flag"], t["status"], t["wrong"]) == (g["flag"], g["status"], g["wrong"])
        assert {str(i): int.from_bytes(leaf[64:], "little") for i, leaf in enumerate(t["table"]) if any(leaf)} == g["balances"]
        # the roots chain, a refused transfer publishes equal roots, and the flag says why
        assert t["public"][0] == root and t["applied"] == (t["wrong"] is None) == bool(t["flag"] & 16)
        assert (t["public"][1] != root) == (t["applied"] and t["public"][4] > 0)      # amount zero is applied and changes nothing
        root = t["public"][1]
        want = {None: 31, "overflow": 15 - 4, "overdraft": 15 - 2, "signature": 15 - 1, "recipient": 15 - 8, "self": 15, "id": 15}[t["wrong"]]
        assert t["flag"] == want and t["status"] == {"self": 8, "id": 4}.get(t["wrong"], 0)
        # the sender's leaf is in the tree before, the recipient's in the intermediate tree
        msg = t["message"]
        mask = (1 << (G["height"] - 1)) - 1
        assert T.root_of(ref, t["sender_leaf"], msg[0] & mask, t["sender_path"]) == t["public"][0]
        if t["wrong"] != "recipient":
            assert T.root_of(ref, t["recipient_leaf"], msg[1] & mask, t["recipient_path"]) == t["r1"]
    assert root == le(G["final_root"])
    by_name = {g["name"]: g for g in G["transfers"]}
    amount = lambda name: by_name[name]["public"][4]
    balance = lambda name, k: int.from_bytes(bytes.fromhex(by_name[name][k])[64:], "little")
    assert amount("amount zero") == 0 and amount("whole balance") == balance("whole balance", "sender_leaf")
    assert balance("sum 2^64 - 1", "recipient_leaf") + amount("sum 2^64 - 1") == (1 << 64) - 1
    assert balance("overflow by 1", "recipient_leaf") + amount("overflow by 1") == 1 << 64
    assert amount("overdraft by 1") == balance("overdraft by 1", "sender_leaf") + 1


@pytest.mark.parametrize("height", [2, 4, 9])
def test_rows_of_a_transfer_and_of_what_can_be_wrong_with_it(ref, params, blocks, height):
    """A valid transfer: no failing row.  A wrong new_root: the last root row only.  A wrong R1: the two R1 rows only.  An overflow:
    the sum packing row only.  An overdraft: the diff packing row only.  A recipient sibling taken from the OLD tree: the
    recipient's R1 row only (where the two paths meet below the root)."""
    t = next(t for t in blocks(height)[1] if t["name"] == VALID[height])
    lay = W.transfer_circuit_layout(params, height)
    cs, public = _build(params, height, t)
    assert public == t["public"] and cs.instance == [1] + public and cs.witness[lay["r1"]] == t["r1"]
    assert (len(cs.instance), len(cs.witness), cs.num_constraints) == (lay["num_instance"], lay["num_witness"], lay["num_constraints"])
    assert _failing_rows(cs) == []
    assert lay["new_root_row"] == cs.num_constraints - 1
    inst = [1] + public
    inst[2] = (inst[2] + 1) % R
    assert _failing_rows(cs, instance=inst) == [lay["new_root_row"]]
    inst = [1] + public
    inst[1] = (inst[1] + 1) % R
    assert _failing_rows(cs, instance=inst) == [lay["sender_root_row"]]
    w = list(cs.witness)
    w[lay["r1"]] = (w[lay["r1"]] + 1) % R
    assert _failing_rows(cs, witness=w) == [lay["sender_r1_row"], lay["recipient_r1_row"]]
    amount = public[4]
    assert amount > 0
    # the witness groups sit where the layout says
    balance, rbalance = int.from_bytes(t["sender_leaf"][64:], "little"), int.from_bytes(t["recipient_leaf"][64:], "little")
    bits = lambda v: [(v >> i) & 1 for i in range(64)]
    assert cs.witness[lay["balance"]:lay["diff"]] == bits(balance) and cs.witness[lay["diff"]:lay["sender"]] == bits(balance - amount)
    assert cs.witness[lay["sum"]:lay["recipient_update"]] == bits(rbalance + amount)
    assert cs.witness[lay["recipient_bits"]:lay["recipient"]] == [(byte >> i) & 1 for byte in t["recipient_leaf"] for i in range(8)]
    mb, levels = lay["membership"], lay["levels"]
    assert cs.witness[lay["recipient"] + mb["siblings"]:lay["recipient"] + mb["siblings"] + levels] == t["recipient_path"]
    # an overflow by one, an overdraft by one: the same transfer over a ledger whose balances say so
    which = [c for c in TM.TRANSFERS if c[0] == VALID[height]]
    sender, recipient = t["message"][0], t["message"][1]
    over = TM.transfers(ref, height, which=which, balances={recipient: (1 << 64) - amount})[1][0]
    assert over["flag"] == 15 - 4 and over["message"] == t["message"]
    assert _failing_rows(_build(params, height, over)[0]) == [lay["sum_pack_row"]]
    under = TM.transfers(ref, height, which=which, balances={sender: amount - 1})[1][0]
    assert under["flag"] == 15 - 2 and under["message"] == t["message"]
    assert _failing_rows(_build(params, height, under)[0]) == [lay["pack_row"]]
    if height > 2:
        # 2 -> 3: the paths meet at level 0, below the root; the old tree's path differs from the intermediate tree's there alone
        differ = [l for l in range(levels) if t["old_recipient_path"][l] != t["recipient_path"][l]]
        assert differ == [0]
        stale, stale_public = _build(params, height, dict(t, recipient_path=t["old_recipient_path"]))
        assert _failing_rows(stale) == [lay["recipient_r1_row"]] and stale_public[1] != public[1]
    if height == 4:
        # the same through the builder's own overrides
        wrong, wrong_public = _build(params, height, t, new_root=(public[1] + 1) % R)
        assert wrong_public[1] == (public[1] + 1) % R and _failing_rows(wrong) == [lay["new_root_row"]]
        wrong, _ = _build(params, height, t, r1=(t["r1"] + 1) % R)
        assert _failing_rows(wrong) == [lay["sender_r1_row"], lay["recipient_r1_row"]]
    if height == 9:
        assert (len(cs.instance), len(cs.witness), cs.num_constraints) == (6, 82578, 83569)      # the worked numbers
        assert [int(m[0][-1]) for m in cs.pack().mats] == [216490, 177271, 113681]


def test_every_refusal_of_the_block_fails_its_own_rows(G, params, blocks):
    lay = W.transfer_circuit_layout(params, G["height"])
    s_rows = lay["schnorr"]["num_constraints"]
    for t in blocks(G["height"])[1]:
        if t["wrong"] in (None, "overflow", "overdraft"):
            continue        # the test above
        failing = _failing_rows(_build(params, G["height"], t)[0])
        if t["wrong"] == "signature":
            assert failing and set(failing) <= set(range(s_rows - 8, s_rows))
        elif t["wrong"] == "recipient":
            assert failing == [lay["recipient_r1_row"]]
        elif t["wrong"] == "self":
            assert failing == []        # the sequential no-op: satisfied, and refused by the library all the same
        else:
            assert failing == [lay["recipient_rows"] + lay["levels"]]      # id bit L of the recipient is not zero


def test_the_sender_side_is_the_payment_circuits(params, blocks):
    """Up to and with the sender's root row the transfer circuit is build_payment's, witness for witness and row for row, but for
    the instance: the update blocks come after."""
    t = next(t for t in blocks(4)[1] if t["name"] == "meet at level 0")
    cs, _ = _build(params, 4, t)
    py, _ = W.payment_circuit(params, 4, t["message"], t["signature"], t["sender_leaf"], t["sender_path"], t["recipient_leaf"],
                              t["recipient_path"])
    lay, play = W.transfer_circuit_layout(params, 4), W.payment_circuit_layout(params, 4)
    assert cs.witness[:lay["sender_update"]] == py.witness[:play["recipient_bits"]]
    shift = {("i", 2): ("i", 3), ("i", 3): ("i", 4), ("i", 4): ("i", 5)}       # sender, recipient, amount move up by one
    moved = lambda lc: [(c, shift.get(v, v)) for c, v in lc]
    for k in range(3):
        assert [moved(lc) for lc in py.rows[k][:play["sender_root_row"] + 1]] == list(cs.rows[k][:lay["sender_root_row"] + 1])


def _shape(full, partial, alpha, height, salted):
    ni, nw, nc = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = load_library().swm_transfer_circuit_shape(full, partial, alpha, height, salted, ctypes.byref(ni), ctypes.byref(nw), ctypes.byref(nc))
    return rc, (ni.value, nw.value, nc.value)


@pytest.mark.parametrize("salt", [None, SALT])
def test_layout_equals_the_c_shape_at_every_height(params, salt):
    for height in range(2, 10):
        lay = W.transfer_circuit_layout(params, height, salt is not None)
        got = (lay["num_instance"], lay["num_witness"], lay["num_constraints"])
        assert _shape(8, 29, 17, height, 1 if salt else 0) == (0, got) and M.transfer_circuit_shape(params, height, salt is not None) == got
        s, s_rows, levels = M.schnorr_circuit_shape(10, salt is not None)[1:] + (height - 1,)
        m = 3 * levels + (2 + levels) * C
        assert got == (6, s + 769 + 4 * m - 4 * levels,
                       s_rows + 773 + 2 * (8 + 2 * C + levels * (2 + C) + 1) + 2 * (2 * C + levels * (1 + C) + 1))
    for height in (1, 10):
        with pytest.raises(ValueError):
            W.transfer_circuit_layout(params, height, salt is not None)
        assert _shape(8, 29, 17, height, 1 if salt else 0)[0] == -1
        with pytest.raises(M.MarlinError) as e:
            M.transfer_circuit_shape(params, height, salt is not None)
        assert e.value.code == -1


def test_builder_counts_with_a_salt(ref, params):
    t = TM.transfers(ref, 2, SALT)[1][-1]
    cs, public = _build(params, 2, t, salt=SALT)
    lay = W.transfer_circuit_layout(params, 2, True)
    assert t["applied"] and public == t["public"] and _failing_rows(cs) == []
    assert (len(cs.instance), len(cs.witness), cs.num_constraints) == (lay["num_instance"], lay["num_witness"], lay["num_constraints"])


def test_synthesizer_class_and_public_inputs(params, blocks):
    t = blocks(2)[1][-1]
    cs, public = _build(params, 2, t)
    assert W.transfer_public_inputs(public[0], public[1], t["message"]) == public
    again = M.MarlinInst._synthesize(W.TransferValidation(S.GENERATOR, None, params, 2, public[0], public[1], t["message"], t["signature"],
                                                          t["sender_leaf"], t["sender_path"], t["recipient_leaf"], t["recipient_path"]))
    assert again.witness == cs.witness and again.rows == cs.rows and again.instance == [1] + public


def test_builder_refusals(params, blocks):
    t = blocks(4)[1][0]
    args = [t["message"], t["signature"], t["sender_leaf"], t["sender_path"], t["recipient_leaf"], t["recipient_path"]]
    for k, bad in ((0, args[0][:9]), (2, args[2][:71]), (4, args[4] + b"\0"), (3, args[3][:2]), (5, args[5] + [0]),
                   (2, R.to_bytes(32, "little") + args[2][32:]), (2, bytes([args[2][0] ^ 1]) + args[2][1:])):
        changed = list(args)
        changed[k] = bad
        with pytest.raises(ValueError):
            W.transfer_circuit(params, 4, *changed)
    with pytest.raises(ValueError):
        W.transfer_public_inputs(0, 0, b"short")


def test_shape_call_refusals():
    lib = load_library()
    n = ctypes.c_size_t(0)
    for args in ((8, 29, 17, 1, 0), (8, 29, 17, 10, 0), (8, 29, 17, 31, 1), (7, 29, 17, 4, 0), (0, 29, 17, 4, 0), (8, 248, 17, 4, 0),
                 (8, 29, 1, 4, 0), (8, 29, 65536, 4, 0), (8, 29, 17, 1 << 62, 0), (1 << 63, 29, 17, 4, 0), (8, (1 << 64) - 8, 17, 4, 1)):
        assert _shape(*args)[0] == -1, args
    assert lib.swm_last_error(None).decode().startswith("transfer_circuit_shape")
    assert lib.swm_transfer_circuit_shape(8, 29, 17, 4, 0, None, ctypes.byref(n), ctypes.byref(n)) == -1
    assert lib.swm_transfer_circuit_shape(8, 29, 17, 4, 0, ctypes.byref(n), None, ctypes.byref(n)) == -1
    assert lib.swm_transfer_circuit_shape(8, 29, 17, 4, 0, ctypes.byref(n), ctypes.byref(n), None) == -1


def test_ffi_declares_the_new_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ffi = open(os.path.join(root, "swmarlin-sys", "src", "ffi.rs")).read()
    hdr = open(os.path.join(root, "include", "swmarlin.h")).read()
    names = ("swm_transfer_circuit_shape", "swm_transfer_circuit_create", "swm_transfer_circuit_destroy", "swm_transfer_witness_at",
             "swm_transfer_prove_at", "swm_transfer_prove_many_at")
    for name in names:
        assert "pub fn %s(" % name in ffi and "%s(" % name in hdr
        assert hasattr(load_library(), name)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shape_under_asan_ubsan(tmp_path):
    """csrc/host/transfer_shape.h — the counts and offsets the kernels write witnesses by — against the payment shape it is composed
    of, the formulas, and a cover of [0, num_witness) by its groups, in a stand-alone program (tests/native/transfer_shape_check.cpp)
    built with -fsanitize=address,undefined."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "transfer_shape_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(root, "simpleworks_amd", "csrc"), os.path.join(root, "tests", "native", "transfer_shape_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and ("asan" in out.stderr.lower() or "ubsan" in out.stderr.lower()) and "error:" not in out.stderr:
        pytest.skip("this g++ has no ASan / UBSan runtime")
    assert out.returncode == 0, out.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) >= 8 * 2 * 5 * 6 + 18

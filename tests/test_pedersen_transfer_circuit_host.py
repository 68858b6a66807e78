"""CPU tests of the transfer circuit over a Pedersen account tree: the model of a small ledger and a block of transfers applied in
order (tests/pedersen_transfer_model.py), the circuit's specification workloads.build_pedersen_transfer evaluated row by row in
Python integers at heights 2 and 3 — a valid transfer, a wrong new_root, a wrong R1, an overflow, an overdraft, a recipient sibling
taken from the old tree — and every refusal of a block at height 4, its sender side against build_pedersen_payment, its layout
against the built system, and its SHAPE and chunk plan as the library states them without a GPU
(swm_pedersen_transfer_circuit_shape, csrc/host/pedersen_transfer_shape.h, csrc/host/witness_chunks.h)."""
import ctypes
import os
import shutil
import subprocess

import pytest

import pedersen_payment_model as PM
import pedersen_transfer_model as TM
import schnorr_model as S
from simpleworks_amd import marlin as M, workloads as W
from simpleworks_amd._lib import load_library

R = W.R_MODULUS
SALT = bytes(range(32))
VALID = {2: "zero to one", 3: "meet at level 0"}


@pytest.fixture(scope="module")
def params():
    return W.MerkleParams()


@pytest.fixture(scope="module")
def blocks(params):
    seen = {}

    def get(height, salt=None):
        if (height, salt) not in seen:
            seen[(height, salt)] = TM.transfers(params, height, salt)
        return seen[(height, salt)]
    return get


def _failing_rows(cs, instance=None, witness=None):
    """The row evaluator: every row a z * b z == c z in Python integers; returns the indices of the rows that fail."""
    z = {("i", k): v for k, v in enumerate(cs.instance if instance is None else instance)}
    z.update({("w", k): v for k, v in enumerate(cs.witness if witness is None else witness)})

    def ev(lc):
        return sum(c * z[v] for c, v in lc) % R
    return [i for i, (a, b, c) in enumerate(zip(*cs.rows)) if ev(a) * ev(b) % R != ev(c)]


@pytest.mark.parametrize("height", [2, 3, 4])
def test_model_block(params, blocks, height):
    """The model against itself: the roots chain, a refused transfer publishes equal roots and the flag says why, every path
    leads where it should, and the tree after the block is the tree of the table after the block."""
    first, block, table, levels = blocks(height)
    n = 1 << (height - 1)
    assert TM.ledger(params, height)[0] == first and len(table) == n
    names = [t["name"] for t in block]
    assert "zero to one" in names and ("meet at level 0" in names) == (height > 2) and ("meet at the top level" in names) == (height > 3)
    root = TM.ledger(params, height)[1][-1][0]
    for t in block:
        assert t["public"][0] == root and t["applied"] == (t["wrong"] is None) == bool(t["flag"] & 16), t["name"]
        assert (t["public"][1] != root) == (t["applied"] and t["public"][4] > 0), t["name"]
        root = t["public"][1]
        want = {None: 31, "overflow": 15 - 4, "overdraft": 15 - 2, "signature": 15 - 1, "recipient": 15 - 8, "self": 15, "id": 15}[t["wrong"]]
        assert t["flag"] == want and t["status"] == {"self": 8, "id": 4}.get(t["wrong"], 0), t["name"]
        msg, mask = t["message"], n - 1
        s, r = msg[0] & mask, msg[1] & mask
        w = t["walks"]
        assert W.pedersen_payment_root(params, t["sender_leaf"], s, t["sender_path"]) == t["public"][0] == w["sender_old"][-1]
        assert W.pedersen_payment_root(params, t["debited_leaf"], s, t["sender_path"]) == t["r1"] == w["sender_new"][-1]
        # the recipient's leaf is in the INTERMEDIATE tree (a blank one too: the digest of 72 zero bytes is the blank digest, zero)
        assert W.pedersen_payment_root(params, t["recipient_leaf"], r, t["recipient_path"]) == t["r1"] == w["recipient_mid"][-1]
        assert W.pedersen_payment_root(params, t["credited_leaf"], r, t["recipient_path"]) == t["walked_new_root"] == w["recipient_new"][-1]
        assert all(len(v) == height for v in w.values())
        if s != r:
            # d, the top set bit of sender ^ recipient: the recipient's sibling at d is the sender's NEW digest of that level, the
            # siblings below are the old tree's, and above d the recipient walks the sender's new digests
            d = (s ^ r).bit_length() - 1
            assert t["recipient_path"][d] == w["sender_new"][d]
            assert t["recipient_path"][:d] == t["old_recipient_path"][:d] and t["recipient_path"][d + 1:] == t["sender_path"][d + 1:]
            assert w["recipient_mid"][d + 1:] == w["sender_new"][d + 1:]
        if t["applied"]:
            assert t["public"][1] == t["walked_new_root"]
            assert t["table"][s] == (t["debited_leaf"] if s != r else t["credited_leaf"]) and t["table"][r] == t["credited_leaf"]
    assert root == levels[-1][0] and block[-1]["table"] == table
    assert levels == PM.tree(params, height, {i: leaf for i, leaf in enumerate(table) if any(leaf)})
    assert PM.leaf_digest(params, bytes(72)) == 0


def test_model_chain_and_ring(params):
    """A dependent chain: an account credited and then debited by the next transfer, refusals in the middle."""
    first, block, table, levels = TM.transfers(params, 3, which=TM.CHAIN)
    assert [t["applied"] for t in block] == [True, True, False, False, True, True]
    balances = lambda tab: [int.from_bytes(leaf[64:], "little") for leaf in tab]
    assert balances(first)[1:3] == [1000, 5] and balances(table)[1:3] == [1000 - 600 + 100 + 405, 0]
    assert block[2]["public"][0] == block[2]["public"][1] == block[3]["public"][0] == block[3]["public"][1] == block[4]["public"][0]
    _, ring, table, levels = TM.transfers(params, 3, which=TM.RING * 2)
    assert all(t["applied"] for t in ring) and len(ring) == 6
    assert balances(table)[1:] == [1000 + 2 * (11 - 7), 5 + 2 * (7 - 9), (1 << 64) - 1 - 300 + 2 * (9 - 11)]
    assert levels == PM.tree(params, 3, {i: leaf for i, leaf in enumerate(table) if any(leaf)})


@pytest.mark.parametrize("height", [2, 3])
def test_rows_of_a_transfer_and_of_what_can_be_wrong_with_it(params, blocks, height):
    """A valid transfer: no failing row.  A wrong new_root: the last row only.  A wrong R1: its two rows only.  An overflow: the sum
    row only.  An overdraft: the diff row only.  A recipient sibling taken from the OLD tree: the recipient's R1 row only."""
    t = next(t for t in blocks(height)[1] if t["name"] == VALID[height])
    lay = W.pedersen_transfer_circuit_layout(height)
    cs, public = TM.build(params, height, t)
    assert public == t["public"] == W.pedersen_transfer_public_inputs(t["public"][0], t["public"][1], t["message"])
    assert cs.instance == [1] + public and cs.witness[lay["r1"]] == t["r1"]
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
    levels, mask = lay["levels"], (1 << lay["levels"]) - 1
    s, r = t["message"][0] & mask, t["message"][1] & mask
    balance, rbalance = int.from_bytes(t["sender_leaf"][64:], "little"), int.from_bytes(t["recipient_leaf"][64:], "little")
    bits = lambda v: [(v >> i) & 1 for i in range(64)]
    assert cs.witness[lay["balance"]:lay["diff"]] == bits(balance) and cs.witness[lay["diff"]:lay["sender"]] == bits(balance - amount)
    assert cs.witness[lay["sum"]:lay["recipient_update"]] == bits(rbalance + amount)
    assert cs.witness[lay["recipient_bits"]:lay["recipient"]] == [(byte >> i) & 1 for byte in t["recipient_leaf"] for i in range(8)]
    leaf_w, lvl_w, upd_w = W.PEDERSEN_PAYMENT_LEAF_WITNESSES, W.PEDERSEN_PAYMENT_LEVEL_WITNESSES, W.PEDERSEN_TRANSFER_LEVEL_WITNESSES
    assert lay["update"]["level0"] == leaf_w and lay["update"]["level_witnesses"] == upd_w == 3579 and lay["update"]["level_rows"] == 3587
    for base, index, sibs, curs in ((lay["sender"], s, t["sender_path"], t["walks"]["sender_old"]),
                                    (lay["recipient"], r, t["recipient_path"], t["walks"]["recipient_mid"])):
        # a membership section: the last X3 of the leaf hash is the leaf's digest; per level dir | sibling | left, the last X3 the parent
        assert cs.witness[base + leaf_w - 2] == curs[0]
        for l in range(levels):
            at = base + leaf_w + lvl_w * l
            assert cs.witness[at:at + 3] == [(index >> l) & 1, sibs[l], sibs[l] if (index >> l) & 1 else curs[l]]
            assert cs.witness[at + lvl_w - 2] == curs[l + 1]
    for base, index, sibs, curs in ((lay["sender_update"], s, t["sender_path"], t["walks"]["sender_new"]),
                                    (lay["recipient_update"], r, t["recipient_path"], t["walks"]["recipient_new"])):
        # an update section: per level left' alone, then the bits of left' and right'
        assert cs.witness[base + leaf_w - 2] == curs[0]
        for l in range(levels):
            at = base + leaf_w + upd_w * l
            left, right = (sibs[l], curs[l]) if (index >> l) & 1 else (curs[l], sibs[l])
            assert cs.witness[at] == left
            assert cs.witness[at + 1:at + 513] == [(left >> i) & 1 for i in range(256)] + [(right >> i) & 1 for i in range(256)]
            assert cs.witness[at + upd_w - 2] == curs[l + 1]
    # an overflow by one, an overdraft by one: the same transfer over a ledger whose balances say so
    which = [c for c in TM.TRANSFERS if c[0] == VALID[height]]
    over = TM.transfers(params, height, which=which, balances={t["message"][1]: (1 << 64) - amount})[1][0]
    assert over["flag"] == 15 - 4 and over["message"] == t["message"]
    assert _failing_rows(TM.build(params, height, over)[0]) == [lay["sum_pack_row"]]
    under = TM.transfers(params, height, which=which, balances={t["message"][0]: amount - 1})[1][0]
    assert under["flag"] == 15 - 2 and under["message"] == t["message"]
    assert _failing_rows(TM.build(params, height, under)[0]) == [lay["pack_row"]]
    # the paths meet at level 0: the old tree's path of the recipient differs from the intermediate tree's there alone
    differ = [l for l in range(levels) if t["old_recipient_path"][l] != t["recipient_path"][l]]
    assert differ == [0]
    stale, stale_public = TM.build(params, height, dict(t, recipient_path=t["old_recipient_path"]))
    assert _failing_rows(stale) == [lay["recipient_r1_row"]] and stale_public[1] != public[1]
    if height == 2:
        # the same through the builder's own overrides
        wrong, wrong_public = TM.build(params, height, t, new_root=(public[1] + 1) % R)
        assert wrong_public[1] == (public[1] + 1) % R and _failing_rows(wrong) == [lay["new_root_row"]]
        wrong, _ = TM.build(params, height, t, r1=(t["r1"] + 1) % R)
        assert _failing_rows(wrong) == [lay["sender_r1_row"], lay["recipient_r1_row"]]


def test_every_refusal_of_the_block_fails_its_own_rows(params, blocks):
    lay = W.pedersen_transfer_circuit_layout(4)
    s_rows = lay["schnorr"]["num_constraints"]
    seen = set()
    for t in blocks(4)[1]:
        if t["wrong"] in (None, "overflow", "overdraft"):
            continue        # the test above
        seen.add(t["wrong"])
        failing = _failing_rows(TM.build(params, 4, t)[0])
        if t["wrong"] == "signature":
            assert failing and set(failing) <= set(range(s_rows - 8, s_rows))
        elif t["wrong"] in ("recipient", "self"):
            # a blank leaf's digest is the hash of 72 zero bytes (zero), so crediting a blank leaf is a satisfied system, and a transfer
            # to oneself the sequential no-op: both are refused by the entry points' decision, not by a row
            assert failing == []
        else:
            assert failing == [lay["recipient_rows"] + lay["section_rows"] - 9 + lay["levels"]]      # id bit L of the recipient is not zero
    assert seen == {"signature", "recipient", "self", "id"}


def test_the_sender_side_is_the_pedersen_payment_circuits(params, blocks):
    """Up to and with the sender's root row the circuit is build_pedersen_payment's, witness for witness and row for row, but for the
    instance: the update sections come after."""
    t = next(t for t in blocks(3)[1] if t["name"] == "meet at level 0")
    cs, _ = TM.build(params, 3, t)
    pp, _ = W.pedersen_payment_circuit(params, 3, t["message"], t["signature"], t["sender_leaf"], t["sender_path"], t["recipient_leaf"],
                                       t["recipient_path"])
    lay, play = W.pedersen_transfer_circuit_layout(3), W.pedersen_payment_circuit_layout(3)
    assert lay["sender_update"] == play["recipient_bits"] and lay["sender_root_row"] == play["sender_root_row"]
    assert cs.witness[:lay["sender_update"]] == pp.witness[:play["recipient_bits"]]
    shift = {("i", 2): ("i", 3), ("i", 3): ("i", 4), ("i", 4): ("i", 5)}       # sender, recipient, amount move up by one
    moved = lambda lc: [(c, shift.get(v, v)) for c, v in lc]
    for k in range(3):
        assert [moved(lc) for lc in pp.rows[k][:play["sender_root_row"] + 1]] == list(cs.rows[k][:lay["sender_root_row"] + 1])


class _CountingSystem:
    """The builder's vocabulary, keeping the values and counting the rows."""

    def __init__(self):
        self.instance, self.witness, self.num_constraints = [1], [], 0

    @staticmethod
    def one():
        return ("i", 0)

    def new_input_variable(self, value):
        self.instance.append(int(value) % R)
        return ("i", len(self.instance) - 1)

    def new_witness_variable(self, value):
        self.witness.append(int(value) % R)
        return ("w", len(self.witness) - 1)

    def enforce_constraint(self, a, b, c):
        self.num_constraints += 1


def _lib_shape(height, salted):
    ni, nw, nc = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = load_library().swm_pedersen_transfer_circuit_shape(height, salted, ctypes.byref(ni), ctypes.byref(nw), ctypes.byref(nc))
    return rc, (ni.value, nw.value, nc.value)


def test_layout_equals_the_c_shape_at_every_height_and_the_built_counts(params):
    for salted in (False, True):
        for height in range(2, 10):
            lay = W.pedersen_transfer_circuit_layout(height, salted)
            got = (lay["num_instance"], lay["num_witness"], lay["num_constraints"])
            assert _lib_shape(height, 1 if salted else 0) == (0, got) and M.pedersen_transfer_circuit_shape(height, salted) == got
            s, s_rows, levels = M.schnorr_circuit_shape(10, salted)[1:] + (height - 1,)
            m, u = 3450 + 3581 * levels, 3450 + 3579 * levels
            assert lay["membership_witnesses"] == m and lay["update_witnesses"] == u
            assert got == (6, s + 769 + 2 * m + 2 * u, s_rows + 773 + 2 * (3459 + 3588 * levels) + 2 * (3451 + 3587 * levels))
    # the built system's counts: the shape does not depend on the values, one transfer from index 0 to index 1 with zero siblings and
    # the roots given serves every height
    leaves = {0: PM.leaf(TM.secret(0), 50), 1: PM.leaf(TM.secret(1), 1000)}
    for height, salt in [(h, None) for h in range(2, 10)] + [(2, SALT), (9, SALT)]:
        msg = PM.message(0, 1, 1)
        sig = S.sign(S.GENERATOR, salt, TM.secret(0), S.keygen(S.GENERATOR, TM.secret(0)), 987654321, msg)
        cs = _CountingSystem()
        W.build_pedersen_transfer(cs, S.GENERATOR, salt, params, height, msg, sig, leaves[0], [0] * (height - 1), leaves[1],
                                  [0] * (height - 1), old_root=0, new_root=0, r1=0)
        lay = W.pedersen_transfer_circuit_layout(height, salt is not None)
        assert (len(cs.instance), len(cs.witness), cs.num_constraints) == (lay["num_instance"], lay["num_witness"], lay["num_constraints"])
        if (height, salt) == (9, None):
            assert (len(cs.instance), len(cs.witness), cs.num_constraints) == (6, 200274, 201521)      # the worked numbers: |H| = 2^18


def test_builder_counts_with_a_salt(params):
    t = TM.transfers(params, 2, SALT)[1][-1]
    cs, public = TM.build(params, 2, t, salt=SALT)
    lay = W.pedersen_transfer_circuit_layout(2, True)
    assert t["applied"] and public == t["public"] and _failing_rows(cs) == []
    assert (len(cs.instance), len(cs.witness), cs.num_constraints) == (lay["num_instance"], lay["num_witness"], lay["num_constraints"])


def test_synthesizer_class(params, blocks):
    t = blocks(2)[1][-1]
    cs, public = TM.build(params, 2, t)
    again = M.MarlinInst._synthesize(W.PedersenTransferValidation(S.GENERATOR, None, params, 2, public[0], public[1], t["message"],
                                                                  t["signature"], t["sender_leaf"], t["sender_path"], t["recipient_leaf"],
                                                                  t["recipient_path"]))
    assert again.witness == cs.witness and again.rows == cs.rows and again.instance == [1] + public


def test_shape_call_and_builder_refusals(params, blocks):
    lib = load_library()
    n = ctypes.c_size_t(0)
    for height in (0, 1, 10, 1 << 62):
        assert _lib_shape(height, 0)[0] == -1 and _lib_shape(height, 1)[0] == -1, height
    assert lib.swm_last_error(None).decode().startswith("pedersen_transfer_circuit_shape")
    assert lib.swm_pedersen_transfer_circuit_shape(4, 0, None, ctypes.byref(n), ctypes.byref(n)) == -1
    assert lib.swm_pedersen_transfer_circuit_shape(4, 0, ctypes.byref(n), None, ctypes.byref(n)) == -1
    assert lib.swm_pedersen_transfer_circuit_shape(4, 0, ctypes.byref(n), ctypes.byref(n), None) == -1
    with pytest.raises(M.MarlinError) as e:
        M.pedersen_transfer_circuit_shape(10)
    assert e.value.code == -1
    for height in (1, 10):
        with pytest.raises(ValueError):
            W.pedersen_transfer_circuit_layout(height)
    t = blocks(3)[1][0]
    for changed in ({"message": t["message"][:9]}, {"sender_leaf": t["sender_leaf"][:71]}, {"recipient_leaf": t["recipient_leaf"] + b"\0"},
                    {"sender_path": t["sender_path"][:1]}, {"recipient_path": t["recipient_path"] + [0]},
                    {"sender_leaf": R.to_bytes(32, "little") + t["sender_leaf"][32:]}):
        with pytest.raises(ValueError):
            TM.build(params, 3, dict(t, **changed))
    for height in (1, 10):
        with pytest.raises(ValueError):
            TM.build(params, height, dict(t, sender_path=[0] * (height - 1), recipient_path=[0] * (height - 1)))
    with pytest.raises(ValueError):       # a leaf CRH that does not hold 72 bytes
        TM.build(W.MerkleParams(generators=(params.leaf_gens[:143], params.inner_gens)), 3, t)
    with pytest.raises(ValueError):       # a two-to-one CRH that does not hold two digests
        TM.build(W.MerkleParams(generators=(params.leaf_gens, params.inner_gens[:127])), 3, t)
    with pytest.raises(ValueError):
        W.pedersen_transfer_public_inputs(0, 0, b"short")


def test_header_and_ffi_declare_the_new_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "swmarlin.h")).read()
    ffi = open(os.path.join(root, "swmarlin-sys", "src", "ffi.rs")).read()
    for name in ("swm_pedersen_transfer_circuit_shape", "swm_pedersen_transfer_circuit_create", "swm_pedersen_transfer_circuit_destroy",
                 "swm_pedersen_transfer_witness_at", "swm_pedersen_transfer_prove_at", "swm_pedersen_transfer_prove_many_at"):
        assert "%s(" % name in hdr and "pub fn %s(" % name in ffi
        assert hasattr(load_library(), name)


def _plan(item_bytes, count, cap_bytes):
    per = max(1, cap_bytes // item_bytes)
    return ["%d:%d" % (base, min(per, count - base)) for base in range(0, count, per)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shape_header_and_chunk_planner_under_asan_ubsan(tmp_path):
    """csrc/host/pedersen_transfer_shape.h — counts, offsets, named rows — and the chunk planner of csrc/host/witness_chunks.h,
    which every circuit unit cuts a batch by, printed by a stand-alone program
    (tests/native/pedersen_transfer_shape_check.cpp) built with -fsanitize=address,undefined: every shape line against the layout,
    every plan line against the plan computed here (small caps: below one transfer, exactly k transfers, one byte short of k)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "pedersen_transfer_shape_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(root, "simpleworks_amd", "csrc"), os.path.join(root, "tests", "native", "pedersen_transfer_shape_check.cpp"),
           "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and ("asan" in out.stderr.lower() or "ubsan" in out.stderr.lower()) and "error:" not in out.stderr:
        pytest.skip("this g++ has no ASan / UBSan runtime")
    assert out.returncode == 0, out.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().split("\n")
    shapes = [l.split() for l in lines if l.startswith("shape ")]
    plans = [l.split() for l in lines if l.startswith("plan ")]
    assert lines[-1] == "ok %d" % (len(shapes) + 4 + len(plans) + 1) and len(shapes) == 16 and len(plans) == 8 * 8 + 3
    seen = set()
    for f in shapes:
        height, salted = int(f[1]), f[2] == "1"
        lay = W.pedersen_transfer_circuit_layout(height, salted)
        want = [lay[k] for k in ("num_instance", "num_witness", "num_constraints", "balance", "diff", "sender", "sender_update", "r1",
                                 "recipient_bits", "recipient", "sum", "recipient_update", "membership_witnesses", "update_witnesses",
                                 "section_rows", "update_rows", "pack_row", "sender_root_row", "sender_r1_row", "recipient_r1_row",
                                 "sum_pack_row", "new_root_row")]
        assert [int(v) for v in f[3:]] == want, f
        seen.add((height, salted))
    assert seen == {(h, s) for h in range(2, 10) for s in (False, True)}
    item = 32 * W.pedersen_transfer_circuit_layout(3)["num_witness"]
    for f in plans:
        assert f[4:] == _plan(int(f[1]), int(f[2]), int(f[3])), f
    by_args = {(int(f[1]), int(f[2]), int(f[3])): f[4:] for f in plans}
    assert by_args[item, 7, 3 * item + 5] == ["0:3", "3:3", "6:1"] and by_args[item, 3, item - 1] == ["0:1", "1:1", "2:1"]
    assert by_args[item, 65, 8 * item] == ["%d:8" % (8 * k) for k in range(8)] + ["64:1"] and by_args[item, 0, item] == []
    # the library's own cap at height 9: floor(1 GiB / (32 x 200274)) = 167 transfers per chunk
    big = by_args[32 * 200274, 1000, 1 << 30]
    assert big[0] == "0:167" and big[-1] == "835:165" and len(big) == 6
    # ... which is written once, in witness_chunks.h
    assert [l for l in lines if l.startswith("stage ")] == ["stage %d" % (1 << 30)]

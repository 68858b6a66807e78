"""CPU tests of the payment circuit over a Pedersen account tree: the circuit's specification workloads.build_pedersen_payment
evaluated row by row in Python integers at heights 2 and 4 — a valid payment, a bad signature, an overdraft, a sender's and a
recipient's leaf that are not the tree's — its layout against the built system for every height, its SHAPE as the library states it
without a GPU (swm_pedersen_payment_circuit_shape, csrc/host/pedersen_payment_shape.h), and build_merkle_membership, whose level the
new builder shares, held to the system it built before."""
import ctypes
import hashlib
import os
import shutil
import subprocess

import pytest

import pedersen_payment_model as PM
import schnorr_model as S
from simpleworks_amd import marlin as M, workloads as W
from simpleworks_amd._lib import load_library

R = W.R_MODULUS
SALT = bytes(range(32))
SECRETS = {0: 1234567, 1: 1234584, 7: 1234601}     # leaf index -> secret key; height 2 holds the first two
BALANCES = {0: 1000, 1: 5, 7: (1 << 64) - 1}


@pytest.fixture(scope="module")
def params():
    return W.MerkleParams()


@pytest.fixture(scope="module")
def world(params):
    """height -> (leaves, levels, the valid payment from index 0 to the last leaf)."""
    seen = {}

    def get(height):
        if height not in seen:
            last = (1 << (height - 1)) - 1
            leaves = {i: PM.leaf(SECRETS[i], BALANCES[i]) for i in (0, last)}
            levels = PM.tree(params, height, leaves)
            seen[height] = (leaves, levels, PM.payment(levels, leaves, SECRETS[0], 0, last, 300))
        return seen[height]
    return get


def _failing_rows(cs):
    """The row evaluator: every row a z * b z == c z in Python integers; returns the indices of the rows that fail."""
    z = {("i", k): v for k, v in enumerate(cs.instance)}
    z.update({("w", k): v for k, v in enumerate(cs.witness)})

    def ev(lc):
        return sum(c * z[v] for c, v in lc) % R
    return [i for i, (a, b, c) in enumerate(zip(*cs.rows)) if ev(a) * ev(b) % R != ev(c)]


def _select_or_root_rows(lay, base):
    """The select row of every level of the section whose rows start at `base`, and its root row."""
    levels_at = base + W.PEDERSEN_PAYMENT_LEAF_WITNESSES
    return {levels_at + W.PEDERSEN_PAYMENT_LEVEL_ROWS * l + 1 for l in range(lay["levels"])} | {base + lay["section_rows"] - 1}


@pytest.mark.parametrize("height", [2, 4])
def test_a_valid_payment_satisfies_every_row(params, world, height):
    leaves, levels, p = world(height)
    cs, public = PM.build(params, height, p)
    lay = W.pedersen_payment_circuit_layout(height)
    assert public == p["public"] == W.pedersen_payment_public_inputs(levels[-1][0], p["message"]) and cs.instance == [1] + public
    assert (len(cs.instance), len(cs.witness), cs.num_constraints) == (lay["num_instance"], lay["num_witness"], lay["num_constraints"])
    assert _failing_rows(cs) == []
    # the witness groups sit where the layout says
    w, last = cs.witness, (1 << (height - 1)) - 1
    bits = lambda data: [(byte >> i) & 1 for byte in data for i in range(8)]
    assert w[lay["balance"]:lay["diff"]] == [(1000 >> i) & 1 for i in range(64)]
    assert w[lay["diff"]:lay["sender"]] == [(700 >> i) & 1 for i in range(64)]
    assert w[lay["recipient_bits"]:lay["recipient"]] == bits(p["recipient_leaf"])
    dec = lay["schnorr"]["dec"]
    assert w[dec:dec + 512] + w[lay["balance"]:lay["diff"]] == bits(p["sender_leaf"])
    for base, index, sibs in ((lay["sender"], 0, p["sender_path"]), (lay["recipient"], last, p["recipient_path"])):
        # the last X3 of the leaf hash is the leaf's digest; per level dir | sibling | left, the last X3 the parent
        assert w[base + W.PEDERSEN_PAYMENT_LEAF_WITNESSES - 2] == levels[0][index]
        for l, s in enumerate(sibs):
            at = base + W.PEDERSEN_PAYMENT_LEAF_WITNESSES + W.PEDERSEN_PAYMENT_LEVEL_WITNESSES * l
            assert w[at:at + 3] == [(index >> l) & 1, s, s if (index >> l) & 1 else levels[l][index >> l]]
            assert w[at + W.PEDERSEN_PAYMENT_LEVEL_WITNESSES - 2] == levels[l + 1][index >> (l + 1)]
    # the synthesizer class emits the same system
    again = M.MarlinInst._synthesize(W.PedersenPaymentValidation(S.GENERATOR, None, params, height, public[0], p["message"], p["signature"],
                                                                 p["sender_leaf"], p["sender_path"], p["recipient_leaf"], p["recipient_path"]))
    assert again.witness == cs.witness and again.rows == cs.rows and again.instance == [1] + public


@pytest.mark.parametrize("height", [2, 4])
def test_each_false_statement_fails_its_own_rows_only(params, world, height):
    leaves, levels, p = world(height)
    lay = W.pedersen_payment_circuit_layout(height)
    last, root = (1 << (height - 1)) - 1, levels[-1][0]
    s_rows = lay["schnorr"]["num_constraints"]
    # a bad signature: comparison rows of the Schnorr block only
    bad = PM.payment(levels, leaves, SECRETS[0], 0, last, 300, flip_signature=True)
    assert bad["flag"] == 2
    failing = _failing_rows(PM.build(params, height, bad)[0])
    assert failing and set(failing) <= set(range(s_rows - 8, s_rows))
    # amount = balance + 1: the packing row only
    over = PM.payment(levels, leaves, SECRETS[0], 0, last, 1001)
    assert over["flag"] == 1 and _failing_rows(PM.build(params, height, over)[0]) == [lay["pack_row"]]
    # a sender leaf with one balance bit flipped against the tree: a select or root row of the sender's section only
    flipped = p["sender_leaf"][:64] + bytes([p["sender_leaf"][64] ^ 0x10]) + p["sender_leaf"][65:]
    failing = _failing_rows(PM.build(params, height, p, root=root, sender_leaf=flipped)[0])
    assert failing and set(failing) <= _select_or_root_rows(lay, lay["sender_rows"])
    # the same for the recipient
    flipped = p["recipient_leaf"][:64] + bytes([p["recipient_leaf"][64] ^ 0x10]) + p["recipient_leaf"][65:]
    failing = _failing_rows(PM.build(params, height, p, root=root, recipient_leaf=flipped)[0])
    assert failing and set(failing) <= _select_or_root_rows(lay, lay["recipient_rows"])
    # another public root: both root rows
    failing = _failing_rows(PM.build(params, height, p, root=(root + 1) % R)[0])
    assert failing == [lay["sender_root_row"], lay["recipient_root_row"]] and failing[1] == lay["num_constraints"] - 1


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
    rc = load_library().swm_pedersen_payment_circuit_shape(height, salted, ctypes.byref(ni), ctypes.byref(nw), ctypes.byref(nc))
    return rc, (ni.value, nw.value, nc.value)


@pytest.fixture(scope="module")
def built_counts(params):
    """(height, salted) -> the counts of the built system, heights 2 .. 9.  The shape does not depend on the values: one payment of
    an account to itself at index 0 with zero siblings and the public root given serves every height."""
    out = {}
    leaves = {0: PM.leaf(SECRETS[0], BALANCES[0])}
    for salt in (None, SALT):
        for height in range(2, 10):
            p = PM.payment([[0, 0]] * (height - 1) + [[0]], leaves, SECRETS[0], 0, 0, 1, salt=salt)
            cs, _ = PM.build(params, height, p, salt=salt, root=0, cs=_CountingSystem(), sender_path=[0] * (height - 1),
                             recipient_path=[0] * (height - 1))
            out[height, salt is not None] = (len(cs.instance), len(cs.witness), cs.num_constraints)
    return out


def test_layout_library_and_formulas_equal_the_built_counts(built_counts):
    for (height, salted), got in built_counts.items():
        lay = W.pedersen_payment_circuit_layout(height, salted)
        assert got == (lay["num_instance"], lay["num_witness"], lay["num_constraints"]), (height, salted)
        assert _lib_shape(height, 1 if salted else 0) == (0, got) and M.pedersen_payment_circuit_shape(height, salted) == got
        s, s_rows, levels = M.schnorr_circuit_shape(10, salted)[1:] + (height - 1,)
        assert got == (5, s + 704 + 2 * (3450 + 3581 * levels), s_rows + 708 + 2 * (3459 + 3588 * levels))
    assert built_counts[9, False] == (5, 136045, 137162)      # the worked numbers: |H| = 2^18


def test_shape_call_and_builder_refusals(params, world):
    lib = load_library()
    n = ctypes.c_size_t(0)
    for height in (0, 1, 10, 1 << 62):
        assert _lib_shape(height, 0)[0] == -1, height
    assert lib.swm_last_error(None).decode().startswith("pedersen_payment_circuit_shape")
    assert lib.swm_pedersen_payment_circuit_shape(4, 0, None, ctypes.byref(n), ctypes.byref(n)) == -1
    assert lib.swm_pedersen_payment_circuit_shape(4, 0, ctypes.byref(n), None, ctypes.byref(n)) == -1
    assert lib.swm_pedersen_payment_circuit_shape(4, 0, ctypes.byref(n), ctypes.byref(n), None) == -1
    with pytest.raises(M.MarlinError) as e:
        M.pedersen_payment_circuit_shape(10)
    assert e.value.code == -1
    for height in (1, 10):
        with pytest.raises(ValueError):
            W.pedersen_payment_circuit_layout(height)
    p = world(4)[2]
    for changed in ({"message": p["message"][:9]}, {"sender_leaf": p["sender_leaf"][:71]}, {"recipient_leaf": p["recipient_leaf"] + b"\0"},
                    {"sender_path": p["sender_path"][:2]}, {"message": bytes([0, 8]) + p["message"][2:]},
                    {"sender_leaf": R.to_bytes(32, "little") + p["sender_leaf"][32:]}):
        with pytest.raises(ValueError):
            PM.build(params, 4, p, **changed)
    with pytest.raises(ValueError):       # a leaf CRH that does not hold 72 bytes
        PM.build(W.MerkleParams(generators=(params.leaf_gens[:143], params.inner_gens)), 4, p)


def test_header_and_ffi_declare_the_new_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "swmarlin.h")).read()
    ffi = open(os.path.join(root, "swmarlin-sys", "src", "ffi.rs")).read()
    for name in ("swm_pedersen_payment_circuit_shape", "swm_pedersen_payment_circuit_create", "swm_pedersen_payment_circuit_destroy",
                 "swm_pedersen_payment_witness", "swm_pedersen_payment_witness_at", "swm_pedersen_payment_witness_dev",
                 "swm_pedersen_payment_prove_at", "swm_pedersen_payment_prove_many_at"):
        assert "%s(" % name in hdr and "pub fn %s(" % name in ffi
        assert hasattr(load_library(), name)


class _FlatParams:
    """MerkleParams with every generator the same point, as tests/test_merkle_witness_host.py builds the membership circuit."""
    digest_bits = 256

    def __init__(self):
        g = W.ED_GENERATOR
        row = [g, W.ed_add(g, g)]
        row.append(W.ed_add(row[1], row[1]))
        row.append(W.ed_add(row[2], row[2]))
        self.leaf_gens = [row] * 2
        self.inner_gens = [row] * 128

    def root_from_path(self, leaf_u8, leaf_index, siblings):
        return 0


# (leaf, index, siblings, byte operations) -> counts and the SHA-256 of repr((instance, witness, rows)) as build_merkle_membership
# emitted them before its level became _mw_level; the first case is tests/test_merkle_witness_host.py's
MEMBERSHIP_BEFORE = [((0xA7, 1, [5], 16), (10, 3751, 3815), "2c268eba35c3ecbdd2b0938c35d70a6eb182a494620594dfc42ef4919983c1e7"),
                     ((0x3C, 2, [7, 11], 0), (10, 7204, 7227), "35d291f10660f3e03d711eeba43c9ae3aa929ba8590bd7651643446bd996eb33")]


@pytest.mark.parametrize("case,counts,digest", MEMBERSHIP_BEFORE)
def test_build_merkle_membership_emits_the_system_it_did(case, counts, digest):
    cs = M.ConstraintSystem()
    W.build_merkle_membership(cs, _FlatParams(), case[0], case[1], case[2], gadget_byte_ops=case[3])
    assert (len(cs.instance), len(cs.witness), cs.num_constraints) == counts
    assert hashlib.sha256(repr((cs.instance, cs.witness, cs.rows)).encode()).hexdigest() == digest


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shape_header_under_asan_ubsan_equals_the_layout(tmp_path):
    """csrc/host/pedersen_payment_shape.h — the counts and offsets the kernels write witnesses by — printed by a stand-alone program
    (tests/native/pedersen_payment_shape_check.cpp) built with -fsanitize=address,undefined, line for line against the layout."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "pedersen_payment_shape_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(root, "simpleworks_amd", "csrc"), os.path.join(root, "tests", "native", "pedersen_payment_shape_check.cpp"),
           "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and ("asan" in out.stderr.lower() or "ubsan" in out.stderr.lower()) and "error:" not in out.stderr:
        pytest.skip("this g++ has no ASan / UBSan runtime")
    assert out.returncode == 0, out.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.split("\n")
    assert lines[16] == "ok 20"
    seen = set()
    for line in lines[:16]:
        f = line.split()
        assert f[0] == "shape"
        height, salted = int(f[1]), f[2] == "1"
        lay = W.pedersen_payment_circuit_layout(height, salted)
        want = [lay[k] for k in ("num_instance", "num_witness", "num_constraints", "balance", "diff", "sender", "recipient_bits", "recipient",
                                 "membership_witnesses", "section_rows")]
        assert [int(v) for v in f[3:]] == want, line
        seen.add((height, salted))
    assert seen == {(h, s) for h in range(2, 10) for s in (False, True)}

"""CPU tests of integer programs: the circuit a tape denotes (workloads.build_program), evaluated row by row in Python integers —
every op at every width against the semantics of the reference's gadgets in plain integers (tests/program_model.py, recorded in
tests/golden/program.json), on honest and on tampered assignments — and its SHAPE and validator as the library states them without a
GPU (swm_program_circuit_shape, csrc/host/program_shape.h): the GPU witness synthesis (csrc/program_witness.hip) addresses its trace
and its output by that plan.  (The limit of 2^20 witnesses per item cannot be reached within 4096 instructions — the widest op, DIV
on U64, has 192 — so it is stated and checked by the validator but has no case here.)"""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import program_model as PM
from simpleworks_amd import marlin as M, workloads as W
from simpleworks_amd._lib import load_library
from simpleworks_amd.program import BOOL, U8, U16, U32, U64, U128, Program

R = W.R_MODULUS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "program.json")) as f:
    GOLDEN = json.load(f)
UNITS = PM.unit_programs()
# per op: (witnesses, rows) as (multiple of W, constant) — the formulas of the issue's layout, written out here on their own
FORMULA = {"and": ((1, 0), (1, 0)), "or": ((1, 0), (1, 0)), "xor": ((1, 0), (1, 0)), "nand": ((1, 0), (1, 0)), "nor": ((1, 0), (1, 0)),
           "not": ((0, 0), (0, 0)), "add": ((1, 1), (1, 2)), "sub": ((1, 0), (1, 1)), "mul": ((2, 0), (2, 1)), "div": ((3, 0), (3, 2)),
           "shift_left": ((0, 0), (0, 0)), "shift_right": ((0, 0), (0, 0)), "rotate_left": ((0, 0), (0, 0)),
           "rotate_right": ((0, 0), (0, 0)), "gt": ((1, 1), (1, 2)), "gte": ((1, 1), (1, 2)), "lt": ((1, 1), (1, 2)),
           "lte": ((1, 1), (1, 2)), "eq": ((0, 2), (0, 2)), "select": ((1, 0), (1, 0))}
WITNESS_OPS = [op for op, (w, _) in FORMULA.items() if w != (0, 0)]


def _failing_rows(cs, instance=None, witness=None):
    """The row evaluator: every row a z * b z == c z in Python integers; returns the indices of the rows that fail."""
    z = {("i", k): v for k, v in enumerate(cs.instance if instance is None else instance)}
    z.update({("w", k): v for k, v in enumerate(cs.witness if witness is None else witness)})

    def ev(lc):
        return sum(c * z[v] for c, v in lc) % R
    return [i for i, (a, b, c) in enumerate(zip(*cs.rows)) if ev(a) * ev(b) % R != ev(c)]


def _shape(tape):
    lib = load_library()
    buf = (ctypes.c_uint8 * max(1, len(tape))).from_buffer_copy(bytes(tape).ljust(1, b"\0"))
    ni, nw, nc = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = lib.swm_program_circuit_shape(buf, len(tape), ctypes.byref(ni), ctypes.byref(nw), ctypes.byref(nc))
    return rc, (ni.value, nw.value, nc.value)


def _unit_counts(op, t):
    Wd = PM.width(t)
    (wk, wc), (rk, rc) = FORMULA[op]
    inputs = 2 * Wd + (1 if op == "select" else 0)
    out = 1 if op in PM.COMPARISONS + ("eq",) else Wd
    return 1 + out, inputs + wk * Wd + wc, inputs + rk * Wd + rc + out


def _op_at(op):
    """The index of a unit program's op instruction: after its two (select: three) inputs."""
    return 3 if op == "select" else 2


# ------------------------------------------------------------------------------------------------------------- unit programs
@pytest.mark.parametrize("name", sorted(UNITS))
def test_unit_program(name):
    """Every op at every width: the tape is the fixture's, the counts are the formulas', the library's and the layout's; over the
    extremal pairs and eight random ones the output is the plain-integer one and every row holds exactly when the status is 0."""
    P, op, t, positions = UNITS[name]
    gold = GOLDEN["unit"][name]
    tape = P.tape()
    assert tape.hex() == gold["tape"]
    want = _unit_counts(op, t)
    lay = W.program_circuit_layout(tape)
    assert tuple(gold["counts"]) == want == (lay["num_instance"], lay["num_witness"], lay["num_constraints"])
    assert _shape(tape) == (0, want) and M.program_circuit_shape(tape) == want
    cases = PM.unit_cases(op, t, positions)
    assert PM.hexes(v for _, v, _ in cases) == gold["outputs"] and "".join(str(s) for _, _, s in cases) == gold["status"]
    assert PM.hexes(v for private, _, _ in cases for v in private[:2]) == GOLDEN["operands"][str(PM.width(t))]
    for private, value, status in cases:
        cs = M.ConstraintSystem()
        public, outputs, got_status = W.build_program(cs, tape, [], private)
        assert outputs == [value] and got_status == status, (private, outputs, value)
        assert (len(cs.instance), len(cs.witness), cs.num_constraints) == want
        assert public == cs.instance[1:] == W.program_public_inputs(tape, [], [value])
        assert (_failing_rows(cs) == []) == (status == 0), private
        assert lay["witness_at"][_op_at(op)] == 2 * PM.width(t) + (1 if op == "select" else 0)


# ---------------------------------------------------------------------------------------------------------- soundness probes
def _honest(op, t, a, b, c=1, positions=0):
    P, _, _, _ = UNITS["%s_%s" % (op, W.PROGRAM_TYPES[t].lower())]
    tape = P.tape()
    cs = M.ConstraintSystem()
    W.build_program(cs, tape, [], [a, b, c] if op == "select" else [a, b])
    assert _failing_rows(cs) == []
    return cs, W.program_circuit_layout(tape)


@pytest.mark.parametrize("t", (U8, U64, U128))
@pytest.mark.parametrize("op", WITNESS_OPS)
def test_a_flipped_result_bit_or_a_two_fails_a_row(op, t):
    """One wrong claim, every other witness honest: each witness of the op flipped (a bit) or replaced (the EQ inverse), and a
    non-boolean 2 in its place, fails a row."""
    if t == U128 and op in ("mul", "div"):
        return
    a, b = (200, 7) if t == U8 else ((1 << 63) + 12345, 991) if t == U64 else ((1 << 127) + 5, (1 << 100) + 3)
    cs, lay = _honest(op, t, a, b)
    first = lay["witness_at"][_op_at(op)]
    assert first + FORMULA[op][0][0] * PM.width(t) + FORMULA[op][0][1] == len(cs.witness)
    for k in range(first, len(cs.witness)):
        for wrong in ((1 - cs.witness[k]) % R if cs.witness[k] in (0, 1) else (cs.witness[k] + 1) % R, 2):
            witness = list(cs.witness)
            witness[k] = wrong
            assert _failing_rows(cs, witness=witness), (op, k, wrong)


@pytest.mark.parametrize("t", PM.UNSIGNED)
@pytest.mark.parametrize("op", PM.COMPARISONS)
def test_the_flipped_answer_of_a_comparison_fails(op, t):
    Wd = PM.width(t)
    for a, b in ((5, 5), (5, 6), ((1 << Wd) - 1, 0), (0, (1 << Wd) - 1)):
        cs, lay = _honest(op, t, a, b)
        k = lay["witness_at"][2] + Wd   # the top bit of the sum
        witness = list(cs.witness)
        witness[k] ^= 1
        assert _failing_rows(cs, witness=witness)
        # and the published answer alone
        instance = list(cs.instance)
        instance[1] ^= 1
        assert _failing_rows(cs, instance=instance) == [cs.num_constraints - 1]


@pytest.mark.parametrize("t", (U8, U16, U32, U64))
def test_quotient_plus_one_with_remainder_minus_divisor_fails(t):
    Wd = PM.width(t)
    mask = (1 << Wd) - 1
    a, b = mask - 3, 7
    cs, lay = _honest("div", t, a, b)
    at = lay["witness_at"][2]
    q, rem = a // b + 1, (a % b - b) & mask
    witness = list(cs.witness)
    witness[at:at + Wd] = [(q >> i) & 1 for i in range(Wd)]
    witness[at + Wd:at + 2 * Wd] = [(rem >> i) & 1 for i in range(Wd)]
    assert _failing_rows(cs, witness=witness)
    # with the third decomposition adjusted as well the product row still fails: rem - b wraps in 2^W, not in the field
    tt = (b - 1 - rem) & mask
    witness[at + 2 * Wd:at + 3 * Wd] = [(tt >> i) & 1 for i in range(Wd)]
    assert _failing_rows(cs, witness=witness)


@pytest.mark.parametrize("name", ("add_u8", "xor_u128", "eq_u64", "select_bool", "rotate_left_u16_1", "not_u32"))
def test_a_wrong_public_output_fails_its_output_row(name):
    P, op, t, positions = UNITS[name]
    cs = M.ConstraintSystem()
    W.build_program(cs, P.tape(), [], [3, 1, 1] if op == "select" else [3, 1])
    outs = len(cs.instance) - 1
    for k in range(outs):
        instance = list(cs.instance)
        instance[1 + k] ^= 1
        assert _failing_rows(cs, instance=instance) == [cs.num_constraints - outs + k]


def test_gt_and_div_decompositions_are_unique_at_u8():
    """On the packed integers, over all 256 x 256 operand pairs: the rows of GT have one solution and its top bit is a > b; the rows
    of DIV have one solution, (a // b, a % b), and none when b = 0.  No equation can wrap: every side is below 2^17 << r."""
    a = np.arange(256, dtype=np.int64)[:, None]
    b = np.arange(256, dtype=np.int64)[None, :]
    s = a - b - 1 + 256                      # the only integer with a - b - 1 + 2^W - s = 0, and it has 9 bits
    assert s.min() >= 0 and s.max() < 512 and np.array_equal(s >> 8, (a > b).astype(np.int64))
    A = np.arange(256, dtype=np.int64)[:, None]
    for bv in range(256):
        rem = np.arange(256, dtype=np.int64)[None, :]
        t = bv - 1 - rem                     # row 2: b - 1 - rem = t with t in [0, 256)
        ok_rem = (t >= 0) & (t < 256)
        num = A - rem                        # row 1: q b = a - rem with q in [0, 256)
        if bv == 0:
            assert not ok_rem.any()
            continue
        solves = ok_rem & (num >= 0) & (num % bv == 0) & (num // bv < 256)
        assert np.array_equal(solves.sum(axis=1), np.ones(256, dtype=np.int64))
        which = solves.argmax(axis=1)
        assert np.array_equal(which, np.arange(256) % bv)


@pytest.mark.parametrize("t", PM.UNSIGNED)
def test_sub_underflow_leaves_its_packing_row_unsatisfied(t):
    Wd = PM.width(t)
    P = UNITS["sub_%s" % W.PROGRAM_TYPES[t].lower()][0]
    for a, b in ((0, 1), (5, (1 << Wd) - 1), ((1 << (Wd - 1)) - 1, 1 << (Wd - 1))):
        cs = M.ConstraintSystem()
        _, outputs, status = W.build_program(cs, P.tape(), [], [a, b])
        lay = W.program_circuit_layout(P.tape())
        assert status == PM.UNDERFLOW and outputs == [(a - b) % (1 << Wd)]
        assert _failing_rows(cs) == [lay["row_at"][2] + Wd]
        assert all(v in (0, 1) for v in cs.witness)


@pytest.mark.parametrize("t", (U8, U16, U32, U64))
def test_div_by_zero_leaves_its_range_row_unsatisfied(t):
    Wd = PM.width(t)
    P = UNITS["div_%s" % W.PROGRAM_TYPES[t].lower()][0]
    for a in (0, 1, (1 << Wd) - 1):
        cs = M.ConstraintSystem()
        _, outputs, status = W.build_program(cs, P.tape(), [], [a, 0])
        lay = W.program_circuit_layout(P.tape())
        assert status == PM.DIV_ZERO and outputs == [0]
        assert _failing_rows(cs) == [lay["row_at"][2] + 3 * Wd + 1]
        at = lay["witness_at"][2]
        bits = cs.witness[at:at + 3 * Wd]
        q, rem, tt = (sum(x << i for i, x in enumerate(bits[j * Wd:(j + 1) * Wd])) for j in range(3))
        assert (q, rem, tt) == (0, a, (-1 - a) % (1 << Wd))   # the documented wrapped values


# ------------------------------------------------------------------------------------------------------- the test circuit
def test_the_test_circuit_program_is_build_test_circuit_verbatim():
    tape = PM.test_circuit_program().tape()
    assert tape.hex() == GOLDEN["test_circuit"]["tape"] and GOLDEN["test_circuit"]["counts"] == [1, 16, 24]
    for a, b in ((0xA7, 0xA7), (0, 0), (255, 255), (3, 4)):
        ref = W.test_circuit(a, b)
        cs = M.ConstraintSystem()
        public, outputs, status = W.build_program(cs, tape, [], [a, b])
        assert cs.rows == ref.rows and cs.witness == ref.witness and cs.instance == ref.instance == [1]
        assert public == [] and outputs == [] and status == (0 if a == b else PM.ASSERT)
        assert (_failing_rows(cs) == []) == (a == b)
    assert _shape(tape) == (0, (1, 16, 24))
    again = M.MarlinInst._synthesize(W.ProgramSynthesizer(tape, [], [9, 9]))
    assert again.rows == W.test_circuit(9, 9).rows and again.witness == W.test_circuit(9, 9).witness


# ------------------------------------------------------------------------------------------------------- the mixed program
def test_mixed_program_rows_outputs_and_shape():
    gold = GOLDEN["mixed"]
    tape = PM.mixed_program().tape()
    assert tape.hex() == gold["tape"] and len(tape) // 32 - 1 == gold["instructions"] >= 48
    counts = tuple(gold["counts"])
    assert _shape(tape) == (0, counts) and max(counts[2], counts[0] + counts[1]) <= 1 << 13
    lay = W.program_circuit_layout(tape)
    assert (lay["num_instance"], lay["num_witness"], lay["num_constraints"]) == counts
    # the per-op formulas, instruction by instruction
    ins, _ = W.program_parse(tape)
    names = {"SHL": "shift_left", "SHR": "shift_right", "ROTL": "rotate_left", "ROTR": "rotate_right"}
    nw = nc = 0
    for k, (name, t, *_) in enumerate(ins):
        assert (lay["witness_at"][k], lay["row_at"][k]) == (nw, nc), (k, name)
        Wd = PM.width(t)
        if name == "INPUT_PRIVATE":
            nw, nc = nw + Wd, nc + Wd
        elif name in ("ASSERT_EQ", "OUTPUT"):
            nc += Wd
        elif name not in ("INPUT_PUBLIC", "CONST"):
            (wk, wc), (rk, rc) = FORMULA[names.get(name, name.lower())]
            nw, nc = nw + wk * Wd + wc, nc + rk * Wd + rc
    assert (nw, nc) == counts[1:]
    rows = PM.mixed_inputs(12)
    first = None
    for i, (pub, priv) in enumerate(rows):
        cs, public = W.program_circuit(tape, pub, priv)
        outputs, status = PM.mixed_eval(pub, priv)
        assert PM.hexes(pub) == gold["public"][i] and PM.hexes(priv) == gold["private"][i]
        assert PM.hexes(outputs) == gold["outputs"][i] and status == int(gold["status"][i]) == 0
        assert public == cs.instance[1:] == W.program_public_inputs(tape, pub, outputs)
        assert (len(cs.instance), len(cs.witness), cs.num_constraints) == counts
        assert _failing_rows(cs) == []
        # the shape depends on the tape alone: every assignment gives one matrix triple
        first = first or cs.rows
        assert cs.rows == first


def test_mixed_program_refusals_fail_their_own_rows():
    tape = PM.mixed_program().tape()
    gold = GOLDEN["mixed"]["refusals"]
    rows = PM.mixed_inputs(65, underflow=(31,), div_zero=(64,))
    lay = W.program_circuit_layout(tape)
    ins, _ = W.program_parse(tape)
    for i, expect in ((31, PM.UNDERFLOW), (64, PM.DIV_ZERO | PM.ASSERT)):
        cs = M.ConstraintSystem()
        _, outputs, status = W.build_program(cs, tape, *rows[i])
        assert status == expect == int(gold["status"][i]) and PM.hexes(outputs) == gold["outputs"][str(i)]
        bad = _failing_rows(cs)
        owners = {max(k for k in range(len(ins)) if lay["row_at"][k] <= r) for r in bad}
        assert {ins[k][0] for k in owners} == ({"SUB"} if i == 31 else {"DIV", "ASSERT_EQ"})


# ----------------------------------------------------------------------------------------------------- limits and refusals
def _tape(words):
    return W.program_header(len(words)) + b"".join(words)


def _refused(tape):
    with pytest.raises(ValueError):
        W.program_parse(tape)
    rc, _ = _shape(tape)
    assert rc == -1
    assert load_library().swm_last_error(None).decode().startswith("program_circuit_shape")
    with pytest.raises(M.MarlinError) as e:
        M.program_circuit_shape(tape)
    assert e.value.code == -1


def test_limits_and_refusals():
    w = W.program_word
    inp = [w("INPUT_PRIVATE", U8), w("INPUT_PRIVATE", U8)]
    ok = _tape(inp + [w("ADD", U8, 0, 1), w("OUTPUT", U8, 2)])
    assert _shape(ok) == (0, (9, 25, 34))
    # 4096 instructions pass, 4097 do not
    assert _shape(_tape(inp + [w("XOR", U8, 0, 1)] * 4094))[0] == 0
    _refused(_tape(inp + [w("XOR", U8, 0, 1)] * 4095))
    # the header
    _refused(b"")
    _refused(ok[:31])
    _refused(b"SWMPROG2" + ok[8:])
    _refused(ok[:12] + b"\1" + ok[13:])
    _refused(ok[:-1])
    _refused(ok + bytes(32))
    _refused(W.program_header(5) + ok[32:])
    # U128 MUL and DIV, arithmetic and shifts on BOOL
    for t, op in ((U128, "MUL"), (U128, "DIV"), (BOOL, "ADD"), (BOOL, "GT"), (BOOL, "SHL")):
        _refused(_tape([w("INPUT_PRIVATE", t), w("INPUT_PRIVATE", t), w(op, t, 0, 1 if op != "SHL" else 0)]))
    assert _shape(_tape([w("INPUT_PRIVATE", U128)] * 2 + [w("ADD", U128, 0, 1)]))[0] == 0
    # codes, reserved bytes, operands, immediates
    _refused(_tape(inp + [bytes([0, U8]) + bytes(30)]))
    _refused(_tape(inp + [bytes([26, U8]) + bytes(30)]))
    _refused(_tape(inp + [bytes([W.PROGRAM_OP["NOT"], 6]) + bytes(30)]))
    word = bytearray(w("ADD", U8, 0, 1))
    word[9] = 1
    _refused(_tape(inp + [bytes(word)]))
    _refused(_tape(inp + [w("ADD", U8, 0, 2)]))                      # a register that is not defined yet (its own)
    _refused(_tape(inp + [w("ADD", U8, 0, 0xFFFF)]))
    _refused(_tape(inp + [w("ADD", U16, 0, 1)]))                     # of another type
    _refused(_tape(inp + [w("NOT", U8, 0, 1)]))                      # an unused operand field that is set
    _refused(_tape(inp + [w("ADD", U8, 0, 1, imm=1)]))               # an immediate where none belongs
    _refused(_tape(inp + [w("SELECT", U8, 0, 0, 1)]))                # the condition is no BOOL
    _refused(_tape(inp + [w("CONST", U8, imm=256)]))
    _refused(_tape(inp + [w("CONST", BOOL, imm=2)]))
    _refused(_tape(inp + [w("CONST", U64, imm=1 << 64)]))
    assert _shape(_tape(inp + [w("CONST", U128, imm=(1 << 128) - 1)]))[0] == 0
    _refused(_tape(inp + [w("SHL", U8, 0, imm=1 << 32)]))
    assert _shape(_tape(inp + [w("ROTR", U8, 0, imm=(1 << 32) - 1)]))[0] == 0
    # inputs come first, public then private
    _refused(_tape(inp + [w("XOR", U8, 0, 1), w("INPUT_PRIVATE", U8)]))
    _refused(_tape(inp + [w("INPUT_PUBLIC", U8)]))
    _refused(_tape([w("INPUT_PUBLIC", U8, imm=1)]))
    # NULL outputs
    lib = load_library()
    n = ctypes.c_size_t(0)
    buf = (ctypes.c_uint8 * len(ok)).from_buffer_copy(ok)
    assert lib.swm_program_circuit_shape(buf, len(ok), None, ctypes.byref(n), ctypes.byref(n)) == -1
    assert lib.swm_program_circuit_shape(None, 64, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == -1


def test_builder_names_and_its_refusals():
    P = Program()
    a, b, c = P.private_input(U32), P.private_input(U32), P.private_input(BOOL)
    for name in ("and_", "or_", "xor", "nand", "nor", "add", "sub", "mul", "div", "shift_left", "shift_right", "rotate_left",
                 "rotate_right", "compare", "is_eq", "enforce_equal", "not_"):
        assert callable(getattr(a, name))
    r = P.select(c, a.add(b), a)
    assert r.type == U32 and a.compare(b, "lte").type == BOOL and a.is_eq(b).type == BOOL
    with pytest.raises(ValueError):
        a.add(c)
    with pytest.raises(ValueError):
        a.compare(b, "ne")
    with pytest.raises(ValueError):
        P.select(a, a, b)
    Q = Program()
    x = Q.private_input(U128)
    x.mul(x)
    with pytest.raises(ValueError):
        Q.tape()
    with pytest.raises(ValueError):
        W.program_public_inputs(PM.mixed_program().tape(), [1], [])
    with pytest.raises(ValueError):
        W.build_program(M.ConstraintSystem(), PM.test_circuit_program().tape(), [], [1])


def test_header_binding_and_ffi_declare_the_seven_symbols():
    ffi = open(os.path.join(ROOT, "swmarlin-sys", "src", "ffi.rs")).read()
    hdr = open(os.path.join(ROOT, "include", "swmarlin.h")).read()
    for name in ("swm_program_circuit_shape", "swm_program_create", "swm_program_destroy", "swm_program_witness", "swm_program_witness_dev",
                 "swm_program_prove", "swm_program_prove_many"):
        assert "pub fn %s(" % name in ffi and "%s(" % name in hdr
        assert hasattr(load_library(), name)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shape_under_asan_ubsan(tmp_path):
    """csrc/host/program_shape.h — the validator, the counts and the plan the kernels address by — over the fixture tapes and 10 000
    seeded mutations of them, in a stand-alone program (tests/native/program_shape_check.cpp) built with
    -fsanitize=address,undefined: every mutant is refused or has a plan that holds the kernels' invariants."""
    exe = str(tmp_path / "program_shape_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "simpleworks_amd", "csrc"), os.path.join(ROOT, "tests", "native", "program_shape_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and ("asan" in out.stderr.lower() or "ubsan" in out.stderr.lower()) and "error:" not in out.stderr:
        pytest.skip("this g++ has no ASan / UBSan runtime")
    assert out.returncode == 0, out.stderr[-4000:]
    tapes = [GOLDEN["unit"][k] for k in sorted(GOLDEN["unit"])] + [GOLDEN["mixed"], GOLDEN["test_circuit"]]
    listing = tmp_path / "tapes.txt"
    listing.write_text("".join("%s %d %d %d\n" % (g["tape"], *g["counts"]) for g in tapes))
    run = subprocess.run([exe, str(listing)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    words = run.stdout.split()
    assert words[:2] == ["ok", str(len(tapes))] and int(words[2]) + int(words[3]) == 10000
    assert int(words[2]) >= 500 and int(words[3]) >= 500   # both kinds of mutant occur in number

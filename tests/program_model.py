"""What the program tests share: the unit programs (one op each), the mixed program, their operands, and the semantics of every op
in PLAIN PYTHON INTEGERS — written from the reference's gadgets (src/gadgets/*.rs), not from workloads.build_program, which is the
thing under test.  tests/golden/gen_golden_program.py writes tests/golden/program.json from these."""
import random

from simpleworks_amd import workloads as W
from simpleworks_amd.program import BOOL, U8, U16, U32, U64, U128, Program

TYPES = (BOOL, U8, U16, U32, U64, U128)
UNSIGNED = (U8, U16, U32, U64, U128)
BITWISE = ("and", "or", "xor", "nand", "nor")
COMPARISONS = ("gt", "gte", "lt", "lte")
SHIFTS = ("shift_left", "shift_right", "rotate_left", "rotate_right")
UNDERFLOW, DIV_ZERO, ASSERT = 1, 2, 4


def width(t):
    return 1 if t == BOOL else 4 << t


def py_op(op, Wd, a, b=0, c=0, positions=0):
    """(result, status) of one op on Wd-bit values, as the reference's gadgets define it (status: what they refuse)."""
    mask = (1 << Wd) - 1
    if op == "and":
        return a & b, 0
    if op == "or":
        return a | b, 0
    if op == "xor":
        return a ^ b, 0
    if op == "nand":
        return ~(a & b) & mask, 0
    if op == "nor":
        return ~(a | b) & mask, 0
    if op == "not":
        return ~a & mask, 0
    if op == "add":
        return (a + b) % (1 << Wd), 0
    if op == "sub":
        return ((a - b) % (1 << Wd), 0) if a >= b else ((a - b) % (1 << Wd), UNDERFLOW)
    if op == "mul":
        return (a * b) % (1 << Wd), 0
    if op == "div":
        return (a // b, 0) if b else (0, DIV_ZERO)
    if op == "shift_left":
        return ((a << positions) & mask if positions < Wd else 0), 0
    if op == "shift_right":
        return (a >> positions if positions < Wd else 0), 0
    if op in ("rotate_left", "rotate_right"):
        k = positions % Wd
        if op == "rotate_right":
            k = (Wd - k) % Wd
        return ((a << k) | (a >> (Wd - k))) & mask, 0
    if op == "gt":
        return int(a > b), 0
    if op == "gte":
        return int(a >= b), 0
    if op == "lt":
        return int(a < b), 0
    if op == "lte":
        return int(a <= b), 0
    if op == "eq":
        return int(a == b), 0
    if op == "select":
        return (a if c else b), 0
    raise ValueError(op)


def hexes(values):
    """Values as the fixture writes them: one string of hex words."""
    return " ".join("%x" % v for v in values)


def extremal(Wd):
    """The pairs over {0, 1, 2^(W-1) - 1, 2^(W-1), 2^W - 1} (for a BOOL: over {0, 1})."""
    values = sorted({0, 1 & ((1 << Wd) - 1), (1 << (Wd - 1)) - 1, 1 << (Wd - 1), (1 << Wd) - 1})
    return [(a, b) for a in values for b in values]


def operands(Wd):
    """The extremal pairs, then eight seeded random ones."""
    rng = random.Random(0x5157 + Wd)
    return extremal(Wd) + [(rng.getrandbits(Wd), rng.getrandbits(Wd)) for _ in range(8)]


def unit_programs():
    """name -> (Program, op, type, positions): two private inputs (three for select: the condition last), the op, OUTPUT."""
    out = {}

    def unit(name, op, t, positions=0):
        P = Program()
        a, b = P.private_input(t), P.private_input(t)
        if op in BITWISE or op in ("add", "sub", "mul", "div"):
            method = {"and": "and_", "or": "or_"}.get(op, op)
            r = getattr(a, method)(b)
        elif op == "not":
            r = a.not_()
        elif op in SHIFTS:
            r = getattr(a, op)(positions)
        elif op in COMPARISONS:
            r = a.compare(b, op)
        elif op == "eq":
            r = a.is_eq(b)
        else:
            r = P.select(P.private_input(BOOL), a, b)
        P.output(r)
        out[name] = (P, op, t, positions)
    for t in TYPES:
        tn = W.PROGRAM_TYPES[t].lower()
        for op in BITWISE + ("not", "eq", "select"):
            unit("%s_%s" % (op, tn), op, t)
        if t == BOOL:
            continue
        for op in ("add", "sub") + COMPARISONS + (("mul", "div") if t != U128 else ()):
            unit("%s_%s" % (op, tn), op, t)
        for op in SHIFTS:
            for positions in (0, 1, width(t) - 1, width(t), width(t) + 1):
                unit("%s_%s_%d" % (op, tn, positions), op, t, positions)
    return out


def unit_cases(op, t, positions, pairs=None):
    """[(private values, output, status)] of a unit program over `pairs` (default: operands(W))."""
    Wd = width(t)
    cases = []
    for k, (a, b) in enumerate(operands(Wd) if pairs is None else pairs):
        c = (k ^ (k >> 1)) & 1
        value, status = py_op(op, Wd, a, b, c, positions)
        cases.append(([a, b, c] if op == "select" else [a, b], value, status))
    return cases


# ---------------------------------------------------------------------------------------------------------------- the mixed program
def mixed_program():
    """48 instructions over all six types: 2 public and 9 private inputs, every op family, 7 outputs.  SUB on U64 underflows when
    d < e; DIV on U32 has the divisor c."""
    P = Program()
    x8, fl = P.public_input(U8), P.public_input(BOOL)
    a16, b32, c32 = P.private_input(U16), P.private_input(U32), P.private_input(U32)
    d64, e64 = P.private_input(U64), P.private_input(U64)
    f128, g128 = P.private_input(U128), P.private_input(U128)
    h8, k = P.private_input(U8), P.private_input(BOOL)
    t4 = x8.xor(P.constant(U8, 0x5A)).add(h8).rotate_left(3).nand(x8)
    n16 = a16.mul(P.constant(U16, 257)).shift_right(5).nor(a16)
    q32 = b32.div(c32)
    d32 = b32.sub(q32.mul(c32))
    P.constant(BOOL, 1).enforce_equal(d32.compare(c32, "lt"))
    x64 = d64.sub(e64).add(d64).xor(e64.rotate_right(17))
    o64 = P.select(d64.compare(e64, "gte"), x64, d64).or_(e64.shift_left(60))
    f2 = f128.add(g128).and_(g128.not_())
    eq = f2.is_eq(f128)
    b4 = f128.compare(g128, "gt").xor(eq).or_(k).and_(fl).nor(f128.compare(g128, "lte"))
    b5 = P.select(fl, b4, k)
    eq8 = t4.is_eq(h8)
    for r in (t4, n16, d32, o64, f2, b5, eq8):
        P.output(r)
    return P


def mixed_eval(public, private):
    """(outputs, status) of mixed_program in plain integers."""
    x8, fl = public
    a16, b32, c32, d64, e64, f128, g128, h8, k = private
    status = 0
    t = py_op("rotate_left", 8, (x8 ^ 0x5A) + h8 & 0xFF, positions=3)[0]
    t4 = ~(t & x8) & 0xFF
    n16 = ~((a16 * 257 % 65536 >> 5) | a16) & 0xFFFF
    q32, st = py_op("div", 32, b32, c32)
    status |= st
    d32, st = py_op("sub", 32, b32, q32 * c32 % (1 << 32))
    status |= st
    if not d32 < c32:
        status |= ASSERT
    s64, st = py_op("sub", 64, d64, e64)
    status |= st
    x64 = ((s64 + d64) % (1 << 64)) ^ py_op("rotate_right", 64, e64, positions=17)[0]
    o64 = (x64 if d64 >= e64 else d64) | (e64 << 60) % (1 << 64)
    f2 = (f128 + g128) % (1 << 128) & ~g128 & ((1 << 128) - 1)
    eq = int(f2 == f128)
    b4 = 1 - ((((int(f128 > g128) ^ eq) | k) & fl) | int(f128 <= g128))
    b5 = b4 if fl else k
    return [t4, n16, d32, o64, f2, b5, int(t4 == h8)], status


def mixed_inputs(count, seed=1, underflow=(), div_zero=()):
    """`count` executions (public, private) with status 0, except the items named: d < e there, or c = 0."""
    rng = random.Random(seed)
    rows = []
    for i in range(count):
        d, e = sorted((rng.getrandbits(64), rng.getrandbits(64)), reverse=True)
        if i % 7 == 3:
            e = d
        f, g = rng.getrandbits(128), rng.getrandbits(128)
        if i % 5 == 2:
            g = 0   # f2 = f: the EQ of the program is true
        c = rng.getrandbits(32) | 1
        if i in underflow:
            d, e = min(d, e - 1) if e else 0, max(e, 1)
        if i in div_zero:
            c = 0
        rows.append(([rng.getrandbits(8), i & 1], [rng.getrandbits(16), rng.getrandbits(32), c, d, e, f, g, rng.getrandbits(8), (i >> 1) & 1]))
    return rows


def test_circuit_program():
    """examples/test-circuit.rs:13-26 as a program: two private U8 and one enforce_equal."""
    P = Program()
    a, b = P.private_input(U8), P.private_input(U8)
    a.enforce_equal(b)
    return P


test_circuit_program.__test__ = False

"""Seeded random R1CS of irregular shape, emitted into any object with the builder vocabulary (one, new_input_variable,
new_witness_variable, enforce_constraint): pyref.marlin.ConstraintSystem (the model) and
simpleworks_amd.marlin.ConstraintSystem (the product) build the same system from the same parameters.

A row is (A-combination) * (B-combination) = C.  C is a fresh witness that holds the product (times a small coefficient) or,
when the product is zero, sometimes nothing.  A combination draws its columns without repetition, then may gain a term
with a zero coefficient, a second term on a column it already holds, and a pair of terms on a fresh column that cancel to
zero; its terms are then shuffled.  So the number of non-zeros of a combination once merged equals the number of columns
drawn first, whatever was added afterwards.

CASES is the table the fixture tests/golden/differential.json is generated from (tests/golden/gen_golden_differential.py).
"""
import random

from pyref.bls12_377 import R

DEFAULTS = dict(
    seed=0,
    inputs=2,            # public inputs (the instance holds the constant one in front of them)
    free=4,              # witnesses that no row defines
    rows=8,              # random rows
    a=[1, 3], b=[1, 3],  # columns drawn per combination: [lo, hi]
    p_empty_a=0.0, p_empty_b=0.0,  # a combination is empty
    p_empty_c=0.5,       # C is empty, given that the product is zero
    p_zero=0.0,          # a term with a zero coefficient is added
    p_dup=0.0,           # a second term on a column the combination already holds
    p_cancel=0.0,        # two terms on a fresh column that sum to zero
    zero_assignment=False,  # every variable but the constant one is zero
    a_without_one=False,    # A never reads the constant one
    fixed=[],            # rows of exactly [columns in A, columns in B], placed first
    hub=0,               # rows (hub witness) * 1 = fresh witness: one column used by that many rows
    empty_rows=0,        # rows with A, B and C empty: half of them first, the rest last
    repeat=0,            # rows enforced a second time, cyclically (more rows than variables)
)


def emit(cs, params):
    """Builds the system of `params` (a dict over DEFAULTS) into cs.  Returns the public input."""
    p = dict(DEFAULTS, **params)
    assert set(p) == set(DEFAULTS), sorted(set(p) - set(DEFAULTS))
    rnd = random.Random(p["seed"])

    def value():
        return 0 if p["zero_assignment"] else rnd.randrange(R)

    vars_, vals = [cs.one()], [1]
    for _ in range(p["inputs"]):
        v = value()
        vars_.append(cs.new_input_variable(v))
        vals.append(v)
    public = vals[1:]
    for _ in range(p["free"]):
        v = value()
        vars_.append(cs.new_witness_variable(v))
        vals.append(v)

    def coeff():
        return rnd.choice([1, 2, R - 1, rnd.randrange(1, R)])

    def combination(lo, hi, p_empty, first):
        if rnd.random() < p_empty:
            return [], 0
        pool = range(first, len(vars_))
        drawn = rnd.sample(pool, min(rnd.randint(lo, hi), len(pool)))
        terms = [(coeff(), k) for k in drawn]
        if rnd.random() < p["p_zero"]:
            terms.append((0, rnd.choice(pool)))
        if rnd.random() < p["p_dup"]:
            terms.append((rnd.randrange(1, R), rnd.choice(drawn)))
        rest = [k for k in pool if k not in drawn]
        if rnd.random() < p["p_cancel"] and rest:
            k, c = rnd.choice(rest), coeff()
            terms += [(c, k), (R - c, k)]
        rnd.shuffle(terms)
        return [(c, vars_[k]) for c, k in terms], sum(c * vals[k] for c, k in terms) % R

    rows = []

    def row(a, va, b, vb):
        prod = va * vb % R
        if prod == 0 and rnd.random() < p["p_empty_c"]:
            c = []
        else:
            k = rnd.choice([1, 1, 2, R - 1])
            w = cs.new_witness_variable(prod * pow(k, -1, R) % R)
            vars_.append(w)
            vals.append(prod * pow(k, -1, R) % R)
            c = [(k, w)]
        cs.enforce_constraint(a, b, c)
        rows.append((a, b, c))

    for _ in range(p["empty_rows"] // 2):
        cs.enforce_constraint([], [], [])
    first_a = 1 if p["a_without_one"] else 0
    for na, nb in p["fixed"]:
        a, va = combination(na, na, 0.0, first_a)
        b, vb = combination(nb, nb, 0.0, 0)
        row(a, va, b, vb)
    for _ in range(p["rows"]):
        a, va = combination(p["a"][0], p["a"][1], p["p_empty_a"], first_a)
        b, vb = combination(p["b"][0], p["b"][1], p["p_empty_b"], 0)
        row(a, va, b, vb)
    if p["hub"]:
        hub = 1 + p["inputs"]  # the first free witness
        assert p["free"] >= 1
        for _ in range(p["hub"]):
            c = coeff()
            row([(c, vars_[hub])], c * vals[hub] % R, [(1, cs.one())], 1)
    for i in range(p["repeat"]):
        cs.enforce_constraint(*rows[i % len(rows)])
    for _ in range(p["empty_rows"] - p["empty_rows"] // 2):
        cs.enforce_constraint([], [], [])
    return public


_MIX = dict(p_zero=0.3, p_dup=0.3, p_cancel=0.3)

CASES = [
    # ---- instance lengths 1, 2, 3, 4, 6, 9, 17 (the padded instance has 1, 2, 4, 4, 8, 16, 32 columns)
    ("in0_tall", dict(seed=101, inputs=0, free=3, rows=6, repeat=30, **_MIX)),
    ("in1", dict(seed=102, inputs=1, free=4, rows=10, a=[1, 4], b=[2, 5], **_MIX)),
    ("in2", dict(seed=103, inputs=2, free=3, rows=9, a=[2, 6], b=[1, 2])),
    ("in3", dict(seed=104, inputs=3, free=5, rows=12, a=[1, 3], b=[1, 3], **_MIX)),
    ("in5", dict(seed=105, inputs=5, free=4, rows=12, a=[1, 3], b=[2, 4], p_dup=0.5)),
    ("in8", dict(seed=106, inputs=8, free=2, rows=11, a=[1, 5], b=[1, 5], p_cancel=0.5)),
    # (free = 10: the SRS is sized from the unpadded system, so the 15 padding columns must not carry |H| past a power of two)
    ("in16", dict(seed=107, inputs=16, free=10, rows=10, a=[1, 8], b=[1, 3], p_zero=0.5)),
    # ---- rows against variables
    ("rows_eq_vars", dict(seed=111, inputs=3, free=4, rows=12, repeat=8, p_empty_c=0.0)),
    ("rows_gt_vars", dict(seed=112, inputs=1, free=2, rows=5, repeat=40, a=[1, 2], b=[1, 2], **_MIX)),
    # ---- |K| against |H|
    ("k_lt_h", dict(seed=121, inputs=0, free=40, rows=4, a=[1, 1], b=[1, 1])),
    ("k_eq_h", dict(seed=122, inputs=3, free=0, rows=12, a=[1, 1], b=[1, 1])),
    ("k_gt_h", dict(seed=123, inputs=2, free=3, rows=10, a=[4, 8], b=[3, 6], **_MIX)),
    # ---- empty combinations, rows and matrices
    ("empty_a_rows", dict(seed=131, inputs=2, free=4, rows=12, p_empty_a=0.4, **_MIX)),
    ("empty_b_rows", dict(seed=132, inputs=1, free=4, rows=12, p_empty_b=0.4, p_empty_c=0.3)),
    ("empty_ab_rows", dict(seed=133, inputs=3, free=3, rows=14, p_empty_a=0.3, p_empty_b=0.3, p_empty_c=0.7, **_MIX)),
    ("empty_rows", dict(seed=134, inputs=2, free=3, rows=8, empty_rows=5, p_empty_a=0.2, p_empty_c=1.0)),
    ("a_matrix_empty", dict(seed=135, inputs=1, free=4, rows=8, p_empty_a=1.0, p_empty_c=0.4, b=[1, 4])),
    ("c_matrix_empty", dict(seed=136, inputs=2, free=6, rows=9, zero_assignment=True, a_without_one=True, p_empty_c=1.0,
                            a=[1, 3], b=[1, 4], p_dup=0.3)),
    # ---- assignments
    ("zero_assignment", dict(seed=141, inputs=3, free=5, rows=10, zero_assignment=True, p_empty_c=0.3, **_MIX)),
    ("zero_assignment_no_inputs", dict(seed=142, inputs=0, free=6, rows=7, zero_assignment=True, p_empty_c=0.0, a=[2, 5])),
    # ---- balance: nnz(A) against nnz(B)
    ("a_denser", dict(seed=151, inputs=2, free=5, rows=10, a=[3, 6], b=[1, 2], p_zero=0.3)),
    ("b_denser", dict(seed=152, inputs=2, free=5, rows=10, a=[1, 2], b=[3, 6], p_cancel=0.3)),
    ("ab_tie", dict(seed=153, inputs=1, free=6, rows=11, a=[2, 2], b=[2, 2], p_dup=0.4)),
    # ---- long rows and columns
    ("row_64_65", dict(seed=161, inputs=0, free=65, rows=0, fixed=[[64, 1], [65, 1]], p_dup=1.0, p_cancel=1.0)),
    ("row_70", dict(seed=162, inputs=1, free=72, rows=2, fixed=[[70, 2]], p_zero=1.0, p_dup=1.0)),
    ("hub_66", dict(seed=163, inputs=1, free=2, rows=2, hub=66)),
    # ---- everything at once, three seeds
    ("mixed_1", dict(seed=171, inputs=4, free=6, rows=16, a=[1, 7], b=[1, 7], p_empty_a=0.15, p_empty_b=0.15, empty_rows=2,
                     **_MIX)),
    ("mixed_2", dict(seed=172, inputs=0, free=8, rows=20, a=[1, 9], b=[1, 4], p_empty_a=0.1, p_empty_b=0.2, repeat=5, **_MIX)),
    ("mixed_3", dict(seed=173, inputs=6, free=3, rows=18, a=[1, 4], b=[1, 9], p_empty_b=0.1, empty_rows=1, p_zero=0.6,
                     p_dup=0.6, p_cancel=0.6)),
    ("mixed_wide", dict(seed=174, inputs=2, free=30, rows=10, a=[6, 14], b=[1, 3], p_zero=0.5, p_dup=0.5, p_cancel=0.5)),
]

# cases without a public input: the bumped-input rejection has nothing to bump there
NO_PUBLIC_INPUT = [name for name, p in CASES if dict(DEFAULTS, **p)["inputs"] == 0]


def raw_csr(cs, to_mont_limbs):
    """The three matrices of a product ConstraintSystem as the builder was given them: every term in the order it was
    listed, no merging, no sorting, zero coefficients kept.  Columns follow the rule of ConstraintSystem._csr (instance
    columns first).  Returns three (rowptr, col, val) with val from to_mont_limbs(list of ints)."""
    import numpy as np
    ninst = len(cs.instance)
    out = []
    for rows in cs.rows:
        rowptr, cols, vals = [0], [], []
        for lc in rows:
            for coeff, (kind, k) in lc:
                cols.append(k if kind == "i" else ninst + k)
                vals.append(int(coeff))
            rowptr.append(len(cols))
        out.append((np.array(rowptr, dtype=np.uint32), np.array(cols, dtype=np.uint32),
                    to_mont_limbs(vals) if vals else np.zeros((0, 4), dtype=np.uint64)))
    return out

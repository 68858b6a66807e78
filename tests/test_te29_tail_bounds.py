"""The general addition of the 29-bit domain (csrc/fq29.cuh: te29_slot_add, te29_slot_add_sync, te29_quad_add, te29_store_384 — what
the one-lane bucket stage runs) on the CPU, through the `tail` part of tools/check_te29.py: the column bound of each of the nine
products and of the store's with every limb at its documented maximum, and the limb-level emulation on chains of slot_add steps
— running sum, weighted sum, scan, the shift phase's doublings, fold and tree — against the group law on Python integers."""
import importlib.util
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
LIMIT = (1 << 64) - (1 << 29)


@pytest.fixture(scope="module")
def te29():
    sys.path.insert(0, TOOLS)
    try:
        spec = importlib.util.spec_from_file_location("check_te29_tail", os.path.join(TOOLS, "check_te29.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(TOOLS)
    return mod


def test_worst_column_is_below_the_limit(te29):
    """Nine products and the store's, widest accepted operand forms (X below 3p, Y below 2p, T and Z: N — doubling and the identity are
    operands of those forms): the worst column stays below 2^64 - 2^29, and would not with neither first-round operand normalised."""
    bounds = te29.worst_case_tail()
    assert len(bounds) == 10, bounds
    worst = max(bounds.values())
    print("worst column %.4f x 2^64" % worst)
    assert worst * (1 << 64) < LIMIT, bounds
    raw = te29.worst_case_tail(norm_first=False)
    assert raw["A (Y1-X1+4p)(Y2-X2+4p)"] > 1.0 and raw["B (Y1+X1)(Y2+X2)"] > 1.0, raw


def test_build_time_table_is_the_tools(te29):
    """csrc/te29_bounds_gen.inc, which fq29.cuh's static_assert evaluates, is what the tool emits from the operand maxima it
    bounds — and fq29.cuh includes it and asserts over all of its rows."""
    csrc = os.path.join(ROOT, "simpleworks_amd", "csrc")
    with open(os.path.join(csrc, "te29_bounds_gen.inc")) as f:
        assert f.read() == te29.bounds_header()
    assert set(te29.tail_operands()) == set(te29.worst_case_tail())
    src = open(os.path.join(csrc, "fq29.cuh")).read()
    assert '#include "te29_bounds_gen.inc"' in src and "static_assert(te29_slot_add_bounds_ok()" in src
    assert "for (const Te29Bound& r : TE29_TAIL_BOUNDS)" in src


def test_tool_entry_point(te29):
    """what `python tools/check_te29.py tail` runs: its own chains, the printed worst column and its assertion"""
    worst, n = te29.tail_main(2, verbose=False)
    assert worst * (1 << 64) < LIMIT and n > 200


def test_bucket_stages_match_the_group_law(te29):
    """Bucket stages of 4 and 8 lanes, one, two and four buckets per lane, on partial sums of every accepted form (first of a segment,
    after additions, the identity for an empty bucket, a repeated partial sum, P and -P in one bucket): every step of the walk
    and the stage's (A, R) equal the reference, A = sum (b + 1) S_b and R = sum S_b; no limb or column wraps."""
    rng = random.Random(2931)
    te29.peak[0] = 0
    pool = [te29.g1_mul_fast(te29.G, rng.randrange(1, te29.R)) for _ in range(24)]
    total = 0
    for lanes, log_m in ((4, 0), (4, 2), (8, 1)):
        parts, wref = [], []
        for b in range(lanes << log_m):
            kind = (b + lanes) % 6
            segs, ref = [], None
            if kind in (1, 2, 3):
                for _ in range(2 if kind == 2 else 1):
                    pts = [rng.choice(pool) for _ in range(1 if kind == 3 else rng.randrange(2, 5))]
                    signs = [rng.random() < 0.5 for _ in pts]
                    a, r = te29.run_chain(pts, signs)
                    segs.append(a)
                    ref = te29.g1_add(ref, r)
            if kind == 4:
                a, r = te29.run_chain([rng.choice(pool), rng.choice(pool)], [False, True])
                segs, ref = [a, a], te29.g1_add(r, r)
            if kind == 5:
                pt = rng.choice(pool)
                segs = [te29.from_row(*te29.row_of(pt), False), te29.from_row(*te29.row_of(pt), True)]
            parts.append(segs or [te29.IDENT])
            wref.append(ref)
        total += te29.bucket_stage(parts, lanes, log_m, wref)[2]
    assert total > 150 and te29.peak[0] < LIMIT


def test_extremal_slots_do_not_wrap(te29):
    """Slots with every coordinate at the edge of its accepted form, in value and in limb pattern, and the identity: every ordered
    pair through an addition, the sum doubled and added back; every product is the Montgomery product of its operands and comes
    back N, every result is a slot in form (asserted inside the emulation)."""
    te29.peak[0] = 0
    ext = te29.extremal_points()
    assert len(ext) == 8
    for a in ext:
        for q in ext:
            r = te29.slot_add(a, q)
            te29.slot_add(q, te29.slot_add(r, r))
            te29.store_384(r)
    assert 0 < te29.peak[0] < LIMIT

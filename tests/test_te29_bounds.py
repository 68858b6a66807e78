"""The 29-bit limb form of the accumulation (csrc/fq29.cuh) on the CPU, through tools/check_te29.py: the bit-level emulation —
every uint32 limb operation, every 64-bit column sum with the asm carry rule — on random chains of subgroup points (each step
against the group law on Python integers) and on chains of extremal rows; the interval bound of every product's columns with each
limb at its documented maximum; and the multiplier generator against the three committed texts."""
import importlib.util
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
CSRC = os.path.join(ROOT, "simpleworks_amd", "csrc")


@pytest.fixture(scope="module")
def te29():
    sys.path.insert(0, TOOLS)
    try:
        spec = importlib.util.spec_from_file_location("check_te29", os.path.join(TOOLS, "check_te29.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(TOOLS)
    return mod


def test_random_chains_match_the_group_law(te29):
    """300 chains of 2 .. 9 entries with random signs over a pool of random subgroup points, the identity, repeated points
    (doubling) and opposite ones (cancellation): no wrap anywhere, every intermediate sum the reference's point, and the
    epilogue's slot an N value of the 28-bit domain standing for the same point."""
    rng = random.Random(2901)
    pool = [te29.g1_mul_fast(te29.G, rng.randrange(1, te29.R)) for _ in range(40)] + [None, te29.G]
    n_add = 0
    for c in range(300):
        pts = [rng.choice(pool) for _ in range(rng.randrange(2, 10))]
        signs = [rng.random() < 0.5 for _ in pts]
        if c % 10 == 1:
            pts[1], signs[1] = pts[0], signs[0]          # P + P through the unified law
        if c % 10 == 2:
            pts[1], signs[1] = pts[0], not signs[0]      # P + (-P)
        if c % 10 == 3:
            pts[-1] = None                               # P + O
        acc, ref = te29.run_chain(pts, signs)
        n_add += len(pts) - 1
        if c % 5 == 0:
            assert te29.c28.to_w([te29.to_slot(v) for v in acc]) == ref
    assert n_add >= 1000 and te29.peak[0] < 1 << 64


def test_extremal_rows_do_not_wrap(te29):
    """Rows with every limb full, with coordinates p - 1, 0 and 1, and the identity row, each as the first entry of a segment and as
    the row of six successive additions, both signs: every limb operation and column stays in range, every product is the
    Montgomery product of its operands and comes back N (asserted inside the emulation), the epilogue's slot is in form."""
    assert te29.run_extremal() == 5 * 2 * 5 * 2 * 6
    assert te29.peak[0] < 1 << 64


def test_worst_case_column_bound_is_below_2_64(te29):
    """Every product of te29_from_row, te29_madd_row and te29_to_slot with each operand limb at its documented maximum and every
    m_k at 2^29 - 1: the largest column sum, carry rule included, is below 2^64 with F and H normalised — and above it with
    fewer normalisations, which is why there are two."""
    bounds = te29.worst_case("FH")
    assert len(bounds) == 13 and max(bounds.values()) < 1.0, bounds
    for fewer in ("", "F", "H", "E", "G"):
        assert max(te29.worst_case(fewer).values()) > 1.0, fewer
    assert max(te29.worst_case("EG").values()) >= max(bounds.values())


@pytest.mark.parametrize("mode, name", [("fq28", "fq28_mul_asm.inc"), ("fr29", "fr29_mul_asm.inc"), ("fq29", "fq29_mul_asm.inc")])
def test_generator_reproduces_the_committed_text(mode, name):
    out = subprocess.run([sys.executable, os.path.join(TOOLS, "gen_mul28_asm.py"), mode], check=True, capture_output=True).stdout
    with open(os.path.join(CSRC, name), "rb") as f:
        assert out == f.read()

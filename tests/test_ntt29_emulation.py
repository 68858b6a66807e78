"""A reduced run of tools/check_ntt29.py (the bit-level emulation of fr29.cuh + ntt_pass_lazy with the host plan mirrored in its
plan()) on the inputs at which the plan's bounds are tight, so that a change to lazy_plan that is carried over to the emulator meets
these inputs in every run of the non-GPU suite: the extremal tiles (all b0 r - 1, all zero, top / 0 alternating at every butterfly
distance) at every tile size up to 2^8 and both input bounds, and whole transforms of the reduced edge inputs (constants, combs
next to the pass boundary and at both ends, root orbits) against their closed forms for the plans (6, 2) (all four directions /
variants), (8, 4) (forward coset: b_in = 2 in both passes) and (9, 3) (inverse coset: b_in = 1 first, the scaled store last).

About 10 s of pure Python.  `python tools/check_ntt29.py` adds: the tiles of 2^9 .. 2^12 elements (the sizes at which the b_in = 1
chain reaches B = 64 and the sixth radix-4 step exists), every comb level, the single-element and tight-fill inputs, all four
directions / variants for every plan the tool lists (the one-pass 2^10 among them), the random transforms against the direct DFT
and the closed forms themselves against the direct DFT."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import check_ntt29 as C  # noqa: E402

FWD, FWD_COSET, INV, INV_COSET = (False, False), (False, True), (True, False), (True, True)


def test_extremal_tiles_hold_every_bound():
    assert C.check_tiles(8) == sum(2 * (2 + 2 * log_r) for log_r in range(1, 9))


def test_closed_forms_equal_the_direct_dft():
    """the second reference of tests/test_gpu_ntt_edges.py, against the quadratic sum at a size with every family distinct"""
    for d in C.edge_inputs(4, 2):
        x = C.materialize(d, 4)
        for inverse, coset in (FWD, FWD_COSET, INV, INV_COSET):
            assert C.closed_form(d, 4, inverse, coset) == C.dft(x, 4, inverse, coset), (d, inverse, coset)


@pytest.mark.parametrize("plan, variants", [((6, 2), (FWD, FWD_COSET, INV, INV_COSET)), ((8, 4), (FWD_COSET,)), ((9, 3), (INV_COSET,))])
def test_extremal_transforms_equal_their_closed_forms(plan, variants):
    """three, two and three passes (b_in = 2 from the second pass on, and in the first pass of a forward coset transform)"""
    n_inputs = len(C.edge_inputs(plan[0], C.pass_radices(*plan)[0], reduced=True))
    assert C.check_edge_transforms((plan,), variants, reduced=True) == n_inputs * len(variants)

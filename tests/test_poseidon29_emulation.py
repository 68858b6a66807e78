"""CPU test: the Poseidon kernel's limb arithmetic (csrc/poseidon.hip), emulated bit for bit by tools/check_poseidon29.py on the
multiplier model of tools/check_ntt29.py, holds every bound it states and equals the big-integer model — a subset of the tool's
own run (parameter sets of r - 1 and of the reference, the smallest and the largest alpha, with and without partial rounds)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import check_poseidon29 as E
import poseidon_model as P

PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")


def test_limb_flow_holds_its_bounds_and_equals_the_model():
    ref = P.load_params(PARAMS)
    assert E.check(ref, fills=("r-1", "reference"), shapes=((8, 29), (2, 0)), alphas=(2, 17)) == 30
    assert E.check(ref, fills=("r-1",), shapes=((2, 1),), alphas=(65535,)) == 5
    assert E.max_limb < 5 << 29
    data = b"Hello World"
    assert E.hash_elements(ref, P.pack_bytes(data), 1)[0] == P.hash_bytes(ref, data)

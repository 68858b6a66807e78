"""Writes tests/golden/program.json: the tapes of the unit programs, of the mixed program and of the test-circuit program as hex,
the unit programs' operands and the inputs of the mixed program's first items (the rest follow from the same seed), the expected
outputs and status bytes — from plain Python integers (tests/program_model.py) — and the three counts of
each circuit, from workloads.build_program.  Every case is run through build_program on the way: the builder's outputs and status
must be the integers', or nothing is written.

    python tests/golden/gen_golden_program.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import program_model as PM  # noqa: E402
from simpleworks_amd import marlin as M, workloads as W  # noqa: E402

MIXED_COUNT = 257
MIXED_INPUTS = 16


def counts(tape):
    lay = W.program_circuit_layout(tape)
    return [lay["num_instance"], lay["num_witness"], lay["num_constraints"]]


def hexes(values):
    """Values as one string of hex words: the fixture stays a few hundred lines."""
    return " ".join("%x" % v for v in values)


def main():
    line = lambda obj: json.dumps(obj, sort_keys=True, separators=(",", ":"))  # noqa: E731
    unit = []
    for name, (P, op, t, positions) in PM.unit_programs().items():
        tape = P.tape()
        cases = PM.unit_cases(op, t, positions)
        for private, value, status in cases:
            cs = M.ConstraintSystem()
            _, outputs, st = W.build_program(cs, tape, [], private)
            assert outputs == [value] and st == status, (name, private, outputs, value, st, status)
        unit.append((name, {"tape": tape.hex(), "op": op, "type": t, "positions": positions, "counts": counts(tape),
                            "outputs": hexes(v for _, v, _ in cases), "status": "".join(str(s) for _, _, s in cases)}))
    mixed = PM.mixed_program().tape()
    rows = PM.mixed_inputs(MIXED_COUNT)
    results = [PM.mixed_eval(pub, priv) for pub, priv in rows]
    for (pub, priv), (outputs, status) in list(zip(rows, results))[:MIXED_INPUTS]:
        got = W.build_program(M.ConstraintSystem(), mixed, pub, priv)
        assert got[1] == outputs and got[2] == status == 0, (pub, priv, got[1:], outputs, status)
    bad = PM.mixed_inputs(65, underflow=(31,), div_zero=(64,))
    bad_results = [PM.mixed_eval(pub, priv) for pub, priv in bad]
    assert [i for i, r in enumerate(bad_results) if r[1]] == [31, 64]
    assert all(bad_results[i] == results[i] for i in range(65) if i not in (31, 64))   # the other items are the first 65 of the batch
    tc = PM.test_circuit_program().tape()
    out = ['{"format":"SWMPROG1",', '"operands":{']
    out += ['"%d":%s,' % (PM.width(t), line(hexes(v for pair in PM.operands(PM.width(t)) for v in pair))) for t in PM.TYPES]
    out[-1] = out[-1][:-1] + "},"
    out.append('"unit":{')
    out += ["%s:%s," % (line(name), line(entry)) for name, entry in sorted(unit)]
    out[-1] = out[-1][:-1] + "},"
    # the mixed program: the inputs of the first items (the rest come from the same seed), the outputs and status bytes of all
    out.append('"mixed":{"tape":%s,"counts":%s,"instructions":%d,' % (line(mixed.hex()), line(counts(mixed)), len(mixed) // 32 - 1))
    out.append('"public":%s,' % line([hexes(pub) for pub, _ in rows[:MIXED_INPUTS]]))
    out.append('"private":[')
    out += [line(hexes(priv)) + "," for _, priv in rows[:MIXED_INPUTS]]
    out[-1] = out[-1][:-1] + "],"
    out.append('"outputs":[')
    out += [",".join(line(hexes(o)) for o, _ in results[k:k + 4]) + "," for k in range(0, MIXED_COUNT, 4)]
    out[-1] = out[-1][:-1] + "],"
    out.append('"status":%s,' % line("".join(str(s) for _, s in results)))
    out.append('"refusals":%s},' % line({"underflow": 31, "div_zero": 64, "status": "".join(str(s) for _, s in bad_results),
                                         "outputs": {str(i): hexes(bad_results[i][0]) for i in (31, 64)}}))
    out.append('"test_circuit":%s}' % line({"tape": tc.hex(), "counts": counts(tc)}))
    path = os.path.join(HERE, "program.json")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    with open(path) as f:
        json.load(f)
    print("wrote %s: %d unit programs, %d bytes" % (path, len(unit), os.path.getsize(path)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the witness synthesis of integer programs (csrc/program_witness.hip) for the mixed program of the tests and for one
64-instruction U64 program, at 2^12 executions each, and in the same process a hipMemsetAsync of the witness's byte count: the
store rate the machine grants.  Then swm_program_prove_many against count x swm_program_prove on the mixed program.

    python tools/program_time.py [--runs 15] [--out profiles/program_time.txt]

Kernel times (program_exec, program_inverse, program_expand) come from the library's own HIP events around its launches
(swm_profile_*), the whole swm_program_witness_dev call from a host clock around the call and a synchronise, the memset from two HIP
events on the stream it runs on; each figure is the median, minimum and maximum of --runs launches after a warm-up.  The first items
of every timed output are compared with workloads.build_program first: what is timed is also right.  There is no threshold: the
figures go to the output file.  Needs an MI355X: there is no fallback."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from blake2s_time import memset_ms  # noqa: E402  (tools/ is on the path when run as a script)


def u64_program():
    """64 instructions on U64: two private inputs, 61 ops that chain through every family, one output."""
    from simpleworks_amd.program import U64, Program
    P = Program()
    a, b = P.private_input(U64), P.private_input(U64)
    x, y = a, b
    for k in range(52):
        step = k % 6
        if step == 0:
            x = x.add(y)
        elif step == 1:
            y = y.xor(x)
        elif step == 2:
            x = x.rotate_left(13 + k)
        elif step == 3:
            y = y.mul(x)
        elif step == 4:
            x = x.and_(y).not_() if k % 12 == 4 else x.or_(y)
        else:
            y = P.select(x.compare(y, "gt"), y, x) if k % 12 == 5 else y.shift_right(3)
    P.output(x.xor(y))
    assert len(P.tape()) // 32 - 1 == 64
    return P


def stats(xs):
    return statistics.median(xs), min(xs), max(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "program_time.txt"))
    args = ap.parse_args()
    assert args.runs >= 15, "median of at least 15 launches"
    import program_model as PM
    from simpleworks_amd import _lib, marlin as M, program as PG, workloads as W

    ctx = M.default_context()
    hip = ctypes.CDLL("libamdhip64.so")   # the runtime the library already runs on
    lines = ["Integer programs, one MI355X, library %s; 2^12 executions per launch; median (min, max) of %d launches after a warm-up"
             % (os.path.basename(_lib.LIB_PATH), args.runs)]
    n = 1 << 12
    rnd = np.random.default_rng(1)
    mixed_rows = PM.mixed_inputs(n)
    u64 = u64_program()
    u64_rows = [([], [int(v[0]), int(v[1])]) for v in rnd.integers(0, 1 << 63, (n, 2), dtype=np.uint64)]
    for label, program, rows in (("mixed", PM.mixed_program(), mixed_rows), ("u64x64", u64, u64_rows)):
        c = PG.ProgramCircuit(program, ctx)
        ni, nw, nc = c.shape()
        a = PG.pack_inputs(c.tape, [p for p, _ in rows], [s for _, s in rows])
        nbytes = n * nw * 32
        d_in, d_w = ctx.to_device(a), ctx.alloc(nbytes)
        d_out, d_st = ctx.alloc(max(1, n * c.layout["output_bytes"])), ctx.alloc(n)

        def launch():
            c.witness_dev(d_in, n, d_w, d_out, d_st)
        launch()
        ctx.synchronize()
        got = d_w.download((2, nw, 4))
        for i in range(2):
            cs = M.ConstraintSystem()
            W.build_program(cs, c.tape, *rows[i])
            assert np.array_equal(got[i], M._to_mont_limbs(cs.witness)), (label, i)
        assert not d_st.download((n,), np.uint8).any()
        # kernels, from the library's events
        ctx.profile_enable(True)
        per = {"program_exec": [], "program_inverse": [], "program_expand": []}
        for _ in range(args.runs):
            ctx.profile_reset()
            launch()
            ctx.synchronize()
            prof = ctx.profile()
            for name in per:
                per[name].append(prof[name]["total_ms"] if name in prof else 0.0)
        ctx.profile_enable(False)
        # the whole call, profiling off
        whole = []
        for _ in range(args.runs):
            ctx.synchronize()
            t0 = time.perf_counter()
            launch()
            ctx.synchronize()
            whole.append((time.perf_counter() - t0) * 1e3)
        s = memset_ms(hip, d_w.ptr, nbytes, args.runs)
        lines.append("%-7s %d instructions, %d witnesses per item, %.3f GB of witnesses per launch" % (label, len(c.tape) // 32 - 1, nw, nbytes / 1e9))
        for name in ("program_exec", "program_inverse", "program_expand"):
            m = stats(per[name])
            lines.append("  %-22s %9.3f ms (min %.3f, max %.3f)%s" % (name, m[0], m[1], m[2], "  %7.1f GB/s of witnesses" % (nbytes / m[0] / 1e6)
                                                                   if name == "program_expand" else ""))
        m, e = stats(whole), stats(per["program_expand"])
        lines.append("  %-22s %9.3f ms (min %.3f, max %.3f)  %8.3f us/item  (host clock, call + synchronise)"
                     % ("swm_program_witness_dev", m[0], m[1], m[2], m[0] * 1e3 / n))
        lines.append("  %-22s %9.3f ms (min %.3f, max %.3f)  %7.1f GB/s;  expand / memset = %.2f,  whole call / memset = %.2f"
                     % ("hipMemsetAsync same bytes", s[0], s[1], s[2], nbytes / s[0] / 1e6, e[0] / s[0], m[0] / s[0]))
        print("\n".join(lines[-6:]), flush=True)
        for b in (d_in, d_w, d_out, d_st):
            b.free()
        if label != "mixed":
            c.free()
            continue
        # swm_program_prove_many against count x swm_program_prove (host clock; keys indexed once)
        cs, _ = W.program_circuit(c.tape, *rows[0])
        packed = cs.pack()
        srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), max(int(mm[0][-1]) for mm in packed.mats),
                                           M.generate_rand())
        pk, _ = M.MarlinInst.index_from_constraint_system(srs, packed)
        srs.free()
        count, reps = 16, 5
        pub, priv = [p for p, _ in rows[:count]], [s for _, s in rows[:count]]
        M.generate_program_proofs(pk, c, pub, priv, M.generate_rand())   # warm-up
        many, single = [], []
        for _ in range(reps):   # alternating, in one process
            t0 = time.perf_counter()
            proofs, _, _ = M.generate_program_proofs(pk, c, pub, priv, M.generate_rand())
            many.append((time.perf_counter() - t0) * 1e3 / count)
            rng = M.generate_rand()
            t0 = time.perf_counter()
            ones = [M.generate_program_proof(pk, c, pub[i], priv[i], rng)[0] for i in range(count)]
            single.append((time.perf_counter() - t0) * 1e3 / count)
            assert ones == proofs
        m, o = stats(many), stats(single)
        lines.append("  prove, %d items, |H| = 2^%d: swm_program_prove_many %8.3f ms/item (min %.3f, max %.3f);  %d x swm_program_prove %8.3f "
                     "ms/item (min %.3f, max %.3f);  %d repetitions, host clock" % (count, (max(nc, ni + nw) - 1).bit_length(), m[0], m[1], m[2],
                                                                                  count, o[0], o[1], o[2], reps))
        print(lines[-1], flush=True)
        pk.free()
        c.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

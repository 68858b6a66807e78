#!/usr/bin/env python3
"""Times the GPU synthesis of the ElGamal encryption witness on both of its paths — a key per item (swm_elgamal_witness_dev) and
one resident key (swm_elgamal_witness_to_dev) — against the Schnorr verification witness it shares its curve half with, and
generate_elgamal_proof against build-then-generate_proof end to end.

    python tools/elgamal_witness_time.py [--runs 9] [--skip-prove] [--out profiles/elgamal_witness_time.txt]

Two steps, each a child process of its own under its own time limit; a step that fails ends the run and nothing more is started.
  kernels  per count (1, 16, 256, 4096 encryptions per launch) and per path: the kernel's time from the library's own HIP events
           around the launch (swm_profile_*), after a warm-up launch, as the median of --runs launches.  In the same process
           swm_schnorr_witness_dev at msg_len 0 for 1 and 256 signatures: the kernel this one was carved from.  Then the three
           ratios DESIGN asks about, each from the medians with the range the minima and maxima allow.
  prove    generate_elgamal_proof (per-item key and resident key) against building the system in Python and generate_proof,
           alternating --runs times on one proving key.
Prints what it measures and writes the same lines to --out.  Needs an MI355X: there is no fallback."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = (1, 16, 256, 4096)
STEP_SECONDS = {"kernels": 240, "prove": 240}


def kernel_ms(ctx, launch, runs, name):
    launch()  # warm-up: code object load, scratch growth
    ctx.synchronize()
    ctx.profile_enable(True)
    out = []
    for _ in range(runs):
        ctx.profile_reset()
        launch()
        ctx.synchronize()
        out.append(ctx.profile()[name]["total_ms"])
    ctx.profile_enable(False)
    return statistics.median(out), min(out), max(out)


def _scalar(tag, i, order):
    return (int.from_bytes(hashlib.sha256(b"%s %d" % (tag, i)).digest(), "little") % order).to_bytes(32, "little")


def _inputs(ctx, EG, params, count):
    """count keys, messages (points of the prime subgroup) and scalars of randomness, made on the GPU from fixed seeds."""
    def scalars(tag):
        return np.frombuffer(b"".join(_scalar(tag, i, EG.GROUP_ORDER) for i in range(count)), dtype=np.uint8).reshape(count, 32)
    pk = ctx.elgamal_keygen(params.h, scalars(b"time secret"))
    msg = ctx.elgamal_keygen(params.h, scalars(b"time message"))
    return pk, msg, scalars(b"time randomness")


def step_kernels(args, say):
    from simpleworks_amd import elgamal as EG, marlin as M, schnorr as SCH, workloads as W
    from simpleworks_amd._lib import DeviceBuffer
    ctx = M.default_context()
    params = EG.Parameters(W.ED_GENERATOR, ctx)
    circuit = EG.ElGamalCircuit(params)
    ni, nw, nc = circuit.shape()
    pk, msg, rs = _inputs(ctx, EG, params, max(COUNTS))
    key0 = EG.ResidentKey(EG.point_from_bytes(pk[0].tobytes()), ctx)
    t0 = time.perf_counter()
    W.elgamal_encryption_circuit(W.ED_GENERATOR, key0.pk, EG.point_from_bytes(msg[0].tobytes()), rs[0].tobytes())
    builder_s = time.perf_counter() - t0
    say("%d witnesses, %d rows; Python builder %.3f s per encryption" % (nw, nc, builder_s))
    t = {}
    for count in COUNTS:
        bufs = [DeviceBuffer(ctx, 64 * count).upload(pk[:count]), DeviceBuffer(ctx, 64 * count).upload(msg[:count]),
                DeviceBuffer(ctx, 32 * count).upload(rs[:count]), DeviceBuffer(ctx, count * nw * 32), DeviceBuffer(ctx, 128 * count),
                DeviceBuffer(ctx, 4 * count + 256)]
        for path, key, name in (("per-item key", None, "elgamal_witness"), ("resident key", key0.h, "elgamal_witness_to")):
            def launch():
                ctx.elgamal_witness_dev(circuit.h, bufs[0], bufs[1], bufs[2], count, bufs[3], bufs[4], bufs[5], key_handle=key)
            t[path, count] = kernel_ms(ctx, launch, args.runs, name)
            assert not bufs[5].download((count,), np.uint32).any(), "an input was refused"
            ct = bufs[4].download((count, 128), np.uint8)
            want = EG.encrypt_many(params, key0 if key else pk[:count], msg[:count], rs[:count])
            assert np.array_equal(ct, want), "the circuit's ciphertexts are not encrypt_many's"
            med, lo, hi = t[path, count]
            say("  %s, count %4d: kernel %.3f ms (min %.3f, max %.3f) = %.4f ms per encryption; builder / GPU per encryption = %.0fx"
                % (path, count, med, lo, hi, med / count, builder_s * 1e3 / (med / count)))
        for b in bufs:
            b.free()
    # the yardstick: the Schnorr verification witness at msg_len 0 (two hash blocks on top of the same curve work)
    sp = SCH.setup(ctx=ctx)
    sc = SCH.SchnorrCircuit(sp, 0)
    snw = sc.shape()[1]
    n = 256
    sk = np.frombuffer(b"".join(_scalar(b"time schnorr secret", i, SCH.GROUP_ORDER) for i in range(n)), dtype=np.uint8).reshape(n, 32)
    k = np.frombuffer(b"".join(_scalar(b"time schnorr nonce", i, SCH.GROUP_ORDER) for i in range(n)), dtype=np.uint8).reshape(n, 32)
    empty = np.zeros((n, 0), dtype=np.uint8)
    spk = ctx.schnorr_keygen(sp.h, sk)
    sig = ctx.schnorr_sign(sp.h, sk, spk, k, empty)
    for count in (1, 256):
        bufs = [DeviceBuffer(ctx, 64 * count).upload(spk[:count]), DeviceBuffer(ctx, 64 * count).upload(sig[:count]),
                DeviceBuffer(ctx, count * snw * 32), DeviceBuffer(ctx, count + 256)]
        t["schnorr", count] = kernel_ms(ctx, lambda: ctx.schnorr_witness_dev(sc.h, bufs[0], None, bufs[1], count, bufs[2], bufs[3]),
                                        args.runs, "schnorr_witness")
        assert bufs[3].download((count,), np.uint8).all(), "a signed message did not verify in the circuit"
        med, lo, hi = t["schnorr", count]
        say("  schnorr_witness, msg_len 0, count %4d: kernel %.3f ms (min %.3f, max %.3f)" % (count, med, lo, hi))
        for b in bufs:
            b.free()

    def ratio(a, b):
        """median / median, with the range min / max .. max / min"""
        return a[0] / b[0], a[1] / b[2], a[2] / b[1]
    say("ratios (median; smallest and largest the minima and maxima allow):")
    say("  1. per-item key / schnorr_witness at one item:      %.2f (%.2f .. %.2f)" % ratio(t["per-item key", 1], t["schnorr", 1]))
    say("  2. per-item key / resident key at one item:         %.2f (%.2f .. %.2f)" % ratio(t["per-item key", 1], t["resident key", 1]))
    say("  3. per-item key / resident key at 4096 items:       %.2f (%.2f .. %.2f)" % ratio(t["per-item key", 4096], t["resident key", 4096]))
    say("     per-item key / resident key at 256 items:        %.2f (%.2f .. %.2f)" % ratio(t["per-item key", 256], t["resident key", 256]))
    say("     per-item key / schnorr_witness at 256 items:     %.2f (%.2f .. %.2f)" % ratio(t["per-item key", 256], t["schnorr", 256]))
    sc.free()
    sp.free()
    key0.free()
    circuit.free()
    params.free()


def step_prove(args, say):
    from simpleworks_amd import elgamal as EG, marlin as M, workloads as W
    ctx = M.default_context()
    params = EG.Parameters(W.ED_GENERATOR, ctx)
    circuit = EG.ElGamalCircuit(params)
    pk, msg, rs = _inputs(ctx, EG, params, 1)
    key_point, msg_point, r = EG.point_from_bytes(pk[0].tobytes()), EG.point_from_bytes(msg[0].tobytes()), rs[0].tobytes()
    resident = EG.ResidentKey(key_point, ctx)
    cs, _ = W.elgamal_encryption_circuit(W.ED_GENERATOR, key_point, msg_point, r)
    packed = cs.pack()
    sizes = (cs.num_constraints, len(cs.instance) + len(cs.witness), max(int(m[0][-1]) for m in packed.mats))
    srs = M.MarlinInst.universal_setup(*sizes, M.generate_rand(), ctx)
    key, _vk = M.MarlinInst.index_from_constraint_system(srs, packed)
    srs.free()

    def by_builder():
        return M.MarlinInst.prove(key, W.ElGamalEncryption(W.ED_GENERATOR, key_point, msg_point, r), M.generate_rand()).data

    def on_gpu():
        return M.generate_elgamal_proof(key, circuit, pk[0].tobytes(), msg[0].tobytes(), r, M.generate_rand())[0]

    def on_gpu_to():
        return M.generate_elgamal_proof(key, circuit, resident, msg[0].tobytes(), r, M.generate_rand())[0]
    assert by_builder() == on_gpu() == on_gpu_to(), "generate_elgamal_proof and build-then-generate_proof disagree"
    host, gpu, gpu_to = [], [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        by_builder()
        t1 = time.perf_counter()
        on_gpu()
        t2 = time.perf_counter()
        on_gpu_to()
        t3 = time.perf_counter()
        host.append(t1 - t0)
        gpu.append(t2 - t1)
        gpu_to.append(t3 - t2)
    say("end to end, %d alternating runs: build + generate_proof %.1f ms (min %.1f, max %.1f), generate_elgamal_proof %.2f ms (min %.2f, "
        "max %.2f), with a ResidentKey %.2f ms (min %.2f, max %.2f), same bytes"
        % (args.runs, statistics.median(host) * 1e3, min(host) * 1e3, max(host) * 1e3, statistics.median(gpu) * 1e3, min(gpu) * 1e3,
           max(gpu) * 1e3, statistics.median(gpu_to) * 1e3, min(gpu_to) * 1e3, max(gpu_to) * 1e3))
    key.free()
    resident.free()
    circuit.free()
    params.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--skip-prove", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elgamal_witness_time.txt"))
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), help="run one step in this process (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        {"kernels": step_kernels, "prove": step_prove}[args.step](args, lambda text: print(text, flush=True))
        return 0
    lines = []
    for step in ("kernels",) + (() if args.skip_prove else ("prove",)):
        try:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--runs", str(args.runs), "--step", step],
                                 stdout=subprocess.PIPE, text=True, timeout=STEP_SECONDS[step])
        except subprocess.TimeoutExpired:
            print("step %s ran past its %d s: stopping" % (step, STEP_SECONDS[step]), file=sys.stderr)
            return 124
        sys.stdout.write(run.stdout)
        sys.stdout.flush()
        if run.returncode != 0:
            print("step %s ended with status %d: stopping" % (step, run.returncode), file=sys.stderr)
            return run.returncode if run.returncode > 0 else 1
        lines += run.stdout.splitlines()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

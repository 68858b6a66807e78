#!/usr/bin/env python3
"""Times the Poseidon hash circuit's witness synthesis (swm_poseidon_witness_dev, bytes form) next to the native hash of the same
inputs (swm_poseidon_hash_bytes_dev), with the reference's parameter set (tests/golden/poseidon_params.json).

    python tools/poseidon_witness_time.py [--runs 15] [--out profiles/poseidon_witness_time.txt] [--no-long]

Per shape — 2^10, 2^14 and 2^16 inputs of 11 bytes (one permutation, 353 witnesses) and of 55 bytes (two permutations, 970
witnesses) — the kernel's time from the library's own HIP events around the launch (swm_profile_*), after a warm-up launch, as the
median of --runs launches, for both kernels, and their ratio.  Then, once, ONE input of 65536 bytes: a serial chain of about 630 000
products on one lane, which the GPU form is not for.  There is no threshold: the figures go to the output file.  Needs an MI355X:
there is no fallback."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_ms(ctx, name, launch, runs, warm=True):
    if warm:
        launch()  # warm-up: code object load
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseidon_witness_time.txt"))
    ap.add_argument("--no-long", action="store_true", help="skip the single 65536-byte input")
    args = ap.parse_args()
    assert args.runs >= 10, "median of at least 10 runs"
    from simpleworks_amd import hash as H
    from simpleworks_amd.marlin import default_context

    ctx = default_context()
    sponge = H.PoseidonSponge(H.PoseidonParameters.from_json(os.path.join(ROOT, "tests", "golden", "poseidon_params.json")), ctx)
    lines = ["Poseidon hash circuit witness (bytes form) next to the native hash, reference parameters (8 + 29 rounds, alpha 17), one "
             "MI355X; kernel time between HIP events, median of %d launches after a warm-up" % args.runs]
    rnd = np.random.default_rng(1)
    for length in (11, 55):
        circuit = H.PoseidonCircuit(sponge, input_len=length)
        nw = circuit.shape()[1]
        for log_n in (10, 14, 16):
            n = 1 << log_n
            msgs = rnd.integers(0, 256, (n, length), dtype=np.uint8)
            d_msgs, d_w, d_out = ctx.alloc(msgs.nbytes).upload(msgs), ctx.alloc(n * nw * 32), ctx.alloc(32 * n)
            w_med, w_lo, w_hi = kernel_ms(ctx, "poseidon_witness_bytes", lambda: ctx.poseidon_witness_dev(circuit.h, d_msgs, n, d_w, d_out, None),
                                          args.runs)
            h_med, h_lo, h_hi = kernel_ms(ctx, "poseidon_hash_bytes", lambda: ctx.poseidon_hash_bytes_dev(sponge.h, d_msgs, length, n, d_out),
                                          args.runs)
            lines.append("%2d bytes x 2^%-2d  witness %9.3f ms (min %.3f, max %.3f; %6.1f MB)   hash %8.3f ms (min %.3f, max %.3f)   ratio %5.2f"
                         % (length, log_n, w_med, w_lo, w_hi, n * nw * 32 / 1e6, h_med, h_lo, h_hi, w_med / h_med))
            print(lines[-1], flush=True)
            for b in (d_msgs, d_w, d_out):
                b.free()
        circuit.free()
    if not args.no_long:
        length = 65536
        circuit = H.PoseidonCircuit(sponge, input_len=length)
        nw = circuit.shape()[1]
        msg = rnd.integers(0, 256, (1, length), dtype=np.uint8)
        d_msg, d_w, d_out = ctx.alloc(msg.nbytes).upload(msg), ctx.alloc(nw * 32), ctx.alloc(32)
        w_ms = kernel_ms(ctx, "poseidon_witness_bytes", lambda: ctx.poseidon_witness_dev(circuit.h, d_msg, 1, d_w, d_out, None), 1, warm=False)[0]
        h_ms = kernel_ms(ctx, "poseidon_hash_bytes", lambda: ctx.poseidon_hash_bytes_dev(sponge.h, d_msg, length, 1, d_out), 1, warm=False)[0]
        lines.append("one input of 65536 bytes (1058 permutations, %d witnesses), measured once: witness %.1f ms, hash %.1f ms" % (nw, w_ms, h_ms))
        print(lines[-1], flush=True)
        for b in (d_msg, d_w, d_out):
            b.free()
        circuit.free()
    sponge.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the Poseidon sponge's device forms (swm_poseidon_hash_fr_dev, swm_poseidon_hash_bytes_dev) with the reference's
parameter set (tests/golden/poseidon_params.json).

    python tools/poseidon_time.py [--runs 11] [--out profiles/poseidon_time.txt]

Per shape — 2^10, 2^16 and 2^20 two-to-one compressions (two elements in, one out: one permutation each) and as many 64-byte
inputs (three elements: two permutations each) — the kernel's time from the library's own HIP events around the launch
(swm_profile_*), after a warm-up launch, as the median of --runs launches, and the hashes and permutations per second that makes.
There is no threshold: the figures go to the output file.  Needs an MI355X: there is no fallback."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_ms(ctx, name, launch, runs):
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
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseidon_time.txt"))
    args = ap.parse_args()
    assert args.runs >= 10, "median of at least 10 runs"
    from simpleworks_amd import hash as H
    from simpleworks_amd.marlin import R_MODULUS, default_context

    ctx = default_context()
    sponge = H.PoseidonSponge(H.PoseidonParameters.from_json(os.path.join(ROOT, "tests", "golden", "poseidon_params.json")), ctx)
    lines = ["Poseidon sponge, reference parameters (8 + 29 rounds, alpha 17), one MI355X; kernel time between HIP events, median of %d "
             "launches after a warm-up" % args.runs]
    rnd = np.random.default_rng(1)
    for log_n in (10, 16, 20):
        n = 1 << log_n
        elems = rnd.integers(0, 256, (n, 2, 32), dtype=np.uint8)
        elems[:, :, 31] &= 0x0F      # < 2^252 < r: canonical
        assert int.from_bytes(elems[0, 0].tobytes(), "little") < R_MODULUS
        msgs = rnd.integers(0, 256, (n, 64), dtype=np.uint8)
        d_elems, d_msgs, d_out = ctx.alloc(elems.nbytes).upload(elems), ctx.alloc(msgs.nbytes).upload(msgs), ctx.alloc(32 * n)
        shapes = (("two-to-one (n_in = 2, n_out = 1)", 1, "poseidon_hash_fr",
                   lambda: ctx.poseidon_hash_fr_dev(sponge.h, d_elems, 2, n, 1, d_out, None)),
                  ("64-byte inputs", 2, "poseidon_hash_bytes", lambda: ctx.poseidon_hash_bytes_dev(sponge.h, d_msgs, 64, n, d_out)))
        for what, perms, name, launch in shapes:
            med, lo, hi = kernel_ms(ctx, name, launch, args.runs)
            lines.append("2^%-2d %-33s %9.3f ms (min %.3f, max %.3f)  %8.2f M hashes/s  %8.2f M permutations/s"
                         % (log_n, what, med, lo, hi, n / med / 1e3, perms * n / med / 1e3))
            print(lines[-1], flush=True)
        for b in (d_elems, d_msgs, d_out):
            b.free()
    sponge.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

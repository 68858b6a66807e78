"""Schnorr signatures per second on the GPU: sign_many and verify_many of simpleworks_amd/schnorr.py at 2^10, 2^14 and 2^18
signatures of 32-byte messages.  Writes profiles/schnorr_rate.json (or --out) and prints it as one JSON line.
usage: schnorr_rate.py [--reps 7] [--warmup 2] [--logs 10,14,18] [--out profiles/schnorr_rate.json]

Per size and per operation, after `warmup` untimed runs, `reps` timed ones, each reported two ways:
  kernel_ms   the kernel alone, between the HIP events the library records around its launch (swm_profile_*)
  call_ms     the whole call on a host clock: host arrays in, staging copies, kernel, results out; it ends in a device synchronise
as median, minimum and maximum; the rates are counts over the medians.  Keys, nonces and messages are seeded; every signature
made here must verify, and a run without a GPU fails.  There is no parent path and no buildable reference to compare with:
the file is a record, not a pass / fail check."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
from simpleworks_amd import marlin as M, schnorr as SCH


def canonical_scalars(gen, n):
    a = gen.integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 31] &= 0x03          # < 2^250 < l
    return a


def timed(ctx, kernel, reps, warmup, call):
    for _ in range(warmup):
        call()
    kernel_ms, call_ms = [], []
    for _ in range(reps):
        ctx.profile_reset()
        t0 = time.perf_counter()
        call()
        call_ms.append((time.perf_counter() - t0) * 1e3)
        kernel_ms.append(ctx.profile()[kernel]["total_ms"])
    return kernel_ms, call_ms


def summary(n, ms):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "per_s": n / (med * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--logs", default="10,14,18")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schnorr_rate.json"))
    args = ap.parse_args()
    assert args.reps >= 5
    ctx = M.default_context()
    params = SCH.setup()
    gen = np.random.default_rng(2024)
    ctx.profile_enable(True)
    rows = []
    for lg in (int(v) for v in args.logs.split(",")):
        n = 1 << lg
        sk, k = canonical_scalars(gen, n), canonical_scalars(gen, n)
        msgs = gen.integers(0, 256, size=(n, 32), dtype=np.uint8)
        pk = ctx.schnorr_keygen(params.h, sk)
        sig = SCH.sign_many(params, sk, pk, msgs, nonces=k)
        assert SCH.verify_many(params, pk, msgs, sig).all(), "a signature made here did not verify"
        row = {"signatures": n, "message_bytes": 32}
        for name, kernel, call in (("sign", "schnorr_sign", lambda: SCH.sign_many(params, sk, pk, msgs, nonces=k)),
                                   ("verify", "schnorr_verify", lambda: SCH.verify_many(params, pk, msgs, sig))):
            kernel_ms, call_ms = timed(ctx, kernel, args.reps, args.warmup, call)
            row[name] = {"kernel": summary(n, kernel_ms), "call": summary(n, call_ms)}
        rows.append(row)
    out = {"workload": "Schnorr on ed-on-BLS12-377: sign_many / verify_many, 32-byte messages, no salt", "reps": args.reps,
           "warmup": args.warmup, "sizes": rows}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

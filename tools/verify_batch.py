"""Batch verification timing: one JSON line per batch size.

    python tools/verify_batch.py [--counts 1,16,256,1024,4096] [--reps 3]

For each count: the wall time of swm_verify_proofs_batch on `count` proofs of the 2^10-row synthetic circuit (median of
--reps), ms per proof, and for count <= 256 the per-proof time of a plain swm_verify_proof loop over the same proofs in the
same run.  SWM_TRACE=1 adds the per-stage breakdown of each batch on stderr."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,16,256,1024,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log-n", type=int, default=10)
    args = ap.parse_args()
    from simpleworks_amd import marlin as M, workloads as W
    counts = [int(c) for c in args.counts.split(",")]
    n = 1 << args.log_n
    rng = M.generate_rand()
    srs = M.generate_universal_srs(n, n, n, rng)
    cases = [W.synthetic_r1cs(n, 0x100 + i, 0x200 + 3 * i) for i in range(8)]
    pk, vk = M.generate_proving_and_verifying_keys(srs, cases[0][0])
    distinct = [M.generate_proof(cases[k % 8][0], pk, rng) for k in range(64)]
    publics_all = [list(cases[k % 8][1]) for k in range(64)]
    M.verify_proofs(vk, publics_all[:16], distinct[:16], M.generate_rand())  # warm-up: pool, kernels, scratch
    for count in counts:
        proofs = [distinct[k % 64] for k in range(count)]
        publics = [publics_all[k % 64] for k in range(count)]
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ok = M.verify_proofs(vk, publics, proofs, M.generate_rand())
            times.append((time.perf_counter() - t0) * 1e3)
            assert ok, "batch rejected honest proofs"
        times.sort()
        wall = times[len(times) // 2]
        line = {"count": count, "batch_ms": round(wall, 3), "ms_per_proof": round(wall / count, 4)}
        if count <= 256:
            r = M.generate_rand()
            t0 = time.perf_counter()
            for pr, pub in zip(proofs, publics):
                assert M.verify_proof(vk, pub, pr, r)
            line["loop_ms_per_proof"] = round((time.perf_counter() - t0) * 1e3 / count, 4)
        print(json.dumps(line), flush=True)
    pk.free()
    srs.free()


if __name__ == "__main__":
    main()

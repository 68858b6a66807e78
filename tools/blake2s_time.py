#!/usr/bin/env python3
"""Times the Blake2s random oracle's two kernels (swm_blake2s_hash_dev, swm_blake2s_witness_dev) and, in the same process, Schnorr
verification at msg_len = 10 (swm_schnorr_verify) for scale and a hipMemsetAsync of the witness kernel's byte count: the store
rate the machine grants.

    python tools/blake2s_time.py [--runs 15] [--out profiles/blake2s_time.txt]

Native hash: 2^20 items of 32, 64 and 65 bytes (one block, one full block, two blocks with every item off a word boundary) on a
device buffer, as hashes per second.  Witness: 2^10 and 2^12 items of 32 bytes (0.71 and 2.85 GB written) into a device buffer,
beside a hipMemsetAsync of the same buffer, and the ratio of the two.  Kernel time is taken from the library's own HIP events
around its launches (swm_profile_*), the memset's from two HIP events on the stream it runs on; each figure is the median,
minimum and maximum of --runs launches after a warm-up.  The first items of every timed output are compared with hashlib and with
the host form first: what is timed is also right.  There is no threshold: the figures go to the output file.  Needs an MI355X:
there is no fallback."""
import argparse
import ctypes
import hashlib
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_ms(ctx, name, launch, runs):
    launch()  # warm-up: code object load, scratch buffers
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


def memset_ms(hip, ptr, nbytes, runs):
    """hipMemsetAsync on the null stream between two events."""
    def check(rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: hipError %d" % (what, rc))
    start, stop = ctypes.c_void_p(), ctypes.c_void_p()
    check(hip.hipEventCreate(ctypes.byref(start)), "hipEventCreate")
    check(hip.hipEventCreate(ctypes.byref(stop)), "hipEventCreate")
    out = []
    for i in range(runs + 1):  # the first is the warm-up
        check(hip.hipEventRecord(start, None), "hipEventRecord")
        check(hip.hipMemsetAsync(ctypes.c_void_p(ptr), 0, ctypes.c_size_t(nbytes), None), "hipMemsetAsync")
        check(hip.hipEventRecord(stop, None), "hipEventRecord")
        check(hip.hipEventSynchronize(stop), "hipEventSynchronize")
        ms = ctypes.c_float(0)
        check(hip.hipEventElapsedTime(ctypes.byref(ms), start, stop), "hipEventElapsedTime")
        if i:
            out.append(ms.value)
    hip.hipEventDestroy(start)
    hip.hipEventDestroy(stop)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blake2s_time.txt"))
    args = ap.parse_args()
    assert args.runs >= 15, "median of at least 15 launches"
    from simpleworks_amd import _lib, random_oracle as RO, schnorr as SCH
    from simpleworks_amd.marlin import default_context

    ctx = default_context()
    hip = ctypes.CDLL("libamdhip64.so")   # the runtime the library already runs on
    lines = ["Blake2s random oracle, one MI355X, library %s; kernel time between HIP events, median (min, max) of %d launches after a "
             "warm-up" % (os.path.basename(_lib.LIB_PATH), args.runs)]
    rnd = np.random.default_rng(1)

    # ---- native hash, and Schnorr verification for scale
    n = 1 << 20
    for length in (32, 64, 65):
        a = rnd.integers(0, 256, (n, length), dtype=np.uint8)
        d_in, d_out = ctx.to_device(a), ctx.alloc(32 * n)
        ctx.blake2s_hash_dev(d_in, length, n, d_out)
        ctx.synchronize()
        got = d_out.download((n, 32), np.uint8)
        for i in (0, 1, 2, 3, n - 1):
            assert got[i].tobytes() == hashlib.blake2s(a[i].tobytes()).digest(), (length, i)
        m = kernel_ms(ctx, "blake2s_hash", lambda: ctx.blake2s_hash_dev(d_in, length, n, d_out), args.runs)
        lines.append("2^20 blake2s_hash     %4d bytes %9.3f ms (min %.3f, max %.3f)  %8.2f ns/item  %9.1f M hashes/s  %7.1f GB/s of input"
                     % (length, m[0], m[1], m[2], m[0] * 1e6 / n, n / m[0] / 1e3, n * length / m[0] / 1e6))
        print(lines[-1], flush=True)
        d_in.free()
        d_out.free()
    sch = SCH.Parameters(ctx=ctx)
    sk = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
    sk[:, 31] &= 0x03       # < 2^250 < l: canonical
    pk = ctx.schnorr_keygen(sch.h, sk)
    sig = np.concatenate([sk[::-1], rnd.integers(0, 256, (n, 32), dtype=np.uint8)], axis=1)   # random: they do not verify, which costs the same
    text = rnd.integers(0, 256, (n, 10), dtype=np.uint8)
    m = kernel_ms(ctx, "schnorr_verify", lambda: ctx.schnorr_verify(sch.h, pk, text, sig), args.runs)
    lines.append("2^20 schnorr_verify   msg_len 10 %9.3f ms (min %.3f, max %.3f)  %8.2f ns/item  %9.3f M items/s   (for scale)"
                 % (m[0], m[1], m[2], m[0] * 1e6 / n, n / m[0] / 1e3))
    print(lines[-1], flush=True)
    sch.free()

    # ---- witness against hipMemsetAsync of the same bytes
    circuit = RO.Blake2sCircuit(32, ctx)
    nw = circuit.shape()[1]
    for log_n in (10, 12):
        n = 1 << log_n
        a = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
        nbytes = n * nw * 32
        d_in, d_w, d_dg = ctx.to_device(a), ctx.alloc(nbytes), ctx.alloc(32 * n)
        ctx.blake2s_witness_dev(d_in, 32, n, d_w, d_dg)
        ctx.synchronize()
        want, _ = circuit.witness_many(a[:2])
        assert np.array_equal(d_w.download((2, nw, 4)), want)
        assert np.array_equal(d_dg.download((n, 32), np.uint8)[-1], np.frombuffer(hashlib.blake2s(a[-1].tobytes()).digest(), dtype=np.uint8))
        w = kernel_ms(ctx, "blake2s_witness", lambda: ctx.blake2s_witness_dev(d_in, 32, n, d_w, d_dg), args.runs)
        ctx.synchronize()
        s = memset_ms(hip, d_w.ptr, nbytes, args.runs)
        lines.append("2^%-2d blake2s_witness  32 bytes   %9.3f ms (min %.3f, max %.3f)  %8.3f us/item  %.3f GB written  %7.1f GB/s"
                     % (log_n, w[0], w[1], w[2], w[0] * 1e3 / n, nbytes / 1e9, nbytes / w[0] / 1e6))
        lines.append("2^%-2d hipMemsetAsync   same bytes %9.3f ms (min %.3f, max %.3f)  %7.1f GB/s;  witness / memset = %.2f"
                     % (log_n, s[0], s[1], s[2], nbytes / s[0] / 1e6, w[0] / s[0]))
        print("\n".join(lines[-2:]), flush=True)
        for b in (d_in, d_w, d_dg):
            b.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

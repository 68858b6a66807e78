#!/usr/bin/env python3
"""Times the four ElGamal kernels (swm_elgamal_keygen, _encrypt, _encrypt_to, _decrypt) and, in the same process, Schnorr
verification at msg_len = 10 (swm_schnorr_verify), the kernel with the same two scalar multiplications.

    python tools/elgamal_time.py [--runs 11] [--out profiles/elgamal_time.txt]

Per size — 2^10, 2^16 and 2^20 items — the kernel's time from the library's own HIP events around its launches (swm_profile_*;
the ladder's kernels run 2^18 items per launch and the launches are summed), after a warm-up call, as the median, minimum and
maximum of --runs calls.  Scalars are random below the group order; public keys, messages and the first halves of the ciphertexts
are random points of the prime subgroup (made by swm_elgamal_keygen), so every lane does the full work; the Schnorr signatures
are random too: they do not verify, which costs the same.  Then the ratios DESIGN §3.5b records.  There is no threshold: the
figures go to the output file.  (SWM_LIB_PATH selects another build of the library for an A/B.)  Needs an MI355X: there is no
fallback."""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elgamal_time.txt"))
    args = ap.parse_args()
    assert args.runs >= 11, "median of at least 11 runs"
    from simpleworks_amd import _lib, elgamal as EG, schnorr as SCH
    from simpleworks_amd.marlin import default_context, generate_rand

    ctx = default_context()
    params = EG.setup(generate_rand(), ctx)
    sch = SCH.Parameters(ctx=ctx)
    lines = ["ElGamal on ed-on-BLS12-377 and Schnorr verification (msg_len 10), one MI355X, library %s; kernel time between HIP events, "
             "median (min, max) of %d calls after a warm-up" % (os.path.basename(_lib.LIB_PATH), args.runs)]
    rnd = np.random.default_rng(1)
    med = {}
    for log_n in (10, 16, 20):
        n = 1 << log_n

        def scalars():
            s = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
            s[:, 31] &= 0x03       # < 2^250 < l: canonical
            return s
        sk, r = scalars(), scalars()
        pk = ctx.elgamal_keygen(params.h, sk)
        msg = ctx.elgamal_keygen(params.h, scalars())
        key = EG.ResidentKey(EG.point_from_bytes(pk[0].tobytes()), ctx)
        ct = ctx.elgamal_encrypt(params.h, pk, msg, r)
        assert np.array_equal(ctx.elgamal_decrypt(sk, ct), msg)                       # what is timed is also right
        assert np.array_equal(ctx.elgamal_encrypt_to(params.h, key.h, msg[:64], r[:64]),
                              ctx.elgamal_encrypt(params.h, np.ascontiguousarray(np.broadcast_to(pk[0], (64, 64))), msg[:64], r[:64]))
        sig = np.concatenate([scalars(), rnd.integers(0, 256, (n, 32), dtype=np.uint8)], axis=1)
        text = rnd.integers(0, 256, (n, 10), dtype=np.uint8)
        out64, out128 = np.empty((n, 64), dtype=np.uint8), np.empty((n, 128), dtype=np.uint8)
        shapes = (("elgamal_keygen", lambda: ctx.elgamal_keygen(params.h, sk, out=out64)),
                  ("elgamal_encrypt", lambda: ctx.elgamal_encrypt(params.h, pk, msg, r, out=out128)),
                  ("elgamal_encrypt_to", lambda: ctx.elgamal_encrypt_to(params.h, key.h, msg, r, out=out128)),
                  ("elgamal_decrypt", lambda: ctx.elgamal_decrypt(sk, ct, out=out64)),
                  ("schnorr_verify", lambda: ctx.schnorr_verify(sch.h, pk, text, sig)))
        for name, launch in shapes:
            med[name, log_n] = m = kernel_ms(ctx, name, launch, args.runs)
            lines.append("2^%-2d %-19s %10.3f ms (min %.3f, max %.3f)  %9.1f ns/item  %8.3f M items/s"
                         % (log_n, name, m[0], m[1], m[2], m[0] * 1e6 / n, n / m[0] / 1e3))
            print(lines[-1], flush=True)
        key.free()
    enc, ver = med["elgamal_encrypt", 16], med["schnorr_verify", 16]
    lines.append("ratio 1: elgamal_encrypt / schnorr_verify per item at 2^16 = %.3f (encrypt median %.3f ms; schnorr_verify median %.3f, "
                 "min %.3f, max %.3f ms: encrypt's median is %s schnorr_verify's max)"
                 % (enc[0] / ver[0], enc[0], ver[0], ver[1], ver[2], "above" if enc[0] > ver[2] else "not above"))
    for log_n in (16, 20):
        lines.append("ratio 2: elgamal_encrypt / elgamal_encrypt_to at 2^%d = %.2f (what the resident key buys)"
                     % (log_n, med["elgamal_encrypt", log_n][0] / med["elgamal_encrypt_to", log_n][0]))
    for line in lines[-3:]:
        print(line, flush=True)
    sch.free()
    params.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

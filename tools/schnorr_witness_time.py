#!/usr/bin/env python3
"""Times the GPU synthesis of the Schnorr verification witness (swm_schnorr_witness_dev) against the Python builder it replaces
(workloads.build_schnorr_verification), and generate_schnorr_proof against build-then-generate_proof end to end.

    python tools/schnorr_witness_time.py [--msg-len 24] [--runs 9] [--skip-prove] [--out profiles/schnorr_witness_time.txt]

Per count (1, 16, 256 signatures per launch): the kernel's time from the library's own HIP events around the launch
(swm_profile_*), after a warm-up launch, as the median of --runs launches, and that divided by count.  The builder's time is a
host clock around one call on this host.  One signature at message lengths that give 2, 3 and 4 hash blocks separates the
per-block cost of Blake2s from the curve arithmetic.  The end-to-end pair alternates the two ways --runs times on one key and
reports both medians.  Prints what it measures and writes the same lines to --out.  Needs an MI355X: there is no fallback."""
import argparse
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_ms(ctx, launch, runs):
    launch()  # warm-up: code object load, scratch growth
    ctx.synchronize()
    ctx.profile_enable(True)
    out = []
    for _ in range(runs):
        ctx.profile_reset()
        launch()
        ctx.synchronize()
        out.append(ctx.profile()["schnorr_witness"]["total_ms"])
    ctx.profile_enable(False)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msg-len", type=int, default=24)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--skip-prove", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schnorr_witness_time.txt"))
    args = ap.parse_args()
    from simpleworks_amd import marlin as M, schnorr as SCH, workloads as W
    from simpleworks_amd._lib import DeviceBuffer

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    ctx = M.default_context()
    params = SCH.setup(ctx=ctx)

    def signed(msg_len, count):
        """count keys, messages of msg_len bytes and their signatures, made on the GPU from fixed seeds."""
        sk = np.frombuffer(b"".join((int.from_bytes(hashlib.sha256(b"time secret %d" % i).digest(), "little") % SCH.GROUP_ORDER)
                                    .to_bytes(32, "little") for i in range(count)), dtype=np.uint8).reshape(count, 32)
        k = np.frombuffer(b"".join((int.from_bytes(hashlib.sha256(b"time nonce %d" % i).digest(), "little") % SCH.GROUP_ORDER)
                                   .to_bytes(32, "little") for i in range(count)), dtype=np.uint8).reshape(count, 32)
        msgs = np.frombuffer(hashlib.shake_128(b"time messages").digest(max(1, msg_len * count)), dtype=np.uint8)[:msg_len * count]
        msgs = msgs.reshape(count, msg_len)
        pk = ctx.schnorr_keygen(params.h, sk)
        sig = ctx.schnorr_sign(params.h, sk, pk, k, msgs)
        assert SCH.verify_many(params, pk, msgs, sig).all()
        return pk, msgs, sig

    def launch_for(circuit, pk, msgs, sig):
        count, nw = pk.shape[0], circuit.shape()[1]
        bufs = [DeviceBuffer(ctx, pk.nbytes).upload(pk), DeviceBuffer(ctx, msgs.nbytes).upload(msgs) if msgs.size else None,
                DeviceBuffer(ctx, sig.nbytes).upload(sig), DeviceBuffer(ctx, count * nw * 32), DeviceBuffer(ctx, count + 256)]
        return bufs, lambda: ctx.schnorr_witness_dev(circuit.h, bufs[0], bufs[1], bufs[2], count, bufs[3], bufs[4])

    circuit = SCH.SchnorrCircuit(params, args.msg_len)
    ni, nw, nc = circuit.shape()
    pk, msgs, sig = signed(args.msg_len, 256)
    point = SCH.point_from_bytes(pk[0].tobytes())
    t0 = time.perf_counter()
    cs, _ = W.schnorr_verification_circuit(W.ED_GENERATOR, None, point, msgs[0].tobytes(), sig[0].tobytes())
    builder_s = time.perf_counter() - t0
    say("msg_len %d, no salt: %d witnesses, %d rows; Python builder %.3f s per signature" % (args.msg_len, nw, nc, builder_s))
    for count in (1, 16, 256):
        bufs, launch = launch_for(circuit, pk[:count], msgs[:count], sig[:count])
        med, lo, hi = kernel_ms(ctx, launch, args.runs)
        assert bufs[4].download((count,), np.uint8).all(), "a signed message did not verify in the circuit"
        say("  count %3d: kernel %.3f ms (min %.3f, max %.3f) = %.3f ms per signature; builder / GPU per signature = %.0fx"
            % (count, med, lo, hi, med / count, builder_s * 1e3 / (med / count)))
        for b in bufs:
            if b is not None:
                b.free()
    # where one signature's time goes: the hash is sequential on one lane, a fixed cost per 64-byte block
    one = {}
    for msg_len in (0, 64, 128):
        c = SCH.SchnorrCircuit(params, msg_len)
        a, m, s = signed(msg_len, 1)
        bufs, launch = launch_for(c, a, m, s)
        one[msg_len] = kernel_ms(ctx, launch, args.runs)[0]
        for b in bufs:
            if b is not None:
                b.free()
        c.free()
    per_block = (one[128] - one[0]) / 2
    say("one signature: 2 blocks %.3f ms, 3 blocks %.3f ms, 4 blocks %.3f ms: %.3f ms per hash block, %.3f ms for the curve arithmetic, "
        "the decompositions and the launch" % (one[0], one[64], one[128], per_block, one[0] - 2 * per_block))
    if not args.skip_prove:
        packed = cs.pack()
        sizes = (cs.num_constraints, len(cs.instance) + len(cs.witness), max(int(m[0][-1]) for m in packed.mats))
        srs = M.MarlinInst.universal_setup(*sizes, M.generate_rand(), ctx)
        key, _vk = M.MarlinInst.index_from_constraint_system(srs, packed)
        srs.free()
        message, signature, key_bytes = msgs[0].tobytes(), sig[0].tobytes(), pk[0].tobytes()

        def by_builder():
            circuit_obj = W.SimpleSchnorrSignatureVerification(W.ED_GENERATOR, None, point, message, signature)
            return M.MarlinInst.prove(key, circuit_obj, M.generate_rand()).data

        def on_gpu():
            return M.generate_schnorr_proof(key, circuit, key_bytes, message, signature, M.generate_rand())
        assert by_builder() == on_gpu(), "generate_schnorr_proof and build-then-generate_proof disagree"
        host, gpu = [], []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            by_builder()
            t1 = time.perf_counter()
            on_gpu()
            t2 = time.perf_counter()
            host.append(t1 - t0)
            gpu.append(t2 - t1)
        say("end to end, msg_len %d, %d alternating runs: build + generate_proof %.1f ms (min %.1f), generate_schnorr_proof %.2f ms (min %.2f), "
            "same bytes" % (args.msg_len, args.runs, statistics.median(host) * 1e3, min(host) * 1e3, statistics.median(gpu) * 1e3, min(gpu) * 1e3))
        key.free()
    circuit.free()
    params.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

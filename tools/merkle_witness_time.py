#!/usr/bin/env python3
"""Times the GPU synthesis of the Merkle-membership witness (swm_merkle_witness_dev) against the Python builder it replaces
(workloads.build_merkle_membership), and SimpleMerkleTree.prove_on_gpu against SimpleMerkleTree.prove end to end.

    python tools/merkle_witness_time.py [--height 19] [--runs 9] [--skip-prove]

Per (gadget_byte_ops, count): the kernel's time from the library's own HIP events around the launch (swm_profile_*), after a
warm-up launch, as the median of --runs launches, and that divided by count.  The builder's time is a host clock around one
call on this host.  The end-to-end pair alternates prove / prove_on_gpu --runs times on one tree and reports both medians.
Needs an MI355X: there is no fallback."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_ms(ctx, launch, runs):
    launch()  # warm-up: code object load, scratch growth
    ctx.synchronize()
    ctx.profile_enable(True)
    out = []
    for _ in range(runs):
        ctx.profile_reset()
        launch()
        ctx.synchronize()
        out.append(ctx.profile()["merkle_witness"]["total_ms"])
    ctx.profile_enable(False)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=19)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--skip-prove", action="store_true")
    args = ap.parse_args()
    from simpleworks_amd import marlin as M, workloads as W
    from simpleworks_amd._lib import DeviceBuffer
    from simpleworks_amd.hash import MerkleCircuit

    ctx = M.default_context()
    params = W.MerkleParams()
    leaf_crh, inner_crh = params.crh(ctx)
    levels = args.height - 1
    g = W._SplitMix(7)
    for ops in (0, 2400):
        circuit = MerkleCircuit(leaf_crh, inner_crh, args.height, ops)
        nw = circuit.shape()[1]
        siblings = [g.fr() for _ in range(levels)]
        t0 = time.perf_counter()
        cs = M.ConstraintSystem()
        W.build_merkle_membership(cs, params, 0xA7, 5, siblings, gadget_byte_ops=ops)
        builder_s = time.perf_counter() - t0
        print("height %d ops %4d: %d witnesses; Python builder %.3f s per path" % (args.height, ops, nw, builder_s), flush=True)
        for count in (1, 16, 256):
            rnd = np.random.default_rng(count)
            sib = np.frombuffer(b"".join(g.fr().to_bytes(32, "little") for _ in range(count * levels)), dtype=np.uint8)
            bufs = [DeviceBuffer(ctx, count + 256).upload(rnd.integers(0, 256, count, dtype=np.uint8)),
                    DeviceBuffer(ctx, 8 * count).upload(rnd.integers(0, 1 << levels, count, dtype=np.uint64)),
                    DeviceBuffer(ctx, sib.nbytes).upload(sib), DeviceBuffer(ctx, count * nw * 32)]
            med, lo, hi = kernel_ms(ctx, lambda: ctx.merkle_witness_dev(circuit.h, bufs[0], bufs[1], bufs[2], count, bufs[3]), args.runs)
            print("  count %3d: kernel %.3f ms (min %.3f, max %.3f) = %.3f ms per path; builder / GPU per path = %.0fx"
                  % (count, med, lo, hi, med / count, builder_s * 1e3 / (med / count)), flush=True)
            for b in bufs:
                b.free()
        circuit.free()
    # where one path's time goes: the levels are sequential (a fixed cost per level), and a launch only gets faster per path
    # once every CU has a workgroup — one path per workgroup, two waves each
    one = {}
    for height in (2, args.height):
        circuit = MerkleCircuit(leaf_crh, inner_crh, height, 0)
        for count in ((1,) if height == 2 else (1, 1024, 4096)):
            sib = np.frombuffer(b"".join(g.fr().to_bytes(32, "little") for _ in range(height - 1)) * count, dtype=np.uint8)
            bufs = [DeviceBuffer(ctx, count + 256).upload(np.full(count, 0xA7, dtype=np.uint8)),
                    DeviceBuffer(ctx, 8 * count).upload(np.zeros(count, dtype=np.uint64)),
                    DeviceBuffer(ctx, sib.nbytes).upload(sib), DeviceBuffer(ctx, count * circuit.shape()[1] * 32)]
            one[height, count] = kernel_ms(ctx, lambda: ctx.merkle_witness_dev(circuit.h, bufs[0], bufs[1], bufs[2], count, bufs[3]), args.runs)[0]
            for b in bufs:
                b.free()
        circuit.free()
    per_level = (one[args.height, 1] - one[2, 1]) / (args.height - 2)
    print("one path, no byte operations: height 2 %.3f ms, height %d %.3f ms: %.3f ms per level, %.3f ms for the leaf hash, launch and first level"
          % (one[2, 1], args.height, one[args.height, 1], per_level, one[2, 1]))
    for count in (1024, 4096):
        print("  count %4d: kernel %.3f ms = %.4f ms per path" % (count, one[args.height, count], one[args.height, count] / count))
    if args.skip_prove:
        return
    # end to end on one tree of 2^(height-1) leaves, the universal SRS sized for the circuit
    ops = 2400
    n = 1 << levels
    leaves = [(37 * i + 11) & 0xFF for i in range(n)]
    cs = M.ConstraintSystem()
    W.build_merkle_membership(cs, params, 0, 0, [0] * levels, gadget_byte_ops=ops)
    packed = cs.pack()
    sizes = (cs.num_constraints, len(cs.instance) + len(cs.witness), max(int(m[0][-1]) for m in packed.mats))
    tree = W.SimpleMerkleTree(leaves, params=params, srs_sizes=sizes, gadget_byte_ops=ops, ctx=ctx)
    idx = 123457 % n
    path = tree.get_merkle_path(idx)
    ref = tree.prove(leaves[idx], path)
    assert tree.prove_on_gpu(leaves[idx], path) == ref, "prove_on_gpu and prove disagree"
    host, gpu = [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        tree.prove(leaves[idx], path)
        t1 = time.perf_counter()
        tree.prove_on_gpu(leaves[idx], path)
        t2 = time.perf_counter()
        host.append(t1 - t0)
        gpu.append(t2 - t1)
    print("end to end, height %d ops %d, %d alternating runs: prove %.1f ms (min %.1f), prove_on_gpu %.2f ms (min %.2f), same bytes"
          % (args.height, ops, args.runs, statistics.median(host) * 1e3, min(host) * 1e3, statistics.median(gpu) * 1e3, min(gpu) * 1e3))
    tree.free()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the resident Merkle tree (csrc/merkle_tree.hip) against the only way to reach the same state without it: a full
swm_merkle_tree_build_dev over all leaves, in the same run on the same GPU.

    python tools/merkle_tree_time.py [--height 19] [--leaf-len 72] [--runs 15] [--out profiles/merkle_tree_time.txt]

Everything stays on the device: leaves are uploaded once, update batches go through swm_merkle_tree_update_dev, paths through
swm_merkle_tree_paths_dev, checks through swm_merkle_verify_paths_dev.  Two figures per operation, each the median of --runs
calls after a warm-up call: "wall" is a host clock around the call and a synchronize with profiling off (what a caller waits
for, launch overheads and the index upload included); "kernels" is the sum of the library's own HIP events around the
operation's launches (swm_profile_*).  Records the rebuild / update ratio at k = 1, the per-level latency that implies
(time of k = 1 / height), and the batch size from which a rebuild is the faster way, if there is one among the sizes tried.
Prints what it measures and writes the same lines to --out.  Needs an MI355X: there is no fallback."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(ctx, call, runs):
    """-> (median wall ms, min wall ms, median kernel-sum ms, {kernel: calls} of one call)."""
    call()
    ctx.synchronize()
    wall = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    ctx.profile_enable(True)
    dev, launches = [], {}
    for _ in range(runs):
        ctx.profile_reset()
        call()
        ctx.synchronize()
        prof = ctx.profile()
        dev.append(sum(v["total_ms"] for v in prof.values()))
        launches = {k: v["calls"] for k, v in prof.items()}
    ctx.profile_enable(False)
    return statistics.median(wall), min(wall), statistics.median(dev), launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=19)
    ap.add_argument("--leaf-len", type=int, default=72)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_tree_time.txt"))
    args = ap.parse_args()
    from simpleworks_amd import hash as H, marlin as M

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    ctx = M.default_context()
    rng = M.generate_rand()
    leaf = H.PedersenCRH.setup(rng, H.LEAF_WINDOWS, ctx=ctx)
    inner = H.PedersenCRH.setup(rng, H.TWO_TO_ONE_WINDOWS, ctx=ctx)
    height, leaf_len = args.height, args.leaf_len
    n, levels = 1 << (height - 1), height - 1
    gen = np.random.default_rng(height)
    leaves = gen.integers(0, 256, size=(n, leaf_len), dtype=np.uint8)
    d_leaves = ctx.to_device(leaves)
    d_nodes = ctx.alloc((2 * n - 1) * 32)
    tree = ctx.merkle_tree_create_from_leaves_dev(leaf.h, inner.h, d_leaves, leaf_len, n)
    say("height %d (%d leaves of %d bytes, %d two-to-one levels), medians of %d calls" % (height, n, leaf_len, levels, args.runs))

    rebuild = measure(ctx, lambda: ctx.merkle_tree_build_dev(leaf.h, inner.h, d_leaves, leaf_len, n, d_nodes), args.runs)
    say("  full rebuild (swm_merkle_tree_build_dev, %d launches): wall %.3f ms (min %.3f), kernels %.3f ms"
        % (sum(rebuild[3].values()), rebuild[0], rebuild[1], rebuild[2]))

    results = {}
    for k in (1, 2, 256, 1 << 14):
        indices = gen.choice(n, size=k, replace=False).astype(np.uint64)
        d_new = ctx.to_device(gen.integers(0, 256, size=(k, leaf_len), dtype=np.uint8))
        r = measure(ctx, lambda: ctx.merkle_tree_update_dev(tree, indices, d_new, leaf_len), args.runs)
        results[k] = r
        say("  update_many k = %5d (%d launches): wall %.3f ms (min %.3f), kernels %.3f ms; rebuild / update: wall %.1fx, kernels %.1fx"
            % (k, sum(r[3].values()), r[0], r[1], r[2], rebuild[0] / r[0], rebuild[2] / r[2]))
        d_new.free()
    one = results[1]
    say("  k = 1: rebuild / update = %.1fx by wall time, %.1fx by kernel time; per-level latency (time of k = 1 / height) = %.1f us wall, "
        "%.1f us kernels" % (rebuild[0] / one[0], rebuild[2] / one[2], one[0] * 1e3 / height, one[2] * 1e3 / height))
    slower = [k for k in sorted(results) if results[k][0] >= rebuild[0]]
    say("  a full rebuild is the faster way from k = %d on (of the sizes tried)" % slower[0] if slower
        else "  no batch size tried (up to %d of %d leaves) is slower than a full rebuild" % (max(results), n))

    count = 1 << 14
    idx = gen.integers(0, n, size=count).astype(np.uint64)
    d_idx, d_sib = ctx.to_device(idx), ctx.alloc(count * levels * 32)
    r = measure(ctx, lambda: ctx.merkle_tree_paths_dev(tree, d_idx, count, d_sib), args.runs)
    say("  generate_proofs, %d paths (%.1f MB): wall %.3f ms (min %.3f), kernel %.3f ms = %.0f GB/s written"
        % (count, count * levels * 32 / 1e6, r[0], r[1], r[2], count * levels * 32 / 1e6 / r[2]))
    # the paths are checked with the ORIGINAL leaf bytes against the tree as the updates left it: a path verifies exactly where
    # no update has changed the leaf's digest
    picked = leaves[idx.astype(np.int64)]
    untouched = (ctx.merkle_tree_nodes(tree)[idx.astype(np.int64)] == leaf.evaluate_many(picked)).all(axis=1)
    d_root, d_pl, d_ok = ctx.to_device(ctx.merkle_tree_root(tree)), ctx.to_device(picked), ctx.alloc(count + 64)
    r = measure(ctx, lambda: ctx.merkle_verify_paths_dev(leaf.h, inner.h, height, d_root, 0, d_pl, leaf_len, d_idx, d_sib, count, d_ok),
                args.runs)
    ok = d_ok.download((count,), np.uint8)
    assert (ok != 0).tolist() == untouched.tolist(), "verify_paths disagrees with the leaf digests of the tree"
    say("  verify_paths, %d paths of %d levels (%d accepted, %d of updated leaves refused): wall %.3f ms (min %.3f), kernel %.3f ms = "
        "%.2f us per path" % (count, levels, int(untouched.sum()), int((~untouched).sum()), r[0], r[1], r[2], r[2] * 1e3 / count))
    for b in (d_leaves, d_nodes, d_idx, d_sib, d_root, d_pl, d_ok):
        b.free()
    ctx.merkle_tree_destroy(tree)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the resident Poseidon Merkle tree (csrc/poseidon_tree.hip), its membership witness and proof
(csrc/poseidon_tree_witness.hip), and beside each figure the Pedersen tree's (csrc/merkle_tree.hip, csrc/merkle_witness.hip) taken
in the same run on the same GPU.

    python tools/poseidon_tree_time.py [--height 19] [--leaf-len 72] [--runs 15] [--out profiles/poseidon_tree_time.txt]

Sections, each a child process of its own under its own time limit (a section that fails or runs out of time ends the run: nothing
more is started on the GPU, what was measured so far is written):
    tree      build from 2^(height - 1) leaves; update with k = 1, 2, 64, 2^14; verify_paths at 2^14 and 2^20 paths
    witness   the membership witness, treeless and from the resident tree, at count 1 and 2^10
    proof     one membership proof end to end, witness included, for both hashes (the Pedersen circuit takes one-byte leaves)
"kernels" is the sum of the library's own HIP events around a call's launches (swm_profile_*), "wall" a host clock around the host
form of the call and a synchronize, copies included; each the median of --runs calls after a warm-up call.  There is no threshold:
the figures go to the output file.  Needs an MI355X: there is no fallback."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARAMS = os.path.join(ROOT, "tests", "golden", "poseidon_params.json")
LIMITS = {"tree": 360, "witness": 240, "proof": 400}   # seconds per section


def measure(ctx, call, runs):
    """-> (median wall ms, median kernel-sum ms, launches of one call)."""
    call()
    ctx.synchronize()
    wall = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    ctx.profile_enable(True)
    dev, launches = [], 0
    for _ in range(runs):
        ctx.profile_reset()
        call()
        ctx.synchronize()
        prof = ctx.profile()
        dev.append(sum(v["total_ms"] for v in prof.values()))
        launches = sum(v["calls"] for v in prof.values())
    ctx.profile_enable(False)
    return statistics.median(wall), statistics.median(dev), launches


def fmt(r):
    return "wall %9.3f ms, kernels %9.3f ms, %2d launches" % r


def section_tree(args, say):
    from simpleworks_amd import hash as H, marlin as M
    ctx = M.default_context()
    height, leaf_len, runs = args.height, args.leaf_len, args.runs
    n = 1 << (height - 1)
    gen = np.random.default_rng(height)
    leaves = gen.integers(0, 256, size=(n, leaf_len), dtype=np.uint8)
    sponge = H.PoseidonSponge(H.PoseidonParameters.from_json(PARAMS), ctx)
    rng = M.generate_rand()
    leaf, inner = H.PedersenCRH.setup(rng, H.LEAF_WINDOWS, ctx=ctx), H.PedersenCRH.setup(rng, H.TWO_TO_ONE_WINDOWS, ctx=ctx)
    made = []

    def build_poseidon():
        made.append(ctx.poseidon_tree_create_from_leaves(sponge.h, leaves))
        if len(made) > 1:
            ctx.poseidon_tree_destroy(made.pop(0))

    def build_pedersen():
        made.append(ctx.merkle_tree_create_from_leaves(leaf.h, inner.h, leaves))
        if len(made) > 1:
            ctx.merkle_tree_destroy(made.pop(0))
    say("  build from %d leaves          poseidon: %s" % (n, fmt(measure(ctx, build_poseidon, runs))))
    pt = made.pop()
    say("  build from %d leaves          pedersen: %s" % (n, fmt(measure(ctx, build_pedersen, runs))))
    mt = made.pop()
    for k in (1, 2, 64, 1 << 14):
        idx = gen.choice(n, size=k, replace=False).astype(np.uint64)
        new = gen.integers(0, 256, size=(k, leaf_len), dtype=np.uint8)
        say("  update k = %5d                  poseidon: %s" % (k, fmt(measure(ctx, lambda: ctx.poseidon_tree_update(pt, idx, new), runs))))
        say("  update k = %5d                  pedersen: %s" % (k, fmt(measure(ctx, lambda: ctx.merkle_tree_update(mt, idx, new), runs))))
        leaves[idx.astype(np.int64)] = new
    p_root, m_root = ctx.poseidon_tree_root(pt), ctx.merkle_tree_root(mt)
    for count in (1 << 14, 1 << 20):
        idx = gen.integers(0, n, size=count).astype(np.uint64)
        picked = leaves[idx.astype(np.int64)]
        sib = ctx.poseidon_tree_paths(pt, height - 1, idx)
        r = measure(ctx, lambda: ctx.poseidon_verify_paths(sponge.h, height, p_root, picked, idx, sib), max(3, runs // 3))
        ok, _ = ctx.poseidon_verify_paths(sponge.h, height, p_root, picked, idx, sib)
        assert ok.all(), "poseidon verify_paths refuses a path of its own tree"
        say("  verify_paths %7d paths         poseidon: %s = %.3f us per path" % (count, fmt(r), r[1] * 1e3 / count))
        sib = ctx.merkle_tree_paths(mt, height - 1, idx)
        r = measure(ctx, lambda: ctx.merkle_verify_paths(leaf.h, inner.h, height, m_root, picked, idx, sib), max(3, runs // 3))
        ok, _ = ctx.merkle_verify_paths(leaf.h, inner.h, height, m_root, picked, idx, sib)
        assert ok.all(), "pedersen verify_paths refuses a path of its own tree"
        say("  verify_paths %7d paths         pedersen: %s = %.3f us per path" % (count, fmt(r), r[1] * 1e3 / count))
    ctx.poseidon_tree_destroy(pt)
    ctx.merkle_tree_destroy(mt)


def section_witness(args, say):
    from simpleworks_amd import hash as H, marlin as M, workloads as W
    ctx = M.default_context()
    height, leaf_len, runs = args.height, args.leaf_len, args.runs
    n = 1 << (height - 1)
    gen = np.random.default_rng(height + 1)
    leaves = gen.integers(0, 256, size=(n, leaf_len), dtype=np.uint8)
    sponge = H.PoseidonSponge(H.PoseidonParameters.from_json(PARAMS), ctx)
    tree = H.PoseidonMerkleTree.new(sponge, leaves)
    circuit = H.PoseidonMembershipCircuit(sponge, height, leaf_len)
    nw = circuit.shape()[1]
    say("  poseidon circuit: num_instance %d, num_witness %d, num_constraints %d" % circuit.shape())
    params = W.MerkleParams()
    leaf, inner = params.crh(ctx)
    u8 = gen.integers(0, 256, size=n, dtype=np.uint8)
    mt = ctx.merkle_tree_create_from_leaves(leaf.h, inner.h, u8.reshape(n, 1))
    mc = H.MerkleCircuit(leaf, inner, height)
    say("  pedersen circuit (one-byte leaves): num_instance %d, num_witness %d, num_constraints %d" % mc.shape())
    for count in (1, 1 << 10):
        idx = gen.integers(0, n, size=count).astype(np.uint64)
        picked = leaves[idx.astype(np.int64)]
        sib = ctx.poseidon_tree_paths(tree.h, height - 1, idx)
        a = measure(ctx, lambda: ctx.poseidon_tree_witness(circuit.h, nw, picked, idx, sib), runs)
        b = measure(ctx, lambda: ctx.poseidon_tree_witness_at(circuit.h, tree.h, nw, picked, idx), runs)
        w0, roots = ctx.poseidon_tree_witness(circuit.h, nw, picked, idx, sib)
        assert np.array_equal(w0, ctx.poseidon_tree_witness_at(circuit.h, tree.h, nw, picked, idx)) and (roots == ctx.poseidon_tree_root(tree.h)).all()
        say("  witness count %5d  poseidon treeless: %s" % (count, fmt(a)))
        say("  witness count %5d  poseidon _at     : %s" % (count, fmt(b)))
        # the Pedersen witness on device buffers: 2^10 of them are 2.9 GB, which the host form would also copy back
        d_l, d_i = ctx.to_device(u8[idx.astype(np.int64)]), ctx.to_device(idx)
        d_s, d_w = ctx.to_device(ctx.merkle_tree_paths(mt, height - 1, idx)), ctx.alloc(count * mc.shape()[1] * 32)
        c = measure(ctx, lambda: ctx.merkle_witness_dev(mc.h, d_l, d_i, d_s, count, d_w), runs)
        say("  witness count %5d  pedersen (device buffers, no copies): %s" % (count, fmt(c)))
        for buf in (d_l, d_i, d_s, d_w):
            buf.free()
    ctx.merkle_tree_destroy(mt)
    tree.free()


def section_proof(args, say):
    from simpleworks_amd import hash as H, marlin as M, workloads as W
    ctx = M.default_context()
    height, leaf_len = args.height, args.leaf_len
    runs = max(5, args.runs // 3)
    n = 1 << (height - 1)
    gen = np.random.default_rng(height + 2)
    leaves = gen.integers(0, 256, size=(n, leaf_len), dtype=np.uint8)
    pparams = H.PoseidonParameters.from_json(PARAMS)
    sponge = H.PoseidonSponge(pparams, ctx)
    tree = H.PoseidonMerkleTree.new(sponge, leaves)
    circuit = H.PoseidonMembershipCircuit(sponge, height, leaf_len)
    index = n - 5
    sib, root, leaf = tree.generate_proof(index), tree.root(), leaves[index].tobytes()
    cs = M.MarlinInst._synthesize(W.PoseidonMerkleTreeVerification(pparams, root, leaf, index, sib))
    packed = cs.pack()
    nnz = max(int(m[0][-1]) for m in packed.mats)
    srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, M.generate_rand())
    pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
    srs.free()

    def wall(call):
        call()
        out = []
        for _ in range(runs):
            t0 = time.perf_counter()
            call()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out), min(out)
    proof = M.generate_poseidon_membership_proof(pk, circuit, root, leaf, index, sib, M.generate_rand())
    assert M.verify_proof(vk, cs.instance[1:], M.MarlinProof(proof), M.generate_rand())
    a = wall(lambda: M.generate_poseidon_membership_proof(pk, circuit, root, leaf, index, sib, M.generate_rand()))
    b = wall(lambda: M.generate_poseidon_membership_proof(pk, circuit, None, leaf, index, None, M.generate_rand(), tree=tree))
    say("  poseidon membership proof, %d rows, %d variables, non-zeros A / B / C %s: prove (walk + record + prover) %.3f ms (min %.3f), "
        "prove_at (gather + record + prover) %.3f ms (min %.3f), %d bytes"
        % (cs.num_constraints, len(cs.instance) + len(cs.witness), " / ".join(str(int(m[0][-1])) for m in packed.mats), a[0], a[1], b[0], b[1],
           len(proof)))
    pk.free()
    tree.free()
    u8 = [int(v) for v in gen.integers(0, 256, size=n)]
    smt = W.SimpleMerkleTree(u8, params=W.MerkleParams(), ctx=ctx)
    path = smt.get_merkle_path(index)
    proof = smt.prove_on_gpu(u8[index], path)
    assert smt.verify(proof, u8[index])
    c = wall(lambda: smt.prove_on_gpu(u8[index], path))
    ped = W.merkle_membership_circuit(height=height, gadget_byte_ops=0, params=smt.params)[0].pack()
    say("  pedersen membership proof (one-byte leaf), %d rows, non-zeros A / B / C %s, witness included: prove %.3f ms (min %.3f), %d bytes"
        % (M.merkle_circuit_shape(height)[2], " / ".join(str(int(m[0][-1])) for m in ped.mats), c[0], c[1], len(proof)))
    say("  pedersen / poseidon: %.1fx against prove, %.1fx against prove_at" % (c[0] / a[0], c[0] / b[0]))
    smt.free()


SECTIONS = {"tree": section_tree, "witness": section_witness, "proof": section_proof}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=19)
    ap.add_argument("--leaf-len", type=int, default=72)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseidon_tree_time.txt"))
    ap.add_argument("--section", choices=sorted(SECTIONS), help="run one section in this process (what the parent starts)")
    args = ap.parse_args()
    if args.section:
        SECTIONS[args.section](args, lambda text: print(text, flush=True))
        return 0
    lines = ["Poseidon Merkle tree beside the Pedersen tree, one MI355X, one run: height %d (%d leaves of %d bytes), medians of %d calls "
             "after a warm-up" % (args.height, 1 << (args.height - 1), args.leaf_len, args.runs)]
    rc = 0
    for name in ("tree", "witness", "proof"):
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--height", str(args.height), "--leaf-len", str(args.leaf_len),
               "--runs", str(args.runs)]
        shown = len(lines)
        lines.append("%s:" % name)
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[name])
            lines += [l for l in out.stdout.splitlines() if l.startswith("  ")]
            rc = out.returncode
            if rc != 0:
                lines.append("  FAILED with exit status %d: %s" % (rc, out.stderr.strip().splitlines()[-1:] or ""))
        except subprocess.TimeoutExpired as e:
            lines += [l for l in (e.stdout or b"").decode(errors="replace").splitlines() if l.startswith("  ")]
            lines.append("  NOT FINISHED within %d s" % LIMITS[name])
            rc = 124
        print("\n".join(lines[shown:]), flush=True)
        if rc != 0:
            break   # nothing more is started on the GPU after a section that failed or hung
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())

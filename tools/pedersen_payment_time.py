#!/usr/bin/env python3
"""Times the payment circuit over a Pedersen account tree (csrc/pedersen_payment_witness.hip): its witness split by launch and its
proof with the witness included, in the manner of tools/payment_time.py (whose figures for the Poseidon form are in
profiles/payment_time.txt).

    python tools/pedersen_payment_time.py [--height 9] [--runs 15] [--out profiles/pedersen_payment_time.txt]

Sections, each a child process of its own under its own time limit (a section that fails or runs out of time ends the run: nothing
more is started on the GPU, what was measured so far is written):
    witness   swm_pedersen_payment_witness_at for 1 and for 256 payments: host wall time, the sum of the library's HIP events around
              its launches (swm_profile_*), and that sum split by kernel; then the sibling form (the walk instead of the gather)
    proof     swm_pedersen_payment_prove_at, the witness included; 8 proofs in one call beside 8 single calls, alternating
Each figure is the median of --runs calls after a warm-up call.  There is no threshold: the figures go to the output file.  Needs
an MI355X: there is no fallback."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"witness": 240, "proof": 500}   # seconds per section
SEQUENTIAL_STAGE_MS = 0.23                # one dependent hash stage of merkle_witness_kernel


def world(height, accounts=3):
    """A ledger over its default Pedersen account tree with `accounts` funded accounts -> (ledger module, parameters, state, keys,
    rng)."""
    from simpleworks_amd import ledger as L, marlin as M
    rng = M.generate_rand()
    pp = L.Parameters.sample(rng)
    state = L.State(1 << height, pp)
    people = [state.sample_keys_and_register(pp, rng) for _ in range(accounts)]
    for acc, _, _ in people:
        state.update_balance(acc, 1 << 40)
    return L, pp, state, people, rng


def _profiled(ctx, call, runs, count, say, what):
    wall = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    ctx.profile_enable(True)
    per_kernel, total = {}, []
    for _ in range(runs):
        ctx.profile_reset()
        call()
        ctx.synchronize()
        prof = ctx.profile()
        total.append(sum(v["total_ms"] for v in prof.values()))
        for name, v in prof.items():
            per_kernel.setdefault(name, []).append((v["total_ms"], v["calls"]))
    ctx.profile_enable(False)
    say("  %3d payments, %s: wall (copies included) %9.3f ms, kernels %8.3f ms = %8.3f us per payment, %d launches"
        % (count, what, statistics.median(wall), statistics.median(total), statistics.median(total) * 1e3 / count,
           sum(v[0][1] for v in per_kernel.values())))
    for name, v in sorted(per_kernel.items(), key=lambda kv: -statistics.median(x[0] for x in kv[1])):
        say("      %-26s %d launch(es) %8.3f ms" % (name, v[0][1], statistics.median(x[0] for x in v)))


def section_witness(args, say):
    from payment_time import payments
    L, pp, state, people, rng = world(args.height)
    ctx = pp.sig_params.ctx
    tree = state.account_merkle_tree
    circuit = L.PedersenPaymentCircuit(pp.sig_params, pp.leaf_crh, pp.two_to_one_crh, args.height)
    say("  circuit at height %d: num_instance %d, num_witness %d, num_constraints %d" % ((args.height,) + circuit.shape()))
    stages = 2 * args.height
    say("  the sequential chain it replaces: %d hash stages of a payment x %.2f ms = %.2f ms, one workgroup per path"
        % (stages, SEQUENTIAL_STAGE_MS, stages * SEQUENTIAL_STAGE_MS))
    for count in (1, 256):
        block = payments(L, pp, state, people, rng, count)
        _, flags = circuit.witness_at(tree, block)
        assert (flags == 3).all()
        _profiled(ctx, lambda: circuit.witness_at(tree, block), args.runs, count, say, "resident tree")
        paths_s = [tree.generate_proof(p[0][0]) for p in block]
        paths_r = [tree.generate_proof(p[0][1]) for p in block]
        w, flags, roots_s, roots_r = circuit.witness_many(block, paths_s, paths_r)
        assert (flags == 3).all() and set(roots_s) == set(roots_r) == {tree.root()}
        _profiled(ctx, lambda: circuit.witness_many(block, paths_s, paths_r), args.runs, count, say, "sibling arrays")
    circuit.free()
    state.free()


def section_proof(args, say):
    from payment_time import _alternate, payments
    from simpleworks_amd import marlin as M
    L, pp, state, people, rng = world(args.height)
    runs = max(5, args.runs // 2)
    tree = state.account_merkle_tree
    circuit, pk, vk = state.pedersen_payment_keys(rng)
    block = payments(L, pp, state, people, rng, 8)
    msg, sig, sender_leaf, recipient_leaf = block[0]
    proof = M.generate_pedersen_payment_proof(pk, circuit, tree, msg, sig, sender_leaf, recipient_leaf, M.generate_rand())
    assert L.verify_payment(vk, [tree.root(), msg[0], msg[1], int.from_bytes(msg[2:], "little")], proof, M.generate_rand())

    def many():
        proofs, flags = M.generate_pedersen_payment_proofs(pk, circuit, tree, block, M.generate_rand())
        assert flags == [3] * len(block)
        return proofs

    def singles():
        r = M.generate_rand()
        return [M.generate_pedersen_payment_proof(pk, circuit, tree, *p, r) for p in block]
    one = lambda: M.generate_pedersen_payment_proof(pk, circuit, tree, msg, sig, sender_leaf, recipient_leaf, M.generate_rand())
    one()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        one()
        t.append((time.perf_counter() - t0) * 1e3)
    say("  payment proof (%d rows, %d witnesses, 4 public inputs), witness included: %8.3f ms (min %8.3f), %d bytes"
        % (circuit.shape()[2], circuit.shape()[1], statistics.median(t), min(t), len(proof)))
    assert many() == singles()
    a, b = _alternate(many, singles, max(3, args.runs // 5))
    say("  %d proofs in one call: %8.3f ms per proof (min %8.3f); %d single calls: %8.3f ms per proof (min %8.3f)"
        % (len(block), a[0] / len(block), a[1] / len(block), len(block), b[0] / len(block), b[1] / len(block)))
    state.free()


SECTIONS = {"witness": section_witness, "proof": section_proof}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=9)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pedersen_payment_time.txt"))
    ap.add_argument("--section", choices=sorted(SECTIONS), help="run one section in this process (what the parent starts)")
    args = ap.parse_args()
    if args.section:
        return SECTIONS[args.section](args, lambda text: print(text, flush=True)) or 0
    lines = ["Payment circuit over a Pedersen account tree of height %d, one MI355X, one run: medians of %d calls (proofs: fewer, see "
             "tools/pedersen_payment_time.py) after a warm-up" % (args.height, args.runs)]
    rc = 0
    for name in ("witness", "proof"):
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--height", str(args.height), "--runs", str(args.runs)]
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

#!/usr/bin/env python3
"""Times the account-update circuit over the Pedersen account tree (csrc/pedersen_account_update_witness.hip): every launch of a
block of dependent operations, beside what the ledger did for the same operations before (one path gather and one
swm_merkle_tree_update each, nothing proved); the whole swm_pedersen_account_update_prove_at call; and bench.py's headline on both
builds.

    python tools/pedersen_account_update_time.py --parent DIR [--height 9] [--runs 15] [--out profiles/pedersen_account_update_time.txt]

--parent DIR: a checkout of the parent commit with its library built.  The sections named "parent ..." run there (their child
process imports DIR's package, not this one), in the same session, between this build's sections.
Sections, each a child process of its own under its own time limit (a section that fails or runs out of time ends the run: nothing
more is started on the GPU, what was measured so far is written):
    witness          swm_pedersen_account_update_witness_at for 1, 8 and 64 dependent operations (balance updates round three accounts,
                     every one witnessed against the tree the one before left): host wall time, the sum of the library's HIP events
                     around its launches (swm_profile_*), and that sum split by launch: pedersen_transfer_check the table against the
                     tree, pedersen_account_update_advance the advancing kernel, pedersen_payment_leaves / _levels the record
                     launches, pedersen_account_update_bits the booleans and the masked bits
    parent updates   the same operations by one path gather and one tree update each, host wall time
    proof            swm_pedersen_account_update_prove_at for a balance update and for a registration, witness and advance included
    headline         bench.py --gpus 1 --steps 20 --warmup 5 on this build and on the parent, alternating, twice each
Each figure is the median of --runs calls after a warm-up call.  There is no threshold: the figures go to the output file.  Needs
an MI355X: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"witness": 240, "parent updates": 240, "proof": 400, "headline": 1000}   # seconds
COUNTS = (1, 8, 64)


def world(root, height, accounts=3):
    """A ledger over the default (Pedersen) account tree with `accounts` funded accounts -> (ledger module, parameters, state, keys,
    rng)."""
    from simpleworks_amd import hash as H, ledger as L, marlin as M
    rng = M.generate_rand()
    pp = L.Parameters.sample(rng, poseidon=H.PoseidonParameters.from_json(os.path.join(root, "tests", "golden", "poseidon_params.json")))
    state = L.State(1 << height, pp)
    people = [state.sample_keys_and_register(pp, rng) for _ in range(accounts)]
    for acc, _, _ in people:
        state.update_balance(acc, 1 << 40)
    return L, pp, state, people, rng


def updates(people, count, salt=0):
    """count balance updates round the accounts: (id, new balance)."""
    return [(people[k % len(people)][0], 1000 + 7 * k + salt) for k in range(count)]


def _median_wall(call, runs, sync):
    call()
    wall = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        sync()
        wall.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(wall), min(wall)


def section_witness(args, say):
    L, pp, state, people, rng = world(HERE, args.height)
    ctx = pp.sig_params.ctx
    circuit = L.PedersenAccountUpdateCircuit(pp.leaf_crh, pp.two_to_one_crh, args.height)
    tree = state.account_merkle_tree
    say("  circuit at height %d: num_instance %d, num_witness %d, num_constraints %d" % ((args.height,) + circuit.shape()))
    table = [state.account_table()]
    turn = [0]
    for count in COUNTS:
        def call():      # every call goes on from the state the one before left; the balances change from call to call
            turn[0] += 1
            block = [(acc, 0, bytes(64), value) for acc, value in updates(people, count, turn[0])]
            _, table[0], _, _, flags, _ = circuit.witness_at(tree, table[0], block)
            assert (flags == 1).all()
        wall = _median_wall(call, args.runs, ctx.synchronize)
        ctx.profile_enable(True)
        per_kernel, total = {}, []
        for _ in range(args.runs):
            ctx.profile_reset()
            call()
            ctx.synchronize()
            prof = ctx.profile()
            total.append(sum(v["total_ms"] for v in prof.values()))
            for name, v in prof.items():
                per_kernel.setdefault(name, []).append((v["total_ms"], v["calls"]))
        ctx.profile_enable(False)
        say("  %3d operations: wall (copies included) %9.3f ms, kernels %8.3f ms = %8.3f us per operation, %d launches"
            % (count, wall[0], statistics.median(total), statistics.median(total) * 1e3 / count, sum(v[0][1] for v in per_kernel.values())))
        for name, v in sorted(per_kernel.items(), key=lambda kv: -statistics.median(x[0] for x in kv[1])):
            say("      %-34s %d launch(es) %8.3f ms" % (name, v[0][1], statistics.median(x[0] for x in v)))
    circuit.free()
    state.free()


def section_parent_updates(args, say):
    L, pp, state, people, rng = world(args.parent, args.height)
    ctx = pp.sig_params.ctx
    tree = state.account_merkle_tree
    turn = [0]
    for count in COUNTS:
        def call():      # what a caller who wanted the circuit's inputs did: the leaf's path, then the update
            turn[0] += 1
            for acc, value in updates(people, count, turn[0]):
                tree.generate_proofs([acc])
                state.update_balance(acc, value)
        wall = _median_wall(call, args.runs, ctx.synchronize)
        say("  %3d operations, one path gather and one update each: wall %9.3f ms (min %9.3f) = %8.3f us per operation"
            % (count, wall[0], wall[1], wall[0] * 1e3 / count))
    state.free()


def section_proof(args, say):
    from simpleworks_amd import marlin as M
    L, pp, state, people, rng = world(HERE, args.height)
    runs = max(5, args.runs // 2)
    tree = state.account_merkle_tree
    circuit, pk, vk = state.pedersen_update_keys(rng)
    table = [state.account_table()]
    turn = [0]

    def balance():
        turn[0] += 1
        proof, public, flag, _, table[0] = M.generate_pedersen_account_update_proof(pk, circuit, tree, table[0], (people[0][0], 0, bytes(64), turn[0]),
                                                                           M.generate_rand())
        assert flag == 1
        return proof, public
    proof, public = balance()
    assert L.verify_update(vk, public, proof, M.generate_rand())
    wall = _median_wall(balance, runs, lambda: None)
    say("  balance update proved (%d rows, %d witnesses, 8 public inputs), witness and advance included: %8.3f ms (min %8.3f), %d bytes"
        % (circuit.shape()[2], circuit.shape()[1], wall[0], wall[1], len(proof)))
    fresh = [len(people) + 1]
    key = L.schnorr.point_bytes(people[0][1])

    def register():      # a new leaf every call: the tree of height 9 has room for the warm-up and the runs
        proof, public, flag, _, table[0] = M.generate_pedersen_account_update_proof(pk, circuit, tree, table[0], (fresh[0], 1, key, 0), M.generate_rand())
        assert flag == 1
        fresh[0] += 1
        return proof, public
    proof, public = register()
    assert L.verify_update(vk, public, proof, M.generate_rand())
    wall = _median_wall(register, runs, lambda: None)
    say("  registration proved under the same key:                                                      %8.3f ms (min %8.3f), %d bytes"
        % (wall[0], wall[1], len(proof)))
    state.free()


def section_headline(args, say):
    rc = 0
    for k in range(4):
        root, name = (HERE, "this build") if k % 2 == 0 else (args.parent, "the parent ")
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True,
                             text=True, timeout=240, cwd=root)
        doc = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        say("  %s: bench.py --gpus 1 --steps 20 --warmup 5: %.1f constraints/s, %.3f ms per step" % (name, doc["value"], doc["ms_per_step"]))
        rc = rc or out.returncode
        if rc:
            break
    return rc


SECTIONS = {"witness": section_witness, "parent updates": section_parent_updates, "proof": section_proof, "headline": section_headline}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="a checkout of the parent commit, its library built")
    ap.add_argument("--height", type=int, default=9)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "pedersen_account_update_time.txt"))
    ap.add_argument("--only", help="comma-separated sections to run (default: all)")
    ap.add_argument("--section", choices=sorted(SECTIONS), help="run one section in this process (what the parent process starts)")
    args = ap.parse_args()
    args.parent = os.path.abspath(args.parent)
    if args.section:
        sys.path.insert(0, args.parent if args.section.startswith("parent") else HERE)
        return SECTIONS[args.section](args, lambda text: print(text, flush=True)) or 0
    lines = ["Account-update circuit over the Pedersen account tree of height %d, one MI355X, one run: medians of %d calls (proofs: fewer, "
             "see tools/pedersen_account_update_time.py) after a warm-up, alternating order where two things are compared" % (args.height, args.runs)]
    rc = 0
    for name in [s.strip() for s in args.only.split(",")] if args.only else list(SECTIONS):
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--parent", args.parent, "--height", str(args.height), "--runs",
               str(args.runs)]
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

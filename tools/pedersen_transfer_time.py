#!/usr/bin/env python3
"""Times the transfer circuit over the Pedersen account tree (csrc/pedersen_transfer_witness.hip): the advancing kernel, the check
and the record launches for blocks of dependent transfers, beside what the ledger does for the same transfers on the parent commit
(the Pedersen payment proof, two swm_merkle_tree_update calls and the path gathers); one transfer proof beside that; a block of
proofs; and bench.py's headline on both builds.

    python tools/pedersen_transfer_time.py --parent DIR [--height 9] [--runs 15] [--out profiles/pedersen_transfer_time.txt]

--parent DIR: a checkout of the parent commit with its library built.  The sections named "parent ..." run there (their child
process imports DIR's package, not this one), in the same session, between this build's sections.
Sections, each a child process of its own under its own time limit (a section that fails or runs out of time ends the run: nothing
more is started on the GPU, what was measured so far is written):
    witness          swm_pedersen_transfer_witness_at for 1, 8 and 256 dependent transfers (a ring 1 -> 2 -> 3 -> 1): host wall
                     time, the sum of the library's HIP events around its launches (swm_profile_*), and that sum split by kernel:
                     pedersen_transfer_advance is the advancing kernel, pedersen_payment_leaves / _levels the record launches
    parent updates   the same transfers by two tree updates and five path gathers each on the parent's library, host wall time
    proof            swm_pedersen_transfer_prove_at for one transfer beside swm_pedersen_payment_prove_at plus two updates for the
                     same transaction on this build, alternating, each under its own key
    parent proof     swm_pedersen_payment_prove_at plus two updates on the parent's library
    block            generate_pedersen_transfer_proofs over 8 transfers per proof, beside 8 single calls, alternating
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
LIMITS = {"witness": 300, "parent updates": 240, "proof": 400, "parent proof": 400, "block": 400, "headline": 1000}   # seconds


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


def ring(L, pp, people, rng, count):
    """count transfers round the funded accounts, each depending on the one before: Transactions."""
    return [L.Transaction.create(pp, people[k % len(people)][0], people[(k + 1) % len(people)][0], 1000 + k, people[k % len(people)][2], rng)
            for k in range(count)]


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
    L, pp, state, people, rng = world(args.height)
    ctx = pp.sig_params.ctx
    circuit = L.PedersenTransferCircuit(pp.sig_params, pp.leaf_crh, pp.two_to_one_crh, args.height)
    tree = state.account_merkle_tree
    say("  circuit at height %d: num_instance %d, num_witness %d, num_constraints %d" % ((args.height,) + circuit.shape()))
    table = [state.account_table()]
    for count in (1, 8, 256):
        block = [(tx.message(), tx.signature.to_bytes()) for tx in ring(L, pp, people, rng, count)]

        def call():      # every call goes on from the state the one before left: the ring keeps every transfer valid
            _, table[0], _, _, flags, _ = circuit.witness_at(tree, table[0], block)
            assert (flags == 31).all()
        runs = args.runs if count < 256 else max(3, args.runs // 5)
        wall = _median_wall(call, runs, ctx.synchronize)
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
        say("  %3d transfers: wall (copies included) %9.3f ms, kernels %8.3f ms = %8.3f us per transfer, %d launches"
            % (count, wall[0], statistics.median(total), statistics.median(total) * 1e3 / count, sum(v[0][1] for v in per_kernel.values())))
        for name, v in sorted(per_kernel.items(), key=lambda kv: -statistics.median(x[0] for x in kv[1])):
            say("      %-28s %d launch(es) %8.3f ms" % (name, v[0][1], statistics.median(x[0] for x in v)))
    circuit.free()
    state.free()


def _old_way(L, state, txs):
    """What the ledger does for a block today, without the proofs: per transaction the five path gathers of validate and of a
    payment witness (sender path, and running digests and siblings of both leaves), then two tree updates."""
    tree = state.account_merkle_tree
    for tx in txs:
        for ids in ([tx.sender], [tx.sender], [tx.recipient], [tx.sender], [tx.recipient]):
            tree.generate_proofs(ids)
        state.update_balance(tx.sender, state.id_to_account_info[tx.sender].balance - tx.amount)
        state.update_balance(tx.recipient, state.id_to_account_info[tx.recipient].balance + tx.amount)


def section_parent_updates(args, say):
    L, pp, state, people, rng = world(args.height)
    ctx = pp.sig_params.ctx
    for count in (1, 8, 256):
        txs = ring(L, pp, people, rng, count)
        runs = args.runs if count < 256 else max(3, args.runs // 5)
        wall = _median_wall(lambda: _old_way(L, state, txs), runs, ctx.synchronize)
        say("  %3d transfers, two updates and five path gathers each: wall %9.3f ms (min %9.3f) = %8.3f us per transfer"
            % (count, wall[0], wall[1], wall[0] * 1e3 / count))
    state.free()


def _alternate(a, b, runs):
    """Two calls in alternating order after a warm-up of each -> ((median, min) of a, (median, min) of b) in ms."""
    a()
    b()
    ta, tb = [], []
    for k in range(runs):
        for call, out in ((a, ta), (b, tb)) if k % 2 == 0 else ((b, tb), (a, ta)):
            t0 = time.perf_counter()
            call()
            out.append((time.perf_counter() - t0) * 1e3)
    return (statistics.median(ta), min(ta)), (statistics.median(tb), min(tb))


def _payment_and_updates(M, L, state, pk, circuit, tx):
    """The parent's way for one transaction: the payment proof against the tree as it stands, then the two updates."""
    tree = state.account_merkle_tree
    sender, recipient = state.id_to_account_info[tx.sender], state.id_to_account_info[tx.recipient]
    M.generate_pedersen_payment_proof(pk, circuit, tree, tx.message(), tx.signature.to_bytes(), sender.to_bytes_le(), recipient.to_bytes_le(),
                                      M.generate_rand())
    state.update_balance(tx.sender, sender.balance - tx.amount)
    state.update_balance(tx.recipient, recipient.balance + tx.amount)


def section_proof(args, say):
    from simpleworks_amd import marlin as M
    L, pp, state, people, rng = world(args.height)
    runs = max(5, args.runs // 2)
    tree = state.account_merkle_tree
    circuit, pk, vk = state.pedersen_transfer_keys(rng)
    py_circuit, py_pk, _ = state.pedersen_payment_keys(rng)
    there = ring(L, pp, people[:2], rng, 1)[0]      # 1 -> 2, again and again: the balances are large
    table = [state.account_table()]

    def transfer(tx=there):
        proof, public, flag, _, table[0] = M.generate_pedersen_transfer_proof(pk, circuit, tree, table[0], tx.message(), tx.signature.to_bytes(),
                                                                              M.generate_rand())
        assert flag == 31
        return proof, public
    proof, public = transfer()
    assert L.verify_transfer(vk, public, proof, M.generate_rand())

    def follow():      # the State's mirror follows the table for the payment's leaves
        for i, info in state.id_to_account_info.items():
            info.balance = int.from_bytes(table[0][i][64:], "little")
    follow()

    def payment():
        _payment_and_updates(M, L, state, py_pk, py_circuit, there)
        table[0] = state.account_table()

    def transfer_synced():
        transfer()
        follow()
    a, b = _alternate(transfer_synced, payment, runs)
    say("  transfer proof (%d rows, %d witnesses, 5 public inputs), witness and advance included: %8.3f ms (min %8.3f), %d bytes"
        % (circuit.shape()[2], circuit.shape()[1], a[0], a[1], len(proof)))
    say("  payment proof (%d rows, %d witnesses) and two updates, this build:               %8.3f ms (min %8.3f)"
        % (py_circuit.shape()[2], py_circuit.shape()[1], b[0], b[1]))
    say("  transfer - (payment + updates): %+.3f ms (%+.1f %%)" % (a[0] - b[0], 100 * (a[0] - b[0]) / b[0]))
    state.free()


def section_parent_proof(args, say):
    from simpleworks_amd import marlin as M
    L, pp, state, people, rng = world(args.height)
    runs = max(5, args.runs // 2)
    circuit, pk, _ = state.pedersen_payment_keys(rng)
    tx = ring(L, pp, people[:2], rng, 1)[0]
    wall = _median_wall(lambda: _payment_and_updates(M, L, state, pk, circuit, tx), runs, lambda: None)
    say("  payment proof (%d rows, %d witnesses) and two updates, the parent's library: %8.3f ms (min %8.3f)"
        % (circuit.shape()[2], circuit.shape()[1], wall[0], wall[1]))
    state.free()


def section_block(args, say):
    from simpleworks_amd import marlin as M
    L, pp, state, people, rng = world(args.height)
    runs = max(3, args.runs // 5)
    tree = state.account_merkle_tree
    circuit, pk, vk = state.pedersen_transfer_keys(rng)
    block = [(tx.message(), tx.signature.to_bytes()) for tx in ring(L, pp, people, rng, 8)]
    table = [state.account_table()]

    def many():
        proofs, _, flags, _, table[0] = M.generate_pedersen_transfer_proofs(pk, circuit, tree, table[0], block, M.generate_rand())
        assert flags == [31] * len(block)
        return proofs

    def singles():
        r = M.generate_rand()
        out = []
        for m, s in block:
            proof, _, _, _, table[0] = M.generate_pedersen_transfer_proof(pk, circuit, tree, table[0], m, s, r)
            out.append(proof)
        return out
    a, b = _alternate(many, singles, runs)
    say("  %d proofs in one call: %8.3f ms per proof (min %8.3f); %d single calls: %8.3f ms per proof (min %8.3f)"
        % (len(block), a[0] / len(block), a[1] / len(block), len(block), b[0] / len(block), b[1] / len(block)))
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


SECTIONS = {"witness": section_witness, "parent updates": section_parent_updates, "proof": section_proof, "parent proof": section_parent_proof,
            "block": section_block, "headline": section_headline}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="a checkout of the parent commit, its library built")
    ap.add_argument("--height", type=int, default=9)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "pedersen_transfer_time.txt"))
    ap.add_argument("--only", help="comma-separated sections to run (default: all)")
    ap.add_argument("--section", choices=sorted(SECTIONS), help="run one section in this process (what the parent process starts)")
    args = ap.parse_args()
    args.parent = os.path.abspath(args.parent)
    if args.section:
        sys.path.insert(0, args.parent if args.section.startswith("parent") else HERE)
        return SECTIONS[args.section](args, lambda text: print(text, flush=True)) or 0
    lines = ["Transfer circuit over the Pedersen account tree of height %d, one MI355X, one run: medians of %d calls (proofs and blocks of "
             "256: fewer, see tools/pedersen_transfer_time.py) after a warm-up, alternating order where two things are compared"
             % (args.height, args.runs)]
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

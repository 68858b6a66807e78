#!/usr/bin/env python3
"""Times the rollup (csrc/rollup_witness.hip): ONE proof for a block of transfers beside one proof per transfer for the same block,
in the same process, under each form's own key.

    python tools/rollup_time.py [--height 9] [--runs 9] [--out profiles/rollup_time.txt]

Sections, each a child process of its own under its own time limit (a section that fails or runs out of time ends the run: nothing
more is started on the GPU, what was measured so far is written):
    poseidon   a block of 8 transfers over the Poseidon account tree: swm_rollup_prove_at beside swm_transfer_prove_many_at on the
               same 8 transfers, alternating; the rollup's split into advance, record, link and prover from the library's HIP events
               around its launches (swm_profile_*, a run of its own); verify_rollup beside 8 x verify_transfer, alternating
    pedersen   the same for a block of 4 transfers over the Pedersen account tree
Each figure is the median of --runs calls after a warm-up call; host wall time around calls that return when the proof is on the
host.  There is no threshold: the figures go to the output file.  Needs an MI355X: there is no fallback."""
import argparse
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"poseidon": 500, "pedersen": 700}   # seconds
BLOCK = {"poseidon": 8, "pedersen": 4}


def world(height, tree, accounts=3):
    from simpleworks_amd import hash as H, ledger as L, marlin as M
    rng = M.generate_rand()
    poseidon = H.PoseidonParameters.from_json(os.path.join(HERE, "tests", "golden", "poseidon_params.json")) if tree == "poseidon" else None
    pp = L.Parameters.sample(rng, poseidon=poseidon)
    state = L.State(1 << height, pp, account_tree=tree)
    people = [state.sample_keys_and_register(pp, rng) for _ in range(accounts)]
    for acc, _, _ in people:
        state.update_balance(acc, 1 << 40)
    return L, M, pp, state, people, rng


def ring(L, pp, people, rng, count):
    """count transfers round the funded accounts, each depending on the one before."""
    return [L.Transaction.create(pp, people[k % len(people)][0], people[(k + 1) % len(people)][0], 1000 + k, people[k % len(people)][2], rng)
            for k in range(count)]


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


def _domains(shape, nnz):
    pow2 = lambda v: 1 << (int(v) - 1).bit_length()
    return pow2(max(shape[2], shape[0] + shape[1])), pow2(nnz)


def _nnz(state, n):
    return n * max(int(m[0][-1]) for m in state._rollup_transfer_system.mats)


def section(args, say, tree):
    L, M, pp, state, people, rng = world(args.height, tree)
    pedersen = tree == "pedersen"
    n = BLOCK[tree]
    ctx = pp.sig_params.ctx
    t0 = time.perf_counter()
    circuit, pk, vk = state.pedersen_transfer_keys(rng) if pedersen else state.transfer_keys(rng)
    t1 = time.perf_counter()
    ru_circuit, ru_pk, ru_vk = state.pedersen_rollup_keys(n, rng) if pedersen else state.rollup_keys(n, rng)
    t2 = time.perf_counter()
    h1, k1 = _domains(circuit.shape(), _nnz(state, 1))
    h2, k2 = _domains(ru_circuit.shape(), _nnz(state, n))
    say("  transfer key: %d rows, %d witnesses, |H| = 2^%d, |K| = 2^%d, derived in %.1f s" % (circuit.shape()[2], circuit.shape()[1], h1.bit_length() - 1,
                                                                                            k1.bit_length() - 1, t1 - t0))
    say("  rollup key of %d: %d rows, %d witnesses, %d public inputs, |H| = 2^%d, |K| = 2^%d, derived in %.1f s (one transfer system, relabelled)"
        % (n, ru_circuit.shape()[2], ru_circuit.shape()[1], ru_circuit.shape()[0] - 1, h2.bit_length() - 1, k2.bit_length() - 1, t2 - t1))
    tree_h = state.account_merkle_tree
    block = [(tx.message(), tx.signature.to_bytes()) for tx in ring(L, pp, people, rng, n)]
    table = [state.account_table()]
    many_entry = M.generate_pedersen_transfer_proofs if pedersen else M.generate_transfer_proofs
    one_entry = M.generate_pedersen_rollup_proof if pedersen else M.generate_rollup_proof
    last = {}

    def many():      # every call goes on from the state the one before left: the ring keeps every transfer valid
        proofs, public, flags, _, table[0] = many_entry(pk, circuit, tree_h, table[0], block, M.generate_rand())
        assert flags == [31] * n
        last["many"] = (proofs, public)

    def rollup():
        proof, public, flags, _, table[0], applied = one_entry(ru_pk, ru_circuit, tree_h, table[0], block, M.generate_rand())
        assert applied and proof is not None
        last["rollup"] = (proof, public)
    a, b = _alternate(rollup, many, args.runs)
    say("  ONE rollup proof of %d transfers, pass and advance included: %9.3f ms (min %9.3f), %d bytes" % (n, a[0], a[1], len(last["rollup"][0])))
    say("  %d transfer proofs in one call (swm_%stransfer_prove_many_at): %9.3f ms (min %9.3f) = %8.3f ms per proof, %d bytes in all"
        % (n, "pedersen_" if pedersen else "", b[0], b[1], b[0] / n, sum(len(p) for p in last["many"][0])))
    say("  rollup - per-transfer proofs: %+.3f ms (%+.1f %%)" % (a[0] - b[0], 100 * (a[0] - b[0]) / b[0]))
    # the rollup's split, from the library's events around every launch: a run of its own (the events serialise the streams)
    ctx.profile_enable(True)
    groups = {"advance": [], "record": [], "link": [], "other witness kernels": [], "prover": []}
    walls = []
    for _ in range(max(3, args.runs // 2)):
        ctx.profile_reset()
        t0 = time.perf_counter()
        rollup()
        ctx.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        sums = dict.fromkeys(groups, 0.0)
        for name, v in ctx.profile().items():
            if name.endswith("transfer_advance"):
                sums["advance"] += v["total_ms"]
            elif name in ("poseidon_tree_record", "pedersen_payment_leaves", "pedersen_payment_levels"):
                sums["record"] += v["total_ms"]
            elif name == "rollup_link":
                sums["link"] += v["total_ms"]
            elif name.startswith(("transfer_", "schnorr_witness", "pedersen_transfer_")):
                sums["other witness kernels"] += v["total_ms"]
            else:
                sums["prover"] += v["total_ms"]
        for k, v in sums.items():
            groups[k].append(v)
    ctx.profile_enable(False)
    say("  the rollup call under per-launch events (wall %9.3f ms): " % statistics.median(walls)
        + ", ".join("%s %.3f ms" % (k, statistics.median(v)) for k, v in groups.items()) + " (sums of kernel times)")
    # the verifier
    proofs, publics = last["many"]
    ru_proof, ru_public = last["rollup"]

    def verify_one():
        assert L.verify_rollup(ru_vk, ru_public, ru_proof, M.generate_rand())

    def verify_many():
        for proof, public in zip(proofs, publics):
            assert L.verify_transfer(vk, public, proof, M.generate_rand())
    a, b = _alternate(verify_one, verify_many, args.runs)
    say("  verify_rollup (%d public inputs): %8.3f ms (min %8.3f); %d x verify_transfer: %8.3f ms (min %8.3f)"
        % (len(ru_public), a[0], a[1], n, b[0], b[1]))
    state.free()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=9)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "rollup_time.txt"))
    ap.add_argument("--only", help="comma-separated sections to run (default: all)")
    ap.add_argument("--section", choices=sorted(LIMITS), help="run one section in this process (what the parent process starts)")
    args = ap.parse_args()
    if args.section:
        sys.path.insert(0, HERE)
        return section(args, lambda text: print(text, flush=True), args.section)
    lines = ["Rollup: one proof for a block of transfers at height %d, one MI355X, one run: medians of %d calls after a warm-up, alternating "
             "order where two things are compared" % (args.height, args.runs)]
    rc = 0
    for name in [s.strip() for s in args.only.split(",")] if args.only else list(LIMITS):
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

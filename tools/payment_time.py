#!/usr/bin/env python3
"""Times the payment circuit (csrc/payment_witness.hip): its witness split by launch, its proof beside the signature-only proof the
ledger made before (swm_schnorr_prove) for the same transaction, a block of proofs beside single calls, and bench.py's headline.

    python tools/payment_time.py [--height 9] [--runs 15] [--out profiles/payment_time.txt]

Sections, each a child process of its own under its own time limit (a section that fails or runs out of time ends the run: nothing
more is started on the GPU, what was measured so far is written):
    witness   swm_payment_witness_at for 1 and for 256 payments: host wall time, the sum of the library's HIP events around its
              launches (swm_profile_*), and that sum split by kernel
    proof     swm_payment_prove_at and swm_schnorr_prove for the same transaction, alternating, each under its own key; the claim
              under test is "about the same: same |H| and |K|"
    block     generate_payment_proofs over 8 payments per proof, beside 8 single calls, alternating
    headline  bench.py --gpus 1 --steps 20 --warmup 5: the 2^20 figure (compare with the parent's, taken in the same session)
Each figure is the median of --runs calls after a warm-up call.  There is no threshold: the figures go to the output file.  Needs
an MI355X: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARAMS = os.path.join(ROOT, "tests", "golden", "poseidon_params.json")
LIMITS = {"witness": 240, "proof": 400, "block": 400, "headline": 400}   # seconds per section


def world(height, accounts=3):
    """A ledger over a Poseidon account tree with `accounts` funded accounts -> (ledger module, parameters, state, keys, rng)."""
    from simpleworks_amd import hash as H, ledger as L, marlin as M
    rng = M.generate_rand()
    pp = L.Parameters.sample(rng, poseidon=H.PoseidonParameters.from_json(PARAMS))
    state = L.State(1 << height, pp, account_tree="poseidon")
    people = [state.sample_keys_and_register(pp, rng) for _ in range(accounts)]
    for acc, _, _ in people:
        state.update_balance(acc, 1 << 40)
    return L, pp, state, people, rng


def payments(L, pp, state, people, rng, count):
    """count valid transfers between the funded accounts, as (message, signature, sender leaf, recipient leaf)."""
    out = []
    for k in range(count):
        a, b = people[k % len(people)], people[(k + 1) % len(people)]
        tx = L.Transaction.create(pp, a[0], b[0], 1000 + k, a[2], rng)
        out.append((tx.message(), tx.signature.to_bytes(), state.id_to_account_info[a[0]].to_bytes_le(),
                    state.id_to_account_info[b[0]].to_bytes_le()))
    return out


def section_witness(args, say):
    L, pp, state, people, rng = world(args.height)
    ctx = pp.sig_params.ctx
    circuit = L.PaymentCircuit(pp.sig_params, pp.poseidon, args.height)
    say("  circuit at height %d: num_instance %d, num_witness %d, num_constraints %d" % ((args.height,) + circuit.shape()))
    for count in (1, 256):
        block = payments(L, pp, state, people, rng, count)
        call = lambda: circuit.witness_at(state.account_merkle_tree, block)
        _, flags = call()
        assert (flags == 3).all()
        wall = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
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
        say("  %3d payments: wall (copies included) %9.3f ms, kernels %8.3f ms = %8.3f us per payment, %d launches"
            % (count, statistics.median(wall), statistics.median(total), statistics.median(total) * 1e3 / count,
               sum(v[0][1] for v in per_kernel.values())))
        for name, v in sorted(per_kernel.items(), key=lambda kv: -statistics.median(x[0] for x in kv[1])):
            say("      %-24s %d launch(es) %8.3f ms" % (name, v[0][1], statistics.median(x[0] for x in v)))
    circuit.free()
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


def section_proof(args, say):
    from simpleworks_amd import marlin as M
    L, pp, state, people, rng = world(args.height)
    runs = max(5, args.runs // 2)
    tree = state.account_merkle_tree
    circuit, pk, vk = state.payment_keys(rng)
    sv_circuit, sv_pk, sv_vk = state.proof_keys(rng)
    msg, sig, sender_leaf, recipient_leaf = payments(L, pp, state, people, rng, 1)[0]
    key = sender_leaf[:64]
    proof = M.generate_payment_proof(pk, circuit, tree, msg, sig, sender_leaf, recipient_leaf, M.generate_rand())
    assert L.verify_payment(vk, [tree.root(), msg[0], msg[1], int.from_bytes(msg[2:], "little")], proof, M.generate_rand())
    assert M.verify_proof(sv_vk, [], M.MarlinProof(M.generate_schnorr_proof(sv_pk, sv_circuit, key, msg, sig, M.generate_rand())), M.generate_rand())
    a, b = _alternate(lambda: M.generate_payment_proof(pk, circuit, tree, msg, sig, sender_leaf, recipient_leaf, M.generate_rand()),
                      lambda: M.generate_schnorr_proof(sv_pk, sv_circuit, key, msg, sig, M.generate_rand()), runs)
    say("  payment proof   (%d rows, %d witnesses, 4 public inputs), witness included: %8.3f ms (min %8.3f), %d bytes"
        % (circuit.shape()[2], circuit.shape()[1], a[0], a[1], len(proof)))
    say("  signature proof (%d rows, %d witnesses, no public input),  witness included: %8.3f ms (min %8.3f)"
        % (sv_circuit.shape()[2], sv_circuit.shape()[1], b[0], b[1]))
    say("  payment - signature: %+.3f ms (%+.1f %%)" % (a[0] - b[0], 100 * (a[0] - b[0]) / b[0]))
    state.free()


def section_block(args, say):
    from simpleworks_amd import marlin as M
    L, pp, state, people, rng = world(args.height)
    runs = max(3, args.runs // 5)
    tree = state.account_merkle_tree
    circuit, pk, vk = state.payment_keys(rng)
    block = payments(L, pp, state, people, rng, 8)

    def many():
        proofs, flags = M.generate_payment_proofs(pk, circuit, tree, block, M.generate_rand())
        assert flags == [3] * len(block)
        return proofs

    def singles():
        r = M.generate_rand()
        return [M.generate_payment_proof(pk, circuit, tree, *p, r) for p in block]
    assert many() == singles()
    a, b = _alternate(many, singles, runs)
    say("  %d proofs in one call: %8.3f ms per proof (min %8.3f); %d single calls: %8.3f ms per proof (min %8.3f)"
        % (len(block), a[0] / len(block), a[1] / len(block), len(block), b[0] / len(block), b[1] / len(block)))
    state.free()


def section_headline(args, say):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True,
                         text=True, timeout=LIMITS["headline"] - 20)
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    doc = json.loads(line)
    say("  bench.py --gpus 1 --steps 20 --warmup 5: %.1f constraints/s, %.3f ms per step" % (doc["value"], doc["ms_per_step"]))
    return out.returncode


SECTIONS = {"witness": section_witness, "proof": section_proof, "block": section_block, "headline": section_headline}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=9)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "payment_time.txt"))
    ap.add_argument("--section", choices=sorted(SECTIONS), help="run one section in this process (what the parent starts)")
    args = ap.parse_args()
    if args.section:
        return SECTIONS[args.section](args, lambda text: print(text, flush=True)) or 0
    lines = ["Payment circuit over a Poseidon account tree of height %d, one MI355X, one run: medians of %d calls (proofs: fewer, see "
             "tools/payment_time.py) after a warm-up, alternating order where two things are compared" % (args.height, args.runs)]
    rc = 0
    for name in ("witness", "proof", "block", "headline"):
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

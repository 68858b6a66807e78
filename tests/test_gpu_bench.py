"""bench.py's N > 1 code path (process group, the library's RCCL communicator, ONE proof over all ranks, the `sharded` object of
the JSON line) executed on a single-GPU box: a FRESH child process with SWM_BENCH_FORCE_DIST=1 and a world of one — so that the
driver's pytest has run those lines before a multi-GPU SCALE run ever does."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.gpu
def test_bench_multi_rank_path_with_a_world_of_one():
    env = dict(os.environ)
    env.update({"SWM_BENCH_FORCE_DIST": "1", "SWM_SHARD_FORCE": "1", "RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1",
                "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(_free_port()), "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--log-n", "16",
                          "--full", "--no-cpu-baseline", "--no-drop-in"], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["value"] > 0
    sh = line["sharded"]
    assert sh and "error" not in sh, sh
    assert sh["proof_bytes_identical_on_all_ranks"] is True
    assert sh["ranks"] == 1 and sh["exchanges_per_proof"] >= 4   # the per-round all-gathers went through the library's communicator
    assert sh["ms_per_proof"] > 0
    assert sh["rccl"].startswith("librccl ") and " version " in sh["rccl"], sh["rccl"]   # which library carried the exchange, and how it was found


@pytest.mark.gpu
def test_bench_two_ranks_through_the_drivers_launcher():
    """The driver's N > 1 command line — python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1
    --master-port P bench.py --gpus 2 … — on a single-GPU box: both ranks on device 0, the collectives over gloo (the hooks
    SWM_BENCH_BACKEND / SWM_BENCH_DEVICE), the sharded leg off (two ranks of one RCCL communicator cannot share a device).  Rank 0
    must print ONE JSON line whose value is the whole job: both ranks' proofs over the max-over-ranks time."""
    pytest.importorskip("torch")
    env = dict(os.environ)
    env.update({"SWM_BENCH_BACKEND": "gloo", "SWM_BENCH_DEVICE": "0", "SWM_BENCH_NO_SHARDED": "1", "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                          "--log-n", "14", "--no-cpu-baseline", "--no-drop-in"], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines          # rank 0 only
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 3 and line["scaling"] == "weak"
    assert abs(line["value"] - 2 * (1 << 14) / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]   # whole-job units / max-over-ranks time
    assert line["sharded"] is None


@pytest.mark.gpu
def test_bench_times_an_r1cs_dump(tmp_path):
    """`bench.py --r1cs FILE`: the constraint system of an SWMR1CS1 dump (how the reference's own circuits — MerkleTreeVerificationU8 as
    ark-r1cs-std lays it out — are timed on a box without Rust) through the whole bench path: load, is_satisfied, SRS, index, proofs,
    verification of the last proof; the line names the file."""
    sys.path.insert(0, ROOT)
    from simpleworks_amd import workloads as W
    cs, _, _ = W.merkle_membership_circuit(height=4, gadget_byte_ops=16)
    path = str(tmp_path / "merkle_h4.r1cs")
    W.dump_r1cs(cs, path)
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--r1cs", path, "--steps", "3", "--warmup", "1", "--full",
                          "--no-cpu-baseline", "--no-drop-in"], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert "merkle_h4.r1cs" in line["config"]["workload"] and line["config"]["per_gpu_units"] == cs.pack().num_constraints
    assert line["value"] > 0 and line["roofline"]["frac"] > 0


@pytest.mark.gpu
def test_bench_overlapped_contexts():
    """`bench.py --overlap 2`: two contexts on the one GPU, a key and a host thread each, proving concurrently after the timed loop; the
    line carries the `overlapped` object and `value` is still the one-proof-at-a-time figure."""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--log-n", "14", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
                          "--no-drop-in", "--overlap", "2"], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    ov = line["overlapped"]
    assert ov["contexts"] == 2 and ov["proofs"] == 6 and ov["ms_per_proof"] > 0
    assert abs(line["value"] - (1 << 14) / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]


def _plain_bench(args):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "SWM_BENCH_FORCE_DIST"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=900,
                         cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_and_the_proof_it_dumps(tmp_path):
    """A plain run carries the headline and none of what --full adds; --steps is the number of timed steps; --dump-outputs writes the
    proof of the LAST timed step: the library's proof number warm-up + steps drawn from the bench's seeded inputs, and it verifies."""
    import numpy as np
    sys.path.insert(0, ROOT)
    from simpleworks_amd import marlin as M
    from simpleworks_amd import workloads as W
    out_dir = tmp_path / "out"
    line = _plain_bench(["--log-n", "12", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out_dir)])
    assert line["unit"] == "constraints/s" and line["higher_is_better"] is True and line["dtype"] and line["metric"]
    assert line["steps"] == 2 and line["warmup"] == 1
    assert abs(line["value"] - (1 << 12) / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    for k in ("roofline", "kernels_ms_per_step", "verify_ms_host", "drop_in", "drop_in_rng", "cpu_baseline"):
        assert k not in line, k
    assert sorted(os.listdir(out_dir)) == ["proof.npy"]
    got = np.load(out_dir / "proof.npy")
    assert got.dtype == np.float32
    n = 1 << 12
    rng = M.generate_rand()
    srs = M.generate_universal_srs(n, n, n, rng)
    cs, public = W.synthetic_r1cs(n, 0x1234567, 0x7654321)
    pk, vk = M.generate_proving_and_verifying_keys(srs, cs)
    srs.free()
    for _ in range(1 + 2):
        proof = M.generate_proof(cs, pk, rng)
    assert bytes(got.astype(np.uint8)) == proof.data
    assert M.verify_proof(vk, public, proof, M.generate_rand())
    pk.free()


@pytest.mark.gpu
def test_bench_msm_dump_is_the_oracles_point(tmp_path):
    """`--workload msm --dump-outputs`: the affine point of the last timed MSM equals the CPU oracle's MSM of the same seeded bases and
    scalars (the bench's scalars are Montgomery residues)."""
    import numpy as np
    from oracle_lib import Oracle, golden, h2i
    from pyref.prng import fr_array
    out_dir = tmp_path / "out"
    line = _plain_bench(["--workload", "msm", "--log-n", "12", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out_dir)])
    assert line["unit"] == "points/s" and line["steps"] == 2 and "cpu_baseline" not in line
    xy = np.load(out_dir / "msm_affine_xy.npy")
    assert xy.dtype == np.float64 and xy.shape == (2, 12)
    orc = Oracle()
    n = 1 << 12
    G = orc.points_to_mont([tuple(h2i(v) for v in golden("g1.json")["generator"])])
    bases = orc.srs_bases(n, h2i(golden("msm.json")["tau"]), G)
    want = orc.jac_to_affine_int(orc.msm(bases, orc.fr_from_mont(fr_array(n, 1000)), threads=4))
    got = orc.points_from_mont(np.ascontiguousarray(xy.astype(np.uint32)).view(np.uint64).reshape(1, 12))[0]
    assert got == want

"""The stream contract of the drop-in boundary (include/swmarlin.h: "_dev ... enqueue on the context's stream", swm_set_stream
for "an externally owned hipStream_t"): every _dev entry point on a CALLER's torch stream, queued behind work that has not run yet.

Every other test of a device form finds the queue empty when the call starts and drains it before it looks, so it cannot see a
launch or copy that is not ordered behind the context's stream, a host argument read after the call has returned, or a staging
area reused before an earlier queued call has consumed it.  Here the caller's stream `s` is kept busy by a GATE — a bounded
torch.cuda._sleep — and behind it, in stream order: the pinned-to-device copy of the input (the device input holds 0xFF bytes
until then: no field element), the library call, and a device-to-device snapshot of every output (0xFF until then).  The host then
waits for `s` alone; swm_synchronize is not called.  Work that ran ahead of `s` read 0xFF; work that was not joined back into `s`
left 0xFF in the snapshot.  The expectation is the C oracle, hashlib, the Python models and the circuit builders that the entry's
own test module uses, never a second call of the entry.

Conclusive or failed: for every entry of CONTRACT that "returns without waiting" the gate's event must still be pending when the
call returns — otherwise the test fails and says so; nothing is skipped or retried.  Arrays that index memory (CSR row pointers and
columns) are in place before the gate, so that a wrong ordering shows as wrong bytes and never as a fault; leaf indices may be
0xFF (the library reports them per item).

The gate.  Cycles per millisecond are calibrated once per module with two events around a fixed _sleep.  Each entry first runs
once ungated with the same shapes (that call grows every scratch buffer, builds every table and loads every kernel, so the gated
call allocates nothing), its host side is timed, and the gate lasts GATE_MULT times that, at least GATE_FLOOR_MS (launch latency,
the copies and Python between the gate and the call's return: well under a millisecond) and at most GATE_CAP_MS.  A gate that is
too short can only make a test fail loudly.  GATE_MULT = 20, GATE_FLOOR_MS = 20, GATE_CAP_MS = 500.  Observed on an MI355X over two
runs, host side of the warm call: 0.01 - 0.06 ms for an entry whose kernels are loaded (0.012 tree paths, 0.03 - 0.05 vec_mul, 0.03
tree build), 0.12 - 0.19 ms for the two-pass NTT, 0.5 - 1.2 ms where the warm call is the first launch of a kernel (the hashes, the
witness forms, the first batch inversion; 1.0 the two payment witnesses): gates of 20 - 24 ms; 6.8 - 7.3 ms for the module's first
NTT, which builds the size's tables (gate 135 - 145 ms).  The entries that wait take their GPU time on the host (spmv 3.3 - 3.8 ms,
MSM 1.0 - 1.1 ms, 20 tree updates 1.5 ms: gates of 65 - 75, 20 - 23 and 30 ms, which for them only have to be busy when the call
starts).  The last test prints the figures of a run (pytest -s).  The module takes about ten seconds, the keys of (f) included.

Left out: see NOT_COVERED (nothing: swm_ntt_fr_sharded_dev runs in its one-rank form)."""
import json
import os
import time

import numpy as np
import pytest

import oracle_lib as OL
from oracle_lib import Oracle, golden, h2i, p64, R
from pyref.prng import fr_array

pytestmark = pytest.mark.gpu

GATE_MULT, GATE_FLOOR_MS, GATE_CAP_MS = 20, 20.0, 500.0
ASYNC, WAITS = "returns without waiting", "waits"

# What each _dev entry point does before it returns, read from the code (csrc/*.hip) and stated in include/swmarlin.h.  An entry
# waits when it hands a host result back or must release a host buffer.
CONTRACT = {
    "swm_batch_inverse_fr_dev": ASYNC,
    "swm_blake2s_hash_dev": ASYNC,
    "swm_blake2s_witness_dev": ASYNC,
    "swm_elgamal_witness_dev": ASYNC,
    "swm_elgamal_witness_to_dev": ASYNC,
    "swm_merkle_tree_build_dev": ASYNC,
    "swm_merkle_tree_create_from_leaves_dev": ASYNC,
    "swm_merkle_tree_paths_dev": ASYNC,
    "swm_merkle_tree_update_dev": {"at most 4 distinct leaves": ASYNC, "more than 4 distinct leaves": WAITS},  # the index list goes up from the call's frame
    "swm_merkle_verify_paths_dev": ASYNC,
    "swm_merkle_witness_dev": ASYNC,
    "swm_msm_g1_dev": WAITS,                 # the result is a host value
    "swm_ntt_fr_dev": ASYNC,                 # (a size's first call builds its tables with a blocking copy)
    "swm_ntt_fr_sharded_dev": WAITS,
    "swm_payment_witness_dev": ASYNC,
    "swm_pedersen_hash_dev": ASYNC,
    "swm_pedersen_payment_witness_dev": ASYNC,
    "swm_poseidon_hash_bytes_dev": ASYNC,
    "swm_poseidon_hash_fr_dev": ASYNC,
    "swm_poseidon_witness_dev": ASYNC,
    "swm_program_witness_dev": ASYNC,
    "swm_schnorr_witness_dev": ASYNC,
    "swm_spmv_fr_dev": WAITS,                # the row statistics that pick the schedule are read back
    "swm_vec_mul_fr_dev": ASYNC,
}
NOT_COVERED = {}         # entry -> why it has no case
CASE_OF = {              # the case of (a) that runs each entry by the protocol
    "swm_batch_inverse_fr_dev": "test_a_batch_inverse", "swm_blake2s_hash_dev": "test_a_blake2s_hash",
    "swm_blake2s_witness_dev": "test_a_blake2s_witness", "swm_elgamal_witness_dev": "test_a_elgamal_witness",
    "swm_elgamal_witness_to_dev": "test_a_elgamal_witness", "swm_merkle_tree_build_dev": "test_a_merkle_tree_build",
    "swm_merkle_tree_create_from_leaves_dev": "test_a_merkle_tree_create_from_leaves", "swm_merkle_tree_paths_dev": "test_a_merkle_tree_paths",
    "swm_merkle_tree_update_dev": "test_a_merkle_tree_update", "swm_merkle_verify_paths_dev": "test_a_merkle_verify_paths",
    "swm_merkle_witness_dev": "test_a_merkle_witness", "swm_msm_g1_dev": "test_a_msm", "swm_ntt_fr_dev": "test_a_ntt",
    "swm_payment_witness_dev": "test_a_payment_witness", "swm_pedersen_hash_dev": "test_a_pedersen_hash",
    "swm_pedersen_payment_witness_dev": "test_a_pedersen_payment_witness", "swm_poseidon_hash_bytes_dev": "test_a_poseidon_hash_bytes",
    "swm_poseidon_hash_fr_dev": "test_a_poseidon_hash_fr", "swm_poseidon_witness_dev": "test_a_poseidon_witness",
    "swm_program_witness_dev": "test_a_program_witness", "swm_schnorr_witness_dev": "test_a_schnorr_witness",
    "swm_spmv_fr_dev": "test_a_spmv", "swm_vec_mul_fr_dev": "test_a_vec_mul", "swm_ntt_fr_sharded_dev": "test_a_ntt_sharded_one_rank",
}
WARM_MS = {}             # case -> host milliseconds of the warm call, gate milliseconds (printed by the last test)

POSEIDON_PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")


# ------------------------------------------------------------------------------------------------ the harness
class Ptr:
    """A torch tensor's address in the two forms the wrappers of simpleworks_amd/_lib.py take: .ptr and int()."""

    def __init__(self, t, offset=0):
        self.t = t
        self.ptr = t.data_ptr() + offset

    def __int__(self):
        return self.ptr


class _Raw:
    """Device memory owned by the library (a tree's node buffer) as a torch tensor, through __cuda_array_interface__."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


def _bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class Env:
    """The module's context on the caller's stream, and the gate."""

    def __init__(self):
        import torch
        import simpleworks_amd as swm
        self.torch = torch
        self.ctx = swm.Context(0)
        self.s = torch.cuda.Stream()
        self.s2 = torch.cuda.Stream()
        self.ctx.set_stream(self.s.cuda_stream)
        assert hasattr(torch.cuda, "_sleep"), "torch.cuda._sleep is missing: no bounded gate"
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.s):
            torch.cuda._sleep(1000000)            # loads the kernel
            e0.record()
            torch.cuda._sleep(20000000)
            e1.record()
        self.s.synchronize()
        self.cycles_per_ms = 20000000 / e0.elapsed_time(e1)

    def close(self):
        self.ctx.set_stream(None)
        self.ctx.close()

    # ---- buffers: allocated on the default stream; run() synchronises the device before its gate
    def dev(self, nbytes):
        """nbytes (at least 16) of a larger allocation: the kernels' word readers may look past an input's last byte, as the host
        forms' staging areas allow for"""
        n = max(int(nbytes), 16)
        return self.torch.empty(n + 256, dtype=self.torch.uint8, device="cuda")[:n]

    def pinned(self, a):
        return self.torch.from_numpy(_bytes(a).copy()).pin_memory()

    def resident(self, a):
        """device tensor holding a, in place before any gate"""
        t = self.dev(_bytes(a).size)
        t.copy_(self.torch.from_numpy(_bytes(a).copy()))
        self.torch.cuda.synchronize()
        return t

    def pair(self, a):
        """(device tensor of a's size, pinned copy of a): an input that goes up behind the gate"""
        n = _bytes(a).size
        return self.dev(n)[:n], self.pinned(a)

    def alias(self, ptr, nbytes):
        return self.torch.as_tensor(_Raw(ptr, nbytes), device="cuda")

    def gate(self, ms):
        """on the current stream: busy for ms milliseconds; the event after it"""
        self.torch.cuda._sleep(int(ms * self.cycles_per_ms))
        g = self.torch.cuda.Event()
        g.record()
        return g

    def gate_ms(self, warm_ms):
        return min(GATE_CAP_MS, max(GATE_FLOOR_MS, GATE_MULT * warm_ms))

    def run(self, name, ins, call, outs, mode=ASYNC, warm=None, after=None, late_outs=None, late_bytes=()):
        """One entry by the protocol.  ins: [(device tensor, pinned source)]; call(): the library entry; outs: device tensors the
        entry writes (whole tensors: guard bytes included); warm(): what to run ungated first (default: call); after(): host code
        right after the entry returns, the gate still pending; late_outs(result): device tensors known only after the call (a
        buffer the entry allocates), of late_bytes bytes each.  Returns the snapshots as numpy uint8 arrays, outs first."""
        torch, s = self.torch, self.s
        snaps = [torch.empty_like(o) for o in outs]
        late = [self.dev(n)[:n] for n in late_bytes]
        # the warm call, ungated, everything in place: its host side sizes the gate
        with torch.cuda.stream(s):
            for d, src in ins:
                d.copy_(src, non_blocking=True)
        s.synchronize()
        t0 = time.perf_counter()
        (warm or call)()
        warm_ms = (time.perf_counter() - t0) * 1e3
        s.synchronize()
        gate_ms = self.gate_ms(warm_ms)
        WARM_MS[name] = (round(warm_ms, 3), gate_ms, mode)
        for d, _ in ins:
            d.fill_(0xFF)
        for o in outs + late:
            o.fill_(0xFF)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g = self.gate(gate_ms)
            for d, src in ins:
                d.copy_(src, non_blocking=True)
            result = call()
            pending = not g.query()
            if after:
                after()
                pending = pending and not g.query()
            for snap, o in zip(snaps + late, outs + (late_outs(result) if late_outs else [])):
                snap.copy_(o)
            done = torch.cuda.Event()
            done.record()
        if mode == ASYNC:
            assert pending, ("%s: inconclusive — the gate of %.1f ms (warm call %.3f ms on the host) had ended when the call returned; "
                             "either the entry waited for the stream, against its contract, or the gate is too short" % (name, gate_ms, warm_ms))
        s.synchronize()            # the caller's stream alone: swm_synchronize is not called
        assert done.query()
        self.result = result
        return [t.cpu().numpy() for t in snaps + late]


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _same_rows(got, want, what, width=32):
    got, want = _bytes(got), _bytes(want)
    assert got.size == want.size, (what, got.size, want.size)
    if not np.array_equal(got, want):
        bad = np.nonzero((got.reshape(-1, width) != want.reshape(-1, width)).any(axis=1))[0]
        ff = int((got.reshape(-1, width)[bad] == 0xFF).all(axis=1).sum())
        raise AssertionError("%s: snapshot differs from the expectation in %d of %d rows of %d bytes, the first at %d (%d of them still 0xFF)"
                             % (what, bad.size, got.size // width, width, bad[0], ff))


def _fr(orc, n, seed, zeros=()):
    x = orc.fr_to_mont(fr_array(n, seed))
    for i in zeros:
        x[i] = 0
    return x


def _fr_mul(orc, a, b):
    out = np.empty_like(a)
    if a.shape[0]:
        orc.lib.oracle_fr_mul(p64(np.ascontiguousarray(a)), p64(np.ascontiguousarray(b)), p64(out), a.shape[0])
    return out


def _binv(orc, x):
    ref = x.copy()
    orc.lib.oracle_batch_inverse_fr(p64(ref), ref.shape[0])
    return ref


# ------------------------------------------------------------------------------------------------ (a) K1 - K4
@pytest.mark.parametrize("log_n,inverse,coset", [(10, 0, 1), (11, 1, 0), (11, 0, 1)])
def test_a_ntt(env, orc, log_n, inverse, coset):
    """2^10: one pass; 2^11: two passes (6 + 5) through ntt.tmp and the pass tables (test_gpu_ntt_edges.py's plans)."""
    x = _fr(orc, 1 << log_n, 7100 + log_n)
    d, src = env.pair(x)
    got, = env.run("ntt_fr_dev 2^%d inv=%d coset=%d" % (log_n, inverse, coset), [(d, src)],
                   lambda: env.ctx.ntt_fr_dev(Ptr(d), log_n, bool(inverse), bool(coset)), [d])
    _same_rows(got, orc.ntt(x, log_n, inverse, coset, threads=8), "ntt")


def test_a_ntt_sharded_one_rank(env, orc):
    """swm_ntt_fr_sharded_dev on a context without a sharding (one rank: both layouts are the whole vector): the plain transform,
    then a wait for the stream.  The exchange of two and more ranks needs one context per rank (test_gpu_marlin.py, test_gpu_multi.py)."""
    log_n = 11
    x = _fr(orc, 1 << log_n, 7150)
    d, src = env.pair(x)
    got, = env.run("ntt_fr_sharded_dev 2^11, one rank", [(d, src)], lambda: env.ctx.ntt_fr_sharded_dev(Ptr(d), log_n, True, False), [d], mode=WAITS)
    _same_rows(got, orc.ntt(x, log_n, 1, 0, threads=8), "sharded ntt, one rank")


def _spmv_case(orc):
    from test_gpu_spmv_plan import _matrix
    _, rowptr, col, val, z = _matrix(orc, "thresholds")
    return rowptr, col, val, z


def test_a_spmv(env, orc):
    """The "thresholds" matrix of test_gpu_spmv_plan.py.  Row pointers and columns are in place (they index memory); the
    coefficients and z go up behind the gate.  The entry reads its row statistics back: it waits."""
    rowptr, col, val, z = _spmv_case(orc)
    rows = rowptr.size - 1
    d_rp, d_col = env.resident(rowptr), env.resident(col)
    (d_val, s_val), (d_z, s_z) = env.pair(val), env.pair(z)
    d_out = env.dev(rows * 32 + 64)
    got, = env.run("spmv_fr_dev thresholds", [(d_val, s_val), (d_z, s_z)],
                   lambda: env.ctx.spmv_fr_dev(Ptr(d_rp), Ptr(d_col), Ptr(d_val), Ptr(d_z), Ptr(d_out), rows), [d_out], mode=WAITS)
    _same_rows(got[:rows * 32], orc.spmv(rowptr, col, val, z, threads=8), "spmv")
    assert (got[rows * 32:] == 0xFF).all()


@pytest.mark.parametrize("n", [2 * 4096 + 5, (1 << 18) + 4096 + 17])
def test_a_batch_inverse(env, orc, n):
    """Both chunk sizes of batch_inverse_run (the bound is 2^18 elements); zeros stay zero."""
    x = _fr(orc, n, 7200 + (n & 0xFF), zeros=(0, 17, 4096, n - 1))
    d, src = env.pair(x)
    got, = env.run("batch_inverse_fr_dev %d" % n, [(d, src)], lambda: env.ctx.batch_inverse_fr_dev(Ptr(d), n), [d])
    _same_rows(got, _binv(orc, x), "batch_inverse")


def _vec_mul_buffers(env, orc, n=1000):
    a, b = _fr(orc, n, 7301), _fr(orc, n, 7302)
    return a, b, env.pair(a), env.pair(b), env.dev(n * 32 + 64)


def test_a_vec_mul(env, orc):
    n = 1000
    a, b, (d_a, s_a), (d_b, s_b), d_out = _vec_mul_buffers(env, orc, n)
    got, = env.run("vec_mul_fr_dev 1000", [(d_a, s_a), (d_b, s_b)], lambda: env.ctx.vec_mul_fr_dev(Ptr(d_a), Ptr(d_b), Ptr(d_out), n), [d_out])
    _same_rows(got[:n * 32], _fr_mul(orc, a, b), "vec_mul")
    assert (got[n * 32:] == 0xFF).all()


@pytest.fixture(scope="module")
def msm_set(env, orc):
    """8192 powers [tau^i]G resident on the module's context, and the same rows for the oracle."""
    G = orc.points_to_mont([tuple(h2i(v) for v in golden("g1.json")["generator"])])
    bases = orc.srs_bases(8192, h2i(golden("msm.json")["tau"]), G)
    bh = env.ctx.srs_upload(bases)
    yield bases, bh
    bh.free()


def test_a_msm(env, orc, msm_set):
    """4096 points, the scalars copied in behind the gate.  The result is a host value: the entry waits.  A scalar of 0xFF bytes is
    no field element: a launch that ran ahead of the copy is refused on the device (SWM_ERR_INVALID_ARG), it cannot fault."""
    bases, bh = msm_set
    n = 4096
    sc = fr_array(n, 7401)
    d, src = env.pair(sc)
    env.run("msm_g1_dev 4096", [(d, src)], lambda: env.ctx.msm_g1_dev(bh, Ptr(d), n, False), [], mode=WAITS)
    assert orc.jac_to_affine_int(env.result) == orc.jac_to_affine_int(orc.msm(bases[:n], sc, threads=8))


# ------------------------------------------------------------------------------------------------ (a) the three hashes
def test_a_blake2s_hash(env):
    """130 items of 65 bytes: items at all four byte offsets within a word (test_gpu_random_oracle.py)."""
    from test_gpu_random_oracle import batch, digests_of
    a = batch(130, 65, seed=11)
    (d_in, src), d_out = env.pair(a), env.dev(130 * 32 + 64)
    got, = env.run("blake2s_hash_dev 130x65", [(d_in, src)], lambda: env.ctx.blake2s_hash_dev(Ptr(d_in), 65, 130, Ptr(d_out)), [d_out])
    _same_rows(got[:130 * 32], digests_of(a), "blake2s")
    assert (got[130 * 32:] == 0xFF).all()


@pytest.fixture(scope="module")
def sponge(env):
    from simpleworks_amd import hash as H
    s = H.PoseidonSponge(H.PoseidonParameters.from_json(POSEIDON_PARAMS), env.ctx)
    yield s
    s.free()


@pytest.fixture(scope="module")
def poseidon_ref():
    import poseidon_model as P
    return P.load_params(POSEIDON_PARAMS)


def _le(h):
    return int.from_bytes(bytes.fromhex(h), "little")


def _rows32(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(len(values), 32).copy()


def _poseidon_pairs(first, count):
    import poseidon_model as P
    want = [_le(h) for h in golden("poseidon.json")["compress"]]
    pairs = [P.poseidon_pair(i) for i in range(first, first + count)]
    return _rows32([v for p in pairs for v in p]), _rows32(want[first:first + count])


def test_a_poseidon_hash_fr(env, sponge):
    """The 130 two-to-one compressions of tests/golden/poseidon.json, with a status word per item."""
    elems, want = _poseidon_pairs(0, 130)
    (d_in, src), d_out, d_st = env.pair(elems), env.dev(130 * 32 + 64), env.dev(4 * 130)
    got, st = env.run("poseidon_hash_fr_dev 130x2", [(d_in, src)],
                      lambda: env.ctx.poseidon_hash_fr_dev(sponge.h, Ptr(d_in), 2, 130, 1, Ptr(d_out), Ptr(d_st)), [d_out, d_st])
    assert not st.any(), "a status word is set: an element was read before it was copied in"
    _same_rows(got[:130 * 32], want, "poseidon_hash_fr")
    assert (got[130 * 32:] == 0xFF).all()


def test_a_poseidon_hash_bytes(env, sponge, poseidon_ref):
    import poseidon_model as P
    ln, count = 55, 130
    msgs = [P.poseidon_input(ln, i) for i in range(count)]
    have = [_le(h) for h in golden("poseidon.json")["bytes"][str(ln)]]
    want = _rows32([have[i] if i < len(have) else P.hash_bytes(poseidon_ref, msgs[i]) for i in range(count)])
    (d_in, src), d_out = env.pair(np.frombuffer(b"".join(msgs), dtype=np.uint8)), env.dev(count * 32 + 64)
    got, = env.run("poseidon_hash_bytes_dev 130x55", [(d_in, src)],
                   lambda: env.ctx.poseidon_hash_bytes_dev(sponge.h, Ptr(d_in), ln, count, Ptr(d_out)), [d_out])
    _same_rows(got[:count * 32], want, "poseidon_hash_bytes")
    assert (got[count * 32:] == 0xFF).all()


@pytest.fixture(scope="module")
def crh(env):
    """LeafHash::setup then TwoToOneHash::setup from a fresh test_rng, as in test_gpu_pedersen.py, on the module's context."""
    from simpleworks_amd import hash as H, marlin as M
    rng = M.generate_rand()
    leaf = H.PedersenCRH.setup(rng, H.LEAF_WINDOWS, ctx=env.ctx)
    inner = H.PedersenCRH.setup(rng, H.TWO_TO_ONE_WINDOWS, ctx=env.ctx)
    yield leaf, inner
    leaf.free()
    inner.free()


def test_a_pedersen_hash(env, orc, crh):
    _, inner = crh
    data = np.random.default_rng(7501).integers(0, 256, size=(130, 64), dtype=np.uint8)
    (d_in, src), d_out = env.pair(data), env.dev(130 * 32 + 64)
    got, = env.run("pedersen_hash_dev 130x64", [(d_in, src)], lambda: env.ctx.pedersen_hash_dev(inner.h, Ptr(d_in), 64, 130, Ptr(d_out)), [d_out])
    _same_rows(got[:130 * 32], OL.pedersen_hash(orc.lib, inner.generators, data, threads=8), "pedersen_hash")
    assert (got[130 * 32:] == 0xFF).all()


# ------------------------------------------------------------------------------------------------ (a) tree forms
def _leaves(seed, n, leaf_len):
    return np.random.default_rng(seed).integers(0, 256, size=(n, leaf_len), dtype=np.uint8)


def _tree(orc, crh, leaves):
    return OL.merkle_tree(orc.lib, crh[0].generators, crh[1].generators, leaves, threads=8)


def _levels(nodes):
    out, off, cnt = [], 0, (len(nodes) + 1) // 2
    while cnt >= 1:
        out.append(nodes[off:off + cnt])
        off += cnt
        cnt >>= 1
    return out


def _paths(nodes, indices):
    """uint8 [count, levels, 32]: the siblings bottom up, from the oracle's nodes"""
    lv = _levels(nodes)
    return np.stack([np.stack([lv[l][(int(i) >> l) ^ 1] for l in range(len(lv) - 1)]) for i in indices])


@pytest.mark.parametrize("height,leaf_len", [(3, 1), (7, 72)])
def test_a_merkle_tree_build(env, orc, crh, height, leaf_len):
    n = 1 << (height - 1)
    leaves = _leaves(7600 + height, n, leaf_len)
    (d_in, src), d_nodes = env.pair(leaves), env.dev((2 * n - 1) * 32 + 64)
    got, = env.run("merkle_tree_build_dev h%d" % height, [(d_in, src)],
                   lambda: env.ctx.merkle_tree_build_dev(crh[0].h, crh[1].h, Ptr(d_in), leaf_len, n, Ptr(d_nodes)), [d_nodes])
    _same_rows(got[:(2 * n - 1) * 32], _tree(orc, crh, leaves), "merkle_tree_build")
    assert (got[(2 * n - 1) * 32:] == 0xFF).all()


@pytest.mark.parametrize("height,leaf_len", [(3, 72), (7, 1)])
def test_a_merkle_tree_create_from_leaves(env, orc, crh, height, leaf_len):
    """The node buffer is allocated by the call: its snapshot is taken behind the call on the caller's stream."""
    ctx = env.ctx
    n = 1 << (height - 1)
    leaves = _leaves(7700 + height, n, leaf_len)
    d_in, src = env.pair(leaves)
    made = []

    def call():
        made.append(ctx.merkle_tree_create_from_leaves_dev(crh[0].h, crh[1].h, Ptr(d_in), leaf_len, n))
        return made[-1]

    def nodes_of(h):
        ptr, count = ctx.merkle_tree_dev_nodes(h)
        assert count == 2 * n - 1
        return [env.alias(ptr, count * 32)]
    try:
        got, = env.run("merkle_tree_create_from_leaves_dev h%d" % height, [(d_in, src)], call, [], late_outs=nodes_of, late_bytes=[(2 * n - 1) * 32])
        _same_rows(got, _tree(orc, crh, leaves), "merkle_tree_create_from_leaves")
    finally:
        for h in made:
            ctx.merkle_tree_destroy(h)


def _resident_tree(crh, leaves):
    from simpleworks_amd import hash as H
    return H.DeviceMerkleTree.new(crh[0], crh[1], [int(r[0]) for r in leaves] if leaves.shape[1] == 1 else [bytes(r) for r in leaves])


def _apply(leaves, indices, new):
    out = leaves.copy()
    for i, row in zip(indices, new):
        out[int(i)] = row
    return out


def _update_case(env, orc, crh, name, indices, mode, seed, clobber=False):
    """swm_merkle_tree_update_dev on a tree of 64 leaves of 72 bytes (height 7): the indices on the host, the new leaves copied in
    behind the gate.  The warm call updates a second tree of the same shape.  clobber: the caller's index array is overwritten with
    0xFF bytes as soon as the call has returned."""
    ctx = env.ctx
    base = _leaves(seed, 64, 72)
    new = _leaves(seed + 1, len(indices), 72)
    tree, other = _resident_tree(crh, base), _resident_tree(crh, base)
    try:
        ptr, count = ctx.merkle_tree_dev_nodes(tree.h)
        nodes = env.alias(ptr, count * 32)
        d_new, src = env.pair(new)
        idx = np.array(indices, dtype=np.uint64)
        warm_idx = idx.copy()

        def after():
            idx[:] = np.uint64(0xFFFFFFFFFFFFFFFF)
        got, = env.run(name, [(d_new, src)], lambda: ctx.merkle_tree_update_dev(tree.h, idx, Ptr(d_new), 72), [], mode=mode,
                       warm=lambda: ctx.merkle_tree_update_dev(other.h, warm_idx, Ptr(d_new), 72), after=after if clobber else None,
                       late_outs=lambda _: [nodes], late_bytes=[count * 32])
        _same_rows(got, _tree(orc, crh, _apply(base, indices, new)), name)
    finally:
        tree.free()
        other.free()


@pytest.mark.parametrize("indices,mode", [([7, 50], ASYNC), ([3, 9, 9, 40, 63, 3], ASYNC), (list(range(3, 63, 3)), WAITS)])
def test_a_merkle_tree_update(env, orc, crh, indices, mode):
    """2 leaves; 6 updates of 4 distinct leaves (the rule counts touched leaves); 20 leaves: an index list goes up, the entry waits."""
    _update_case(env, orc, crh, "merkle_tree_update_dev %d updates" % len(indices), indices, mode, 7800 + len(indices))


def test_a_merkle_tree_paths(env, orc, crh):
    leaves = _leaves(7900, 16, 1)
    tree = _resident_tree(crh, leaves)
    try:
        indices = np.array([0, 15, 6, 6, 9], dtype=np.uint64)
        (d_idx, src), d_sib = env.pair(indices), env.dev(5 * 4 * 32 + 64)
        got, = env.run("merkle_tree_paths_dev h5", [(d_idx, src)], lambda: env.ctx.merkle_tree_paths_dev(tree.h, Ptr(d_idx), 5, Ptr(d_sib)), [d_sib])
        _same_rows(got[:5 * 4 * 32], _paths(_tree(orc, crh, leaves), indices), "merkle_tree_paths")
        assert (got[5 * 4 * 32:] == 0xFF).all()
    finally:
        tree.free()


def test_a_merkle_verify_paths(env, orc, crh):
    """Height 7, 72-byte leaves, one root for all paths: four good paths and one whose second sibling has a flipped bit."""
    leaves = _leaves(8000, 64, 72)
    nodes = _tree(orc, crh, leaves)
    indices = np.array([0, 63, 21, 42, 21], dtype=np.uint64)
    sib = _paths(nodes, indices)
    sib[4, 1, 0] ^= 1
    ins = [env.pair(nodes[-1]), env.pair(leaves[indices.astype(np.int64)]), env.pair(indices), env.pair(sib)]
    d_ok, d_st = env.dev(16), env.dev(32)
    ok, st = env.run("merkle_verify_paths_dev h7", ins,
                     lambda: env.ctx.merkle_verify_paths_dev(crh[0].h, crh[1].h, 7, Ptr(ins[0][0]), 0, Ptr(ins[1][0]), 72, Ptr(ins[2][0]),
                                                             Ptr(ins[3][0]), 5, Ptr(d_ok), Ptr(d_st)), [d_ok, d_st])
    assert st[:20].view(np.uint32).tolist() == [0] * 5, "status: an input was read before it was copied in"
    assert ok[:5].tolist() == [1, 1, 1, 1, 0] and (ok[5:] == 0xFF).all() and (st[20:] == 0xFF).all()


# ------------------------------------------------------------------------------------------------ (a) witness forms
class _WitnessOnly:
    """The builders' vocabulary, keeping the assignment and dropping the rows (as in the circuits' own test modules)."""

    def __init__(self):
        self.witness = []
        self.public = []

    @staticmethod
    def one():
        return ("i", 0)

    def new_input_variable(self, value):
        self.public.append(int(value) % R)
        return ("i", len(self.public))

    def new_witness_variable(self, value):
        self.witness.append(int(value) % R)
        return ("w", len(self.witness) - 1)

    def enforce_constraint(self, a, b, c):
        pass


def _limbs(cs):
    from simpleworks_amd import marlin as M
    return M._to_mont_limbs(cs.witness)


@pytest.fixture(scope="module")
def merkle_params(env):
    """The reference's configuration with the committed fixtures' generators (test_gpu_merkle_witness.py), on the module's context."""
    from simpleworks_amd import workloads as W
    p = W.MerkleParams()
    p.crh(env.ctx)
    return p


def test_a_merkle_witness(env, merkle_params):
    """Height 2 with 16 byte operations, three paths (test_gpu_merkle_witness.py's device case), roots and status."""
    from simpleworks_amd import hash as H, marlin as M, workloads as W
    from test_gpu_merkle_witness import _oracle
    c = H.MerkleCircuit(*merkle_params.crh(env.ctx), 2, 16)
    try:
        nw = c.shape()[1]
        g = W._SplitMix(5)
        leaves, indices = [0x11, 0x22, 0x33], [0, 1, 1]
        paths = [[g.fr()], [g.fr()], [g.fr()]]
        want = [_oracle(M, W, merkle_params, leaves[i], indices[i], paths[i], 16) for i in range(3)]
        ins = [env.pair(np.array(leaves, dtype=np.uint8)), env.pair(np.array(indices, dtype=np.uint64)),
               env.pair(_rows32([s for p in paths for s in p]))]
        d_w, d_roots, d_st = env.dev(3 * nw * 32 + 64), env.dev(96), env.dev(16)
        w, roots, st = env.run("merkle_witness_dev 3", ins,
                               lambda: env.ctx.merkle_witness_dev(c.h, Ptr(ins[0][0]), Ptr(ins[1][0]), Ptr(ins[2][0]), 3, Ptr(d_w), Ptr(d_roots),
                                                                  Ptr(d_st)), [d_w, d_roots, d_st])
        assert st[:12].view(np.uint32).tolist() == [0, 0, 0]
        _same_rows(w[:3 * nw * 32], np.concatenate([x[0] for x in want]), "merkle_witness")
        _same_rows(roots[:96], _rows32([x[2] for x in want]), "merkle_witness roots")
        assert (w[3 * nw * 32:] == 0xFF).all()
    finally:
        c.free()


@pytest.fixture(scope="module")
def mixed(env):
    import program_model as PM
    from simpleworks_amd import program as PG
    c = PG.ProgramCircuit(PM.mixed_program(), env.ctx)
    yield c
    c.free()


def _program_batch(mixed, count, seed):
    """(input rows, the builder's witnesses, the outputs' bytes) of the mixed program of test_gpu_program.py"""
    import program_model as PM
    from simpleworks_amd import marlin as M, program as PG, workloads as W
    rows = PM.mixed_inputs(count, seed=seed)
    a = PG.pack_inputs(mixed.tape, [p for p, _ in rows], [s for _, s in rows])
    want = []
    for pub, priv in rows:
        cs = M.ConstraintSystem()
        W.build_program(cs, mixed.tape, pub, priv)
        want.append(M._to_mont_limbs(cs.witness))
    outs = [PM.mixed_eval(pub, priv)[0] for pub, priv in rows]
    return a, np.concatenate(want), outs


def _program_check(mixed, count, w, out, st, want, outs, what):
    from simpleworks_amd import program as PG
    nw, ob = mixed.shape()[1], mixed.layout["output_bytes"]
    assert not st[:count].any(), what
    _same_rows(w[:count * nw * 32], want, what)
    assert PG.unpack_outputs(mixed.tape, out[:count * ob].reshape(count, ob)) == outs, what
    assert (w[count * nw * 32:] == 0xFF).all() and (out[count * ob:] == 0xFF).all() and (st[count:] == 0xFF).all(), what


def test_a_program_witness(env, mixed):
    """65 executions of the mixed program: one past the wave of the lane-per-item kernel."""
    count = 65
    a, want, outs = _program_batch(mixed, count, 5)
    nw, ob = mixed.shape()[1], mixed.layout["output_bytes"]
    (d_in, src), d_w, d_out, d_st = env.pair(a), env.dev(count * nw * 32 + 64), env.dev(count * ob + 64), env.dev(count + 64)
    w, out, st = env.run("program_witness_dev 65", [(d_in, src)], lambda: mixed.witness_dev(Ptr(d_in), count, Ptr(d_w), Ptr(d_out), Ptr(d_st)),
                         [d_w, d_out, d_st])
    _program_check(mixed, count, w, out, st, want, outs, "program_witness")


def test_a_blake2s_witness(env):
    """Three items of 65 bytes: two blocks each, items 1 and 2 off a word boundary."""
    from simpleworks_amd import random_oracle as RO, workloads as W
    from test_gpu_random_oracle import batch, digests_of
    count, length = 3, 65
    a = batch(count, length, seed=4)
    nw = RO.Blake2sCircuit(length, env.ctx).shape()[1]
    want = []
    for row in a:
        cs = _WitnessOnly()
        W.build_blake2s_hash(cs, row.tobytes())
        want.append(_limbs(cs))
    # items lie back to back: 65-byte items need a 4-byte aligned base only
    (d_in, src), d_w, d_dg = env.pair(a), env.dev(count * nw * 32 + 64), env.dev(count * 32 + 64)
    w, dg = env.run("blake2s_witness_dev 3x65", [(d_in, src)], lambda: env.ctx.blake2s_witness_dev(Ptr(d_in), length, count, Ptr(d_w), Ptr(d_dg)),
                    [d_w, d_dg])
    _same_rows(w[:count * nw * 32], np.concatenate(want), "blake2s_witness")
    _same_rows(dg[:count * 32], digests_of(a), "blake2s_witness digests")
    assert (w[count * nw * 32:] == 0xFF).all() and (dg[count * 32:] == 0xFF).all()


def test_a_poseidon_witness(env, sponge):
    """65 items of 11 bytes, the bytes form (test_gpu_poseidon_circuit.py), outputs and status."""
    import poseidon_model as P
    from simpleworks_amd import hash as H, workloads as W
    count, ln = 65, 11
    c = H.PoseidonCircuit(sponge, input_len=ln)
    try:
        nw = c.shape()[1]
        msgs = [P.poseidon_input(ln, i) for i in range(count)]
        want, digests = [], []
        for m in msgs:
            cs = _WitnessOnly()
            public = W.build_poseidon_hash(cs, sponge.params, data=m, elements=None, n_out=1)
            want.append(_limbs(cs))
            digests += public
        (d_in, src), d_w, d_out, d_st = env.pair(np.frombuffer(b"".join(msgs), dtype=np.uint8)), env.dev(count * nw * 32 + 64), \
            env.dev(count * 32 + 64), env.dev(4 * count)
        w, out, st = env.run("poseidon_witness_dev 65x11", [(d_in, src)],
                             lambda: env.ctx.poseidon_witness_dev(c.h, Ptr(d_in), count, Ptr(d_w), Ptr(d_out), Ptr(d_st)), [d_w, d_out, d_st])
        assert not st.any()
        _same_rows(w[:count * nw * 32], np.concatenate(want), "poseidon_witness")
        _same_rows(out[:count * 32], _rows32(digests), "poseidon_witness outputs")
        assert (w[count * nw * 32:] == 0xFF).all() and (out[count * 32:] == 0xFF).all()
    finally:
        c.free()


@pytest.fixture(scope="module")
def sig_params(env):
    from simpleworks_amd import schnorr
    p = schnorr.Parameters(ctx=env.ctx)
    yield p
    p.free()


def test_a_schnorr_witness(env, sig_params):
    """Three unsalted signatures over the empty message (fixture items 0, 14, 28), the second one under the first one's key: ok = 1, 0, 1."""
    from simpleworks_amd import schnorr as SCH, workloads as W
    G = golden("schnorr.json")
    items = []
    for i in (0, 14, 28):
        v = G["valid"][i]
        assert not v["salted"] and v["message"] == ""
        items.append((bytes.fromhex(v["public_key"]), bytes.fromhex(v["signature"])))
    items[1] = (items[0][0], items[1][1])
    c = SCH.SchnorrCircuit(sig_params, 0)
    try:
        nw = c.shape()[1]
        want = []
        for key, sig in items:
            cs = _WitnessOnly()
            W.build_schnorr_verification(cs, W.ED_GENERATOR, None, (int.from_bytes(key[:32], "little"), int.from_bytes(key[32:], "little")), b"", sig)
            want.append(_limbs(cs))
        ins = [env.pair(np.frombuffer(b"".join(k for k, _ in items), dtype=np.uint8)), env.pair(np.frombuffer(b"".join(s for _, s in items), dtype=np.uint8))]
        d_w, d_ok, d_st = env.dev(3 * nw * 32 + 64), env.dev(16), env.dev(16)
        w, ok, st = env.run("schnorr_witness_dev 3", ins,
                            lambda: env.ctx.schnorr_witness_dev(c.h, Ptr(ins[0][0]), None, Ptr(ins[1][0]), 3, Ptr(d_w), Ptr(d_ok), Ptr(d_st)),
                            [d_w, d_ok, d_st])
        assert st[:12].view(np.uint32).tolist() == [0, 0, 0] and ok[:3].tolist() == [1, 0, 1] and (ok[3:] == 0xFF).all()
        _same_rows(w[:3 * nw * 32], np.concatenate(want), "schnorr_witness")
        assert (w[3 * nw * 32:] == 0xFF).all()
    finally:
        c.free()


@pytest.mark.parametrize("resident", [False, True])
def test_a_elgamal_witness(env, resident):
    """Three encryptions of tests/golden/elgamal.json, per-item keys (swm_elgamal_witness_dev) and under one resident key
    (swm_elgamal_witness_to_dev)."""
    import elgamal_model as E
    from simpleworks_amd import elgamal as EG, workloads as W
    G = golden("elgamal.json")
    generator = E.point_from_bytes(bytes.fromhex(G["generator"]))
    items = [tuple(bytes.fromhex(G["valid"][i][k]) for k in ("public_key", "message", "randomness")) for i in range(3)]
    if resident:
        items = [(items[0][0],) + it[1:] for it in items]
    params = EG.Parameters(generator, env.ctx)
    circuit = EG.ElGamalCircuit(params)
    key = EG.ResidentKey(E.point_from_bytes(items[0][0]), env.ctx) if resident else None
    try:
        nw = circuit.shape()[1]
        want, cts = [], []
        for k, m, r in items:
            cs = _WitnessOnly()
            public = W.build_elgamal_encryption(cs, generator, E.point_from_bytes(k), E.point_from_bytes(m), r)
            want.append(_limbs(cs))
            cts.append(b"".join(v.to_bytes(32, "little") for v in public[2:]))
        cols = [np.frombuffer(b"".join(it[j] for it in items), dtype=np.uint8) for j in range(3)]
        ins = [env.pair(c) for c in cols]
        d_w, d_ct, d_st = env.dev(3 * nw * 32 + 64), env.dev(3 * 128 + 64), env.dev(16)
        used = ins[1:] if resident else ins
        w, ct, st = env.run("elgamal_witness%s_dev 3" % ("_to" if resident else ""), used,
                            lambda: env.ctx.elgamal_witness_dev(circuit.h, None if resident else Ptr(ins[0][0]), Ptr(ins[1][0]), Ptr(ins[2][0]), 3,
                                                                Ptr(d_w), Ptr(d_ct), Ptr(d_st), key_handle=key.h if resident else None),
                            [d_w, d_ct, d_st])
        assert st[:12].view(np.uint32).tolist() == [0, 0, 0]
        _same_rows(w[:3 * nw * 32], np.concatenate(want), "elgamal_witness")
        _same_rows(ct[:3 * 128], np.frombuffer(b"".join(cts), dtype=np.uint8), "elgamal ciphertexts")
        assert (w[3 * nw * 32:] == 0xFF).all() and (ct[3 * 128:] == 0xFF).all()
    finally:
        if key:
            key.free()
        circuit.free()
        params.free()


def _payment_run(env, name, call_dev, circuit, ps, want, roots):
    """The two payment device forms share their argument list: messages, signatures, the two leaves and the two sibling arrays go up
    behind the gate; witness, flags, status and the two walked roots are snapshot."""
    n, nw = len(ps), circuit.shape()[1]
    col = lambda k, width: np.frombuffer(b"".join(p[k] for p in ps), dtype=np.uint8).reshape(n, width)
    ins = [env.pair(col("message", 10)), env.pair(col("signature", 64)), env.pair(col("sender_leaf", 72)), env.pair(col("recipient_leaf", 72)),
           env.pair(np.stack([_rows32(p["sender_path"]) for p in ps])), env.pair(np.stack([_rows32(p["recipient_path"]) for p in ps]))]
    d_w, d_fl, d_st, d_rs, d_rr = env.dev(n * nw * 32 + 64), env.dev(n + 15), env.dev(4 * n), env.dev(32 * n), env.dev(32 * n)
    w, fl, st, rs, rr = env.run(name, ins, lambda: call_dev(circuit.h, None, *[Ptr(d) for d, _ in ins], n, Ptr(d_w), Ptr(d_fl), Ptr(d_st), Ptr(d_rs),
                                                          Ptr(d_rr)), [d_w, d_fl, d_st, d_rs, d_rr])
    assert not st[:4 * n].any(), name
    _same_rows(w[:n * nw * 32], np.concatenate(want), name)
    assert (w[n * nw * 32:] == 0xFF).all() and (fl[n:] == 0xFF).all()
    _same_rows(rs, _rows32([r[0] for r in roots]), name + " sender roots")
    _same_rows(rr, _rows32([r[1] for r in roots]), name + " recipient roots")
    return fl[:n].tolist()


def test_a_payment_witness(env, sponge, sig_params, poseidon_ref):
    """Three payments of tests/payment_model.py at height 4 over the Poseidon account tree, by their siblings (no resident tree)."""
    import payment_model as PM
    import poseidon_tree_model as T
    from simpleworks_amd import ledger as L, workloads as W
    names = ("valid", "whole balance", "blank recipient")
    _, levels = PM.ledger(poseidon_ref, 4, None)
    ps = [p for p in PM.payments(poseidon_ref, 4, None) if p["name"] in names]
    assert len(ps) == 3
    circuit = L.PaymentCircuit(sig_params, sponge, 4)
    try:
        want = []
        for p in ps:
            cs = _WitnessOnly()
            public = W.build_payment(cs, PM.S.GENERATOR, None, sponge.params, 4, p["message"], p["signature"], p["sender_leaf"], p["sender_path"],
                                     p["recipient_leaf"], p["recipient_path"])
            assert public == p["public"]
            want.append(_limbs(cs))
        root = levels[-1][0]
        roots = [(root, T.root_of(poseidon_ref, p["recipient_leaf"], p["message"][1], p["recipient_path"]) if p["wrong"] == "recipient" else root)
                 for p in ps]
        flags = _payment_run(env, "payment_witness_dev 3", env.ctx.payment_witness_dev, circuit, ps, want, roots)
        assert flags == [p["flag"] for p in ps]
    finally:
        circuit.free()


def test_a_pedersen_payment_witness(env, sig_params, merkle_params):
    """Height 3 over the reference's Pedersen account tree (test_gpu_pedersen_payment.py): index 0 pays the last leaf, the last leaf
    pays index 0, and index 0 pays again."""
    import pedersen_payment_model as PM
    from simpleworks_amd import hash as H, ledger as L
    leaf, inner = merkle_params.crh(env.ctx)
    height, last, secrets = 3, 3, (1234567, 1234584)
    leaves = {0: PM.leaf(secrets[0], 1000), last: PM.leaf(secrets[1], 5)}
    tree = H.DeviceMerkleTree.blank(leaf, inner, height, 72)
    circuit = L.PedersenPaymentCircuit(sig_params, leaf, inner, height)
    try:
        tree.update_many(sorted(leaves), [leaves[i] for i in sorted(leaves)])
        root = tree.root()
        pay = lambda secret, a, b, amount: PM.payment(None, leaves, secret, a, b, amount, paths=(root, tree.generate_proof(a), tree.generate_proof(b)))
        ps = [pay(secrets[0], 0, last, 300), pay(secrets[1], last, 0, 5), pay(secrets[0], 0, last, 1)]
        want = []
        for p in ps:
            cs = _WitnessOnly()
            public = PM.build(merkle_params, height, p, cs=cs)[1]
            assert public == cs.public and public[0] == root
            want.append(_limbs(cs))
        flags = _payment_run(env, "pedersen_payment_witness_dev 3", env.ctx.pedersen_payment_witness_dev, circuit, ps, want, [(root, root)] * 3)
        assert flags == [3, 3, 3]
    finally:
        circuit.free()
        tree.free()


# ------------------------------------------------------------------------------------------------ (b) two calls behind one gate
def test_b_two_ntts(env, orc):
    """The same transform twice, back to back, on two vectors: both calls share ntt.tmp and the pass tables, and the second is
    queued before the first has run."""
    log_n = 11
    x, y = _fr(orc, 1 << log_n, 8101), _fr(orc, 1 << log_n, 8102)
    (d_x, s_x), (d_y, s_y) = env.pair(x), env.pair(y)

    def call():
        env.ctx.ntt_fr_dev(Ptr(d_x), log_n, False, True)
        env.ctx.ntt_fr_dev(Ptr(d_y), log_n, False, True)
    gx, gy = env.run("2 x ntt_fr_dev 2^11", [(d_x, s_x), (d_y, s_y)], call, [d_x, d_y])
    _same_rows(gx, orc.ntt(x, log_n, 0, 1, threads=8), "first ntt")
    _same_rows(gy, orc.ntt(y, log_n, 0, 1, threads=8), "second ntt")


def test_b_two_spmvs(env, orc):
    """One matrix, two coefficient and z vectors, separate outputs.  The entry waits, so the first call has run when the second
    starts: what is held here is that its pooled temporaries come back clean behind a busy stream."""
    rowptr, col, val, z = _spmv_case(orc)
    rows = rowptr.size - 1
    val2, z2 = _fr(orc, val.shape[0], 8201), _fr(orc, z.shape[0], 8202)
    d_rp, d_col = env.resident(rowptr), env.resident(col)
    ins = [env.pair(val), env.pair(z), env.pair(val2), env.pair(z2)]
    o1, o2 = env.dev(rows * 32), env.dev(rows * 32)

    def call():
        env.ctx.spmv_fr_dev(Ptr(d_rp), Ptr(d_col), Ptr(ins[0][0]), Ptr(ins[1][0]), Ptr(o1), rows)
        env.ctx.spmv_fr_dev(Ptr(d_rp), Ptr(d_col), Ptr(ins[2][0]), Ptr(ins[3][0]), Ptr(o2), rows)
    g1, g2 = env.run("2 x spmv_fr_dev", ins, call, [o1, o2], mode=WAITS)
    _same_rows(g1, orc.spmv(rowptr, col, val, z, threads=8), "first spmv")
    _same_rows(g2, orc.spmv(rowptr, col, val2, z2, threads=8), "second spmv")


def test_b_two_poseidon_hashes(env, sponge):
    (e1, w1), (e2, w2) = _poseidon_pairs(0, 65), _poseidon_pairs(65, 65)
    ins = [env.pair(e1), env.pair(e2)]
    o1, o2 = env.dev(65 * 32), env.dev(65 * 32)

    def call():
        env.ctx.poseidon_hash_fr_dev(sponge.h, Ptr(ins[0][0]), 2, 65, 1, Ptr(o1), None)
        env.ctx.poseidon_hash_fr_dev(sponge.h, Ptr(ins[1][0]), 2, 65, 1, Ptr(o2), None)
    g1, g2 = env.run("2 x poseidon_hash_fr_dev 65x2", ins, call, [o1, o2])
    _same_rows(g1, w1, "first poseidon")
    _same_rows(g2, w2, "second poseidon")


def test_b_two_program_witnesses(env, mixed):
    count = 5
    (a1, want1, outs1), (a2, want2, outs2) = _program_batch(mixed, count, 6), _program_batch(mixed, count, 7)
    assert not np.array_equal(a1, a2)
    nw, ob = mixed.shape()[1], mixed.layout["output_bytes"]
    ins = [env.pair(a1), env.pair(a2)]
    outs = [env.dev(count * nw * 32 + 64), env.dev(count * ob + 64), env.dev(count + 64), env.dev(count * nw * 32 + 64), env.dev(count * ob + 64),
            env.dev(count + 64)]

    def call():
        mixed.witness_dev(Ptr(ins[0][0]), count, Ptr(outs[0]), Ptr(outs[1]), Ptr(outs[2]))
        mixed.witness_dev(Ptr(ins[1][0]), count, Ptr(outs[3]), Ptr(outs[4]), Ptr(outs[5]))
    got = env.run("2 x program_witness_dev 5", ins, call, outs)
    _program_check(mixed, count, got[0], got[1], got[2], want1, outs1, "first program_witness")
    _program_check(mixed, count, got[3], got[4], got[5], want2, outs2, "second program_witness")


def test_b_two_tree_updates(env, orc, crh):
    """Two updates of 2 leaves each on one tree, the second touching a leaf of the first: the tree is what the four updates give in
    order."""
    ctx = env.ctx
    base = _leaves(8301, 64, 72)
    new1, new2 = _leaves(8302, 2, 72), _leaves(8303, 2, 72)
    i1, i2 = np.array([7, 50], dtype=np.uint64), np.array([50, 12], dtype=np.uint64)
    tree, other = _resident_tree(crh, base), _resident_tree(crh, base)
    try:
        ptr, count = ctx.merkle_tree_dev_nodes(tree.h)
        nodes = env.alias(ptr, count * 32)
        ins = [env.pair(new1), env.pair(new2)]

        def both(h):
            def call():
                ctx.merkle_tree_update_dev(h, i1, Ptr(ins[0][0]), 72)
                ctx.merkle_tree_update_dev(h, i2, Ptr(ins[1][0]), 72)
            return call
        got, = env.run("2 x merkle_tree_update_dev 2", ins, both(tree.h), [], warm=both(other.h), late_outs=lambda _: [nodes],
                       late_bytes=[count * 32])
        _same_rows(got, _tree(orc, crh, _apply(_apply(base, i1, new1), i2, new2)), "two updates")
    finally:
        tree.free()
        other.free()


# ------------------------------------------------------------------------------------------------ (c) host arguments are not retained
def test_c_update_indices_may_be_overwritten_once_the_call_has_returned(env, orc, crh):
    """include/swmarlin.h: "the library never retains host pointers".  swm_merkle_tree_update_dev with at most 4 leaves is the one
    _dev entry that takes a host array beside device data and returns without waiting: its index array is filled with 0xFF bytes
    while the gate is still pending, and the tree still equals a rebuild."""
    _update_case(env, orc, crh, "merkle_tree_update_dev 4 updates, indices overwritten", [63, 0, 31, 32], ASYNC, 8400, clobber=True)


# ------------------------------------------------------------------------------------------------ (d) swm_set_stream itself
def _vec_mul_sync(env, orc, seed, n=1000):
    """vec_mul_fr_dev, drained before and after: the result"""
    torch = env.torch
    a, b = _fr(orc, n, seed), _fr(orc, n, seed + 1)
    d_a, d_b, d_out = env.resident(a), env.resident(b), env.dev(n * 32)
    env.ctx.vec_mul_fr_dev(Ptr(d_a), Ptr(d_b), Ptr(d_out), n)
    env.ctx.synchronize()
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), _fr_mul(orc, a, b)


def test_d_set_stream_waits_for_pending_work_and_lets_go_of_the_callers_stream(env, orc):
    torch, ctx, s = env.torch, env.ctx, env.s
    n = 1000
    a, b, (d_a, s_a), (d_b, s_b), d_out = _vec_mul_buffers(env, orc, n)
    log_n = 11
    x = _fr(orc, 1 << log_n, 8501)
    d_x = env.resident(x)
    snap = torch.empty_like(d_out)
    got, _ = _vec_mul_sync(env, orc, 8510)            # warm: kernels loaded
    d_warm = env.resident(x)
    ctx.ntt_fr_dev(Ptr(d_warm), log_n, False, False)  # ... and this size's tables built
    ctx.synchronize()
    d_a.fill_(0xFF)
    d_b.fill_(0xFF)
    d_out.fill_(0xFF)
    torch.cuda.synchronize()
    try:
        # 1. NULL with work pending behind a gate: returns only when that work is done
        with torch.cuda.stream(s):
            g = env.gate(GATE_FLOOR_MS)
            d_a.copy_(s_a, non_blocking=True)
            d_b.copy_(s_b, non_blocking=True)
            ctx.vec_mul_fr_dev(Ptr(d_a), Ptr(d_b), Ptr(d_out), n)
            assert not g.query(), "inconclusive: the gate had ended before swm_set_stream was called"
            snap.copy_(d_out)
            done = torch.cuda.Event()
            done.record()
            ctx.set_stream(None)
            assert done.query(), "swm_set_stream(NULL) returned while work of the context was pending on the caller's stream"
        _same_rows(snap.cpu().numpy()[:n * 32], _fr_mul(orc, a, b), "vec_mul before swm_set_stream(NULL)")
        # 2. on its own stream again, the library does not touch the caller's: `s` is gated, the call and swm_synchronize return
        with torch.cuda.stream(s):
            g = env.gate(GATE_FLOOR_MS)
        ctx.ntt_fr_dev(Ptr(d_x), log_n, False, False)
        ctx.synchronize()
        pending = not g.query()
        s.synchronize()
        assert pending, "swm_synchronize on the library's own stream returned only after the caller's gated stream had drained"
        _same_rows(d_x.cpu().numpy(), orc.ntt(x, log_n, 0, 0, threads=8), "ntt on the library's own stream")
    finally:
        s.synchronize()
        ctx.set_stream(s.cuda_stream)


def test_d_setting_the_same_stream_twice_and_switching_streams_changes_no_result(env, orc):
    ctx, s, s2 = env.ctx, env.s, env.s2
    try:
        for k, stream in enumerate((s, s, s2, s, None, s2, s2)):
            ctx.set_stream(stream.cuda_stream if stream is not None else None)
            got, want = _vec_mul_sync(env, orc, 8600 + 2 * k)
            _same_rows(got, want, "vec_mul after switch %d" % k)
    finally:
        ctx.set_stream(s.cuda_stream)


# ------------------------------------------------------------------------------------------------ (e) the asynchronous MSM lanes
@pytest.mark.parametrize("defer", ["on", "off"])
def test_e_msm_jobs_on_the_callers_stream(env, orc, msm_set, defer):
    """swm_selftest_msm_jobs with pipe_min = 1: 4096-point jobs take the three-stream pipeline (sort | accumulation | bucket stage on
    auxiliary streams forked from the context's stream).  One plain job and one twin pair (below twin_min the follower keeps its own
    sort: the roles still shape the lanes), bucket stages deferred to the round's joint launch and not.  The call stages its host
    scalars on the context's stream, behind the gate; a warm call with OTHER scalars leaves those in the staging buffer, so a lane
    that ran ahead of the caller's stream computes the wrong sum.  Against the C oracle, as in test_gpu_msm_async.py."""
    torch, ctx, s = env.torch, env.ctx, env.s
    bases, bh = msm_set
    n = 4096
    vecs = [fr_array(n, 8701), fr_array(n, 8702)]
    other = [fr_array(n, 8711), fr_array(n, 8712)]
    jobs = [(0, 0, 0, n, None), (0, 100, 1, n, "lead"), (0, 4096, 1, n, "follow")]
    ctx.selftest_msm_jobs([bh], other, jobs, defer_tail=defer, pipe_min=1)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        env.gate(GATE_FLOOR_MS)
        out, _ = ctx.selftest_msm_jobs([bh], vecs, jobs, defer_tail=defer, pipe_min=1)
    s.synchronize()
    for k, (_, off, v, cnt, _) in enumerate(jobs):
        assert orc.jac_to_affine_int(out[k]) == orc.jac_to_affine_int(orc.msm(np.ascontiguousarray(bases[off:off + cnt]), vecs[v], threads=8)), \
            "job %d (defer %s)" % (k, defer)


# ------------------------------------------------------------------------------------------------ (f) the prover
def _gated_proof(env, prove):
    """prove() with the caller's stream busy when it starts (the prover hands bytes back: it waits)"""
    with env.torch.cuda.stream(env.s):
        env.gate(GATE_FLOOR_MS)
        out = prove()
    env.s.synchronize()
    return out


@pytest.mark.parametrize("name,fixture", [("synthetic_8", "marlin.json"), ("synthetic_2p12", "marlin_large.json")])
def test_f_golden_proofs_on_a_callers_stream_and_after_restoring_the_own_stream(env, name, fixture):
    """The fixtures' proof bytes with the context on the caller's gated stream (synthetic_8: the pinned small-proof upload and the
    one-stream MSM lanes; synthetic_2p12: the pooled path), and again after swm_set_stream(NULL)."""
    from simpleworks_amd import marlin as M, serialization as S, workloads as W
    case = golden(fixture)[name]
    rng = M.generate_rand()
    srs = M.generate_universal_srs(*case["srs"], rng, ctx=env.ctx)
    build = W.synthetic_circuit if fixture == "marlin.json" else lambda *a: W.synthetic_r1cs(*a)[0]
    cs = build(case["num_constraints"], h2i(case["a"]), h2i(case["b"]))
    pk, vk = M.generate_proving_and_verifying_keys(srs, cs)
    pos = rng.word_pos()
    try:
        prove = lambda: S.serialize_proof(M.generate_proof(cs, pk, M.rng_from_chacha(M.TEST_RNG_SEED, pos))).hex()
        assert S.serialize_verifying_key(vk).hex() == case["vk"]
        assert _gated_proof(env, prove) == case["proof"], "on the caller's stream"
        assert _gated_proof(env, prove) == case["proof"], "on the caller's stream, second proof"
        env.ctx.set_stream(None)
        assert _gated_proof(env, prove) == case["proof"], "on the library's own stream"
    finally:
        env.s.synchronize()
        env.ctx.set_stream(env.s.cuda_stream)
        pk.free()
        srs.free()


def test_f_program_proof_from_the_device_witness_on_a_callers_stream(env, mixed):
    """generate_program_proof for the mixed program of test_gpu_program.py: the witness is synthesised on the device and reaches the
    prover by a device-to-device copy.  Byte-identical to the proof of the builder's system, on the caller's gated stream and on the
    library's own."""
    import program_model as PM
    from simpleworks_amd import marlin as M, serialization as S, workloads as W
    pub, priv = PM.mixed_inputs(3)[2]
    cs, _ = W.program_circuit(mixed.tape, pub, priv)
    packed = cs.pack()
    nnz = max(int(m[0][-1]) for m in packed.mats)
    srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, M.generate_rand(), env.ctx)
    pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
    srs.free()
    try:
        want = S.serialize_proof(M.generate_proof(cs, pk, M.generate_rand()))
        prove = lambda: M.generate_program_proof(pk, mixed, pub, priv, M.generate_rand())
        for where in ("caller's stream", "caller's stream again"):
            got, outputs = _gated_proof(env, prove)
            assert got == want and outputs == PM.mixed_eval(pub, priv)[0], where
        env.ctx.set_stream(None)
        got, outputs = _gated_proof(env, prove)
        assert got == want and outputs == PM.mixed_eval(pub, priv)[0], "own stream"
    finally:
        env.s.synchronize()
        env.ctx.set_stream(env.s.cuda_stream)
        pk.free()


# ------------------------------------------------------------------------------------------------ 2. the two uncalled entry points
def _operands(orc, n, seed):
    """n elements over 0, 1, r - 1 and random values, every pair of kinds meeting somewhere (strides 4 and 5)"""
    zero, one, minus_one = orc.fr_mont_from_ints([0, 1, R - 1])
    a, b = _fr(orc, n, seed), _fr(orc, n, seed + 1)
    for k, v in enumerate((zero, one, minus_one)):
        a[k::4] = v
        b[k::5] = v
    return a, b


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 256 * 32 * 256 + 3])
def test_vec_mul_fr_dev_against_the_oracle(env, orc, n):
    """swm_vec_mul_fr_dev, synchronised: around one workgroup, and one element past the capped grid (256 x 32 workgroups of 256
    lanes), where the grid-stride loop takes a second trip; out aliased to a, as the host form calls it."""
    torch, ctx = env.torch, env.ctx
    a, b = _operands(orc, n, 8800 + (n & 0xFF))
    want = _fr_mul(orc, a, b)
    d_a, d_b = env.resident(a) if n else env.dev(32), env.resident(b) if n else env.dev(32)
    d_out = torch.full((n * 32 + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.vec_mul_fr_dev(Ptr(d_a), Ptr(d_b), Ptr(d_out), n)
    ctx.synchronize()
    got = d_out.cpu().numpy()
    _same_rows(got[:n * 32], want, "vec_mul_fr_dev n = %d" % n)
    assert (got[n * 32:] == 0xFF).all()
    if n:
        assert np.array_equal(d_a.cpu().numpy(), _bytes(a)) and np.array_equal(d_b.cpu().numpy(), _bytes(b))
        ctx.vec_mul_fr_dev(Ptr(d_a), Ptr(d_b), Ptr(d_a), n)           # capi.hip: swm_vec_mul_fr runs vec_mul_run(da, db, da)
        ctx.synchronize()
        _same_rows(d_a.cpu().numpy(), want, "vec_mul_fr_dev n = %d, out = a" % n)
    assert ctx.lib.swm_vec_mul_fr_dev(ctx.h, None, None, None, 0) == 0
    assert ctx.lib.swm_vec_mul_fr_dev(ctx.h, None, d_b.data_ptr(), d_out.data_ptr(), 1) == -1


@pytest.mark.parametrize("count", [1, 64, 65, 257])
def test_pedersen_hash_dev_against_the_oracle(env, orc, crh, count):
    """swm_pedersen_hash_dev, synchronised, at the counts around the workgroup of the lanes-per-hash split (test_every_lane_split_vs_
    oracle's inputs: 64 bytes under the two-to-one parameters), and with 33-byte inputs under the leaf parameters: every second item
    starts off a word boundary.  Guard bytes after the digests stay."""
    torch, ctx = env.torch, env.ctx
    leaf, inner = crh
    rng = np.random.default_rng(count)
    for p, ln in ((inner, 64), (leaf, 33)):
        data = rng.integers(0, 256, size=(count, ln), dtype=np.uint8)
        data[0] = 0
        d_in = env.resident(data)
        d_out = torch.full((count * 32 + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.pedersen_hash_dev(p.h, Ptr(d_in), ln, count, Ptr(d_out))
        ctx.synchronize()
        got = d_out.cpu().numpy()
        _same_rows(got[:count * 32], OL.pedersen_hash(orc.lib, p.generators, data, threads=8), "pedersen_hash_dev %d x %d" % (count, ln))
        assert (got[count * 32:] == 0xFF).all() and not got[:32].any()
    assert ctx.lib.swm_pedersen_hash_dev(ctx.h, inner.h, None, 64, 0, None) == 0
    assert ctx.lib.swm_pedersen_hash_dev(ctx.h, inner.h, d_in.data_ptr(), 65, 1, d_out.data_ptr()) == -1     # 65 bytes do not fit 128 x 4 bits


# ------------------------------------------------------------------------------------------------ the table
def test_the_contract_names_every_dev_entry_point_and_each_has_its_case(env):
    """The table names the 24 _dev entry points the header declares; each has its case of (a) or is listed in NOT_COVERED with the
    reason.  Runs last: prints the warm-call times and gate lengths of the cases that ran (pytest -s)."""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swmarlin.h")).read()
    import re
    declared = set(re.findall(r"\bint (swm_\w+_dev)\(", header))
    assert declared == set(CONTRACT) and len(CONTRACT) == 24
    assert set(CASE_OF) | set(NOT_COVERED) == set(CONTRACT) and not set(CASE_OF) & set(NOT_COVERED)
    assert all(callable(globals().get(case)) for case in CASE_OF.values())
    print("\ncycles per ms %.0f" % env.cycles_per_ms)
    print(json.dumps(WARM_MS, indent=1))

"""swm_verify_proofs_batch / marlin.verify_proofs: batch verification of Marlin proofs on the GPU.

Honest batches at the sizes of both paths (host sums below 8 proofs, K1 MSMs from there on), tampered proofs whose per-proof
verdict must equal verify_proof's, malformed points and bytes whose status must equal swm_verify_proof's, the batch algebra
(TW, TC) against a Python-integer model built from oracle/pyref, and the generator's position afterwards."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWM_ERR_INVALID_ARG = -1
SWM_ERR_SERIALIZATION = -7
LOG_N = 10
N_INSTANCES = 12


@pytest.fixture(scope="module")
def M():
    from simpleworks_amd import marlin
    return marlin


@pytest.fixture(scope="module")
def env(M):
    """One key on the 2^10-row synthetic circuit; 300 proofs over N_INSTANCES instances (different public inputs), a few
    proofs in the uncompressed form, and a key + proofs of the manual-constraints circuit (one public input)."""
    from simpleworks_amd import workloads as W
    n = 1 << LOG_N
    rng = M.generate_rand()
    srs = M.generate_universal_srs(n, n, n, rng)
    cases = [W.synthetic_r1cs(n, 0x1000 + 7 * i, 0x2000 + 11 * i) for i in range(N_INSTANCES)]
    pk, vk = M.generate_proving_and_verifying_keys(srs, cases[0][0])
    proofs, publics = [], []
    for k in range(300):
        cs, pub = cases[k % N_INSTANCES]
        proofs.append(M.generate_proof(cs, pk, rng).data)
        publics.append(list(pub))
    unc = [M.generate_proof_uncompressed(cases[k][0], pk, rng) for k in range(10)]
    unc_pub = [list(cases[k][1]) for k in range(10)]
    msrs = M.generate_universal_srs(16, 16, 16, rng)
    mcs = [W.manual_constraints_circuit(a, a) for a in (3, 5, 8, 13, 21, 34, 55, 89, 144)]
    mpk, mvk = M.generate_proving_and_verifying_keys(msrs, mcs[0])
    mproofs = [M.generate_proof(cs, mpk, rng).data for cs in mcs]
    mpub = [[a] for a in (3, 5, 8, 13, 21, 34, 55, 89, 144)]
    yield dict(vk=vk, proofs=proofs, publics=publics, unc=unc, unc_pub=unc_pub, mvk=mvk, mproofs=mproofs, mpub=mpub)
    pk.free()
    mpk.free()
    srs.free()
    msrs.free()


def _batch(M, vk, publics, proofs, rng, flags=0, selftest=False):
    """(rc, ok, results[, tw, tc]) of one batch call; tw / tc as affine int pairs (None = identity)."""
    ctx = M.default_context()
    pi, n_inputs, ptrs, lens, _keep = M._batch_args(publics, proofs)
    ok = ctypes.c_int(-99)
    res = (ctypes.c_int * max(1, len(proofs)))()
    pi_p = pi.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if len(pi) else None
    if not selftest:
        rc = ctx.lib.swm_verify_proofs_batch(ctx.h, vk.h, pi_p, n_inputs, ptrs, lens, len(proofs), flags, rng.h,
                                             ctypes.byref(ok), res)
        return rc, ok.value, list(res[: len(proofs)])
    tw = np.zeros(12, dtype=np.uint64)
    tc = np.zeros(12, dtype=np.uint64)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    rc = ctx.lib.swm_selftest_verify_batch(ctx.h, vk.h, pi_p, n_inputs, ptrs, lens, len(proofs), flags, rng.h,
                                           ctypes.byref(ok), res, tw.ctypes.data_as(u64p), tc.ctypes.data_as(u64p))
    return rc, ok.value, list(res[: len(proofs)]), _g1_from_mont(tw), _g1_from_mont(tc)


def _g1_from_mont(xy):
    from pyref.bls12_377 import Q
    v = [int(x) for x in xy]
    x = sum(v[k] << (64 * k) for k in range(6)) * pow(1 << 384, -1, Q) % Q
    y = sum(v[6 + k] << (64 * k) for k in range(6)) * pow(1 << 384, -1, Q) % Q
    return None if x == 0 and y == 0 else (x, y)


def _single_rc(M, vk, pub, data):
    """swm_verify_proof's (return code, ok) for these bytes."""
    lib = M.load_library()
    pi = M._to_mont_limbs(pub)
    buf = (ctypes.c_uint8 * max(1, len(data))).from_buffer_copy(data.ljust(1, b"\0"))
    ok = ctypes.c_int(-99)
    rng = M.generate_rand()  # (held: the handle is freed with the object)
    rc = lib.swm_verify_proof(vk.h, pi.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if len(pi) else None, len(pi), buf,
                              len(data), rng.h, ctypes.byref(ok))
    return rc, ok.value


def _layout(data, point=48):
    """Byte offsets of a proof's parts: commitments (point offsets in byte order), evaluations, opening witnesses, random_v."""
    pos = 0
    u64 = lambda p: int.from_bytes(data[p:p + 8], "little")
    comms, evals, ws, rvs = [], [], [], []
    nr = u64(pos); pos += 8
    for _ in range(nr):
        nc = u64(pos); pos += 8
        for _ in range(nc):
            comms.append(pos); pos += point
            has = data[pos]; pos += 1
            if has:
                comms.append(pos); pos += point
    ne = u64(pos); pos += 8
    for _ in range(ne):
        evals.append(pos); pos += 32
    nm = u64(pos); pos += 8 + nm
    npf = u64(pos); pos += 8
    for _ in range(npf):
        ws.append(pos); pos += point
        has = data[pos]; pos += 1
        if has:
            rvs.append(pos); pos += 32
    return dict(comms=comms, evals=evals, ws=ws, rvs=rvs)


def _add_fr(data, off, delta=1):
    from pyref.bls12_377 import R
    v = (int.from_bytes(data[off:off + 32], "little") + delta) % R
    return data[:off] + v.to_bytes(32, "little") + data[off + 32:]


# ----------------------------------------------------------------------------------------------------------- honest batches
@pytest.mark.parametrize("count", [1, 2, 3, 64, 300])
def test_honest_batch(M, env, count):
    rc, ok, res = _batch(M, env["vk"], env["publics"][:count], env["proofs"][:count], M.generate_rand())
    assert (rc, ok, res) == (0, 1, [1] * count)
    if count == 1:  # the same decision as swm_verify_proof
        assert _single_rc(M, env["vk"], env["publics"][0], env["proofs"][0]) == (0, 1)


@pytest.mark.parametrize("count", [2, 16])
def test_repeated_proof_bytes(M, env, count):
    """The same proof bytes several times: the MSMs see repeated points (K1 at 16)."""
    half = count // 2
    proofs = env["proofs"][:half] * 2
    publics = env["publics"][:half] * 2
    assert _batch(M, env["vk"], publics, proofs, M.generate_rand()) == (0, 1, [1] * count)


@pytest.mark.parametrize("count", [3, 10])
def test_uncompressed_batch(M, env, count):
    rc, ok, res = _batch(M, env["vk"], env["unc_pub"][:count], env["unc"][:count], M.generate_rand(), flags=1)
    assert (rc, ok, res) == (0, 1, [1] * count)
    # the compressed bytes of the same proofs are malformed in the uncompressed form, and the other way round
    assert _batch(M, env["vk"], env["unc_pub"][:count], env["unc"][:count], M.generate_rand(), flags=0)[2] == \
        [SWM_ERR_SERIALIZATION] * count


@pytest.mark.parametrize("count", [1, 3, 9])
def test_manual_constraints_batch(M, env, count):
    rc, ok, res = _batch(M, env["mvk"], env["mpub"][:count], env["mproofs"][:count], M.generate_rand())
    assert (rc, ok, res) == (0, 1, [1] * count)
    bad = [list(p) for p in env["mpub"][:count]]
    bad[-1][0] += 1
    rc, ok, res = _batch(M, env["mvk"], bad, env["mproofs"][:count], M.generate_rand())
    assert (rc, ok, res) == (0, 0, [1] * (count - 1) + [0])


# ----------------------------------------------------------------------------------------------------------- rejection parity
def _tamper(kind, data, pub, other):
    lay = _layout(data)
    if kind == "evaluation":
        return _add_fr(data, lay["evals"][3]), pub
    if kind == "random_v":
        assert lay["rvs"], "the proofs carry random_v"
        return _add_fr(data, lay["rvs"][0]), pub
    if kind == "commitment":  # z_a (point 1) of a proof of another instance
        o = _layout(other)["comms"][1]
        c = lay["comms"][1]
        return data[:c] + other[o:o + 48] + data[c + 48:], pub
    if kind == "witnesses":
        a, b = lay["ws"]
        return data[:a] + data[b:b + 48] + data[a + 48:b] + data[a:a + 48] + data[b + 48:], pub
    if kind == "public_input":
        return data, [pub[0], pub[1] + 1]
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["evaluation", "random_v", "commitment", "witnesses", "public_input"])
@pytest.mark.parametrize("count", [5, 9])
def test_rejection_parity(M, env, kind, count):
    vk = env["vk"]
    for where in (0, count // 2, count - 1):
        proofs = list(env["proofs"][:count])
        publics = [list(p) for p in env["publics"][:count]]
        proofs[where], publics[where] = _tamper(kind, proofs[where], publics[where], env["proofs"][where + 1])
        rc, ok, res = _batch(M, vk, publics, proofs, M.generate_rand())
        single = M.verify_proof(vk, publics[where], M.MarlinProof(proofs[where]), M.generate_rand())
        assert not single
        assert (rc, ok) == (0, 0)
        assert res == [1] * where + [int(single)] + [1] * (count - where - 1)


# ----------------------------------------------------------------------------------------------------------- malformed points
@functools.lru_cache(maxsize=None)
def _bad_points():
    """(x >= q, an x with no square root, an on-curve point outside the prime-order subgroup)."""
    from pyref import bls12_377 as bls
    x = 2
    while bls.fq_sqrt((x ** 3 + 1) % bls.Q) is not None:
        x += 1
    no_root = x
    x = 5
    while True:
        y = bls.fq_sqrt((x ** 3 + 1) % bls.Q)
        if y is not None and bls.g1_mul_fast((x, y), bls.R) is not None:
            break
        x += 1
    return bls.Q, no_root, (x, y)


def _encode(kind, uncompressed):
    from pyref.bls12_377 import Q
    big_x, no_root, outside = _bad_points()
    if kind == "x_ge_q":
        x, y = big_x, 1
    elif kind == "no_root":
        x, y = no_root, 1
    else:
        x, y = outside
    if uncompressed:
        return x.to_bytes(48, "little") + (y % Q).to_bytes(48, "little")
    return x.to_bytes(48, "little")


@pytest.mark.parametrize("uncompressed", [False, True])
@pytest.mark.parametrize("kind", ["x_ge_q", "no_root", "outside_subgroup", "trailing_bytes"])
@pytest.mark.parametrize("count", [3, 9])
def test_malformed_points(M, env, kind, uncompressed, count):
    key = "unc" if uncompressed else "proofs"
    base_pub = env["unc_pub"] if uncompressed else env["publics"]
    proofs = list(env[key][:count])
    publics = [list(p) for p in base_pub[:count]]
    where = count // 2
    data = proofs[where]
    if kind == "trailing_bytes":
        data = data + b"\0"
    else:
        lay = _layout(data, 96 if uncompressed else 48)
        off = lay["comms"][4] if kind != "outside_subgroup" else lay["ws"][1]
        enc = _encode(kind, uncompressed)
        data = data[:off] + enc + data[off + len(enc):]
    proofs[where] = data
    rc, ok, res = _batch(M, env["vk"], publics, proofs, M.generate_rand(), flags=1 if uncompressed else 0)
    assert (rc, ok) == (0, 0)
    assert res == [1] * where + [SWM_ERR_SERIALIZATION] + [1] * (count - where - 1)
    if uncompressed:  # the host's checked reader of that form (swm_proof_recode parses it before converting)
        n = ctypes.c_size_t(0)
        buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
        assert M.load_library().swm_proof_recode(buf, len(data), 0, None, 0, ctypes.byref(n)) == SWM_ERR_SERIALIZATION
    else:
        assert _single_rc(M, env["vk"], publics[where], data)[0] == SWM_ERR_SERIALIZATION


# ----------------------------------------------------------------------------------------------------------- algebra parity
def _parse_vk(data):
    """The verifying-key fields the model needs (G2 points skipped), in oracle/pyref's dict form."""
    from pyref import marlin as P
    pos = [0]

    def take(n):
        b = data[pos[0]:pos[0] + n]
        pos[0] += n
        return b
    u64 = lambda: int.from_bytes(take(8), "little")
    vk = {"num_variables": u64(), "num_constraints": u64(), "num_non_zero": u64(), "num_instance_variables": u64()}
    comms = []
    for _ in range(u64()):
        c = P.deser_g1(take(48))
        s = P.deser_g1(take(48)) if take(1)[0] else None
        comms.append((c, s))
    vk["index_comms"] = comms
    g, gamma_g = P.deser_g1(take(48)), P.deser_g1(take(48))
    take(192)
    assert take(1)[0] == 1
    dbs = [(u64(), P.deser_g1(take(48))) for _ in range(u64())]
    vk["verifier_key"] = {"g": g, "gamma_g": gamma_g, "degree_bounds_and_shift_powers": dbs}
    return vk


def _model_pairing_inputs(vk, public_input, proof, rands):
    """One proof's (total_w, total_c) of KZG10::batch_check with randomizers `rands` for (beta, gamma): pyref's verify()
    with its first randomizer replaced, in Python integers."""
    from pyref import bls12_377 as bls
    from pyref import marlin as P
    from pyref.bls12_377 import R
    from pyref.poly import Domain
    dx = Domain(len(public_input) + 1)
    public_input = list(public_input) + [0] * (max(len(public_input), dx.size - 1) - len(public_input))
    fs = P._fs_init(vk, public_input)
    comms1, comms2, comms3 = proof["commitments"]
    dh, dk = Domain(vk["num_constraints"]), Domain(vk["num_non_zero"])
    fs.absorb(b"".join(P.tb_commitment(c) for c in comms1))
    alpha = P._sample_outside(dh, fs)
    eta_a, eta_b, eta_c = fs.rand_fr(), fs.rand_fr(), fs.rand_fr()
    fs.absorb(b"".join(P.tb_commitment(c) for c in comms2))
    beta = P._sample_outside(dh, fs)
    fs.absorb(b"".join(P.tb_commitment(c) for c in comms3))
    gamma = fs.rand_fr()
    st = {"alpha": alpha, "eta_a": eta_a, "eta_b": eta_b, "eta_c": eta_c, "beta": beta, "gamma": gamma}
    bounds = [None] * 12 + [None, None, None, None, None, dh.size - 2, None, dk.size - 2, None]
    labels = P.INDEXER_POLYNOMIALS + P.PROVER_POLYNOMIALS
    commitments = {l: (c, d) for l, c, d in zip(labels, list(vk["index_comms"]) + comms1 + comms2 + comms3, bounds)}
    fs.absorb(b"".join(P.tb_fr(e) for e in proof["evaluations"]))
    xi = fs.gen_u128() % R
    pl_of = dict(P.QUERY_SET)
    evaluations = {l: 0 for l in P.LC_WITH_ZERO_EVAL}
    for l, e in zip(sorted(l for l, _ in P.QUERY_SET if l not in P.LC_WITH_ZERO_EVAL), proof["evaluations"]):
        evaluations[l] = e
    lcs = P.construct_linear_combinations(vk, public_input, lambda label, lc, pt: evaluations[label], st)
    lc_comms = {}
    for label, lc in lcs:
        comm, shifted, bound = None, None, None
        for coeff, term in lc:
            if term is None:
                evaluations[label] = (evaluations[label] - coeff) % R
                continue
            (c, s), d = commitments[term]
            if d is not None:
                bound = d
            comm = bls.g1_add(comm, bls.g1_mul_fast(c, coeff))
            if s is not None:
                shifted = bls.g1_add(shifted, bls.g1_mul_fast(s, coeff))
        lc_comms[label] = (comm, shifted, bound)
    pv = vk["verifier_key"]
    shift_power = dict(pv["degree_bounds_and_shift_powers"])
    total_c, total_w = None, None
    for i, (pl, z) in enumerate((("beta", beta), ("gamma", gamma))):
        cc, cv, ch = None, 0, 1
        for l in sorted(l for l, p in P.QUERY_SET if p == pl):
            c, s, d = lc_comms[l]
            v = evaluations[l]
            cc = bls.g1_add(cc, bls.g1_mul_fast(c, ch))
            cv = (cv + v * ch) % R
            ch = ch * xi % R
            if d is not None:
                adj = bls.g1_add(s, bls.g1_neg(bls.g1_mul_fast(shift_power[d], v)))
                cc = bls.g1_add(cc, bls.g1_mul_fast(adj, ch))
                ch = ch * xi % R
        w, rv = proof["pc_proof"][i]
        r = rands[i]
        part = bls.g1_add(bls.g1_add(bls.g1_mul_fast(w, z), cc), bls.g1_neg(bls.g1_mul_fast(pv["g"], cv)))
        if rv is not None:
            part = bls.g1_add(part, bls.g1_neg(bls.g1_mul_fast(pv["gamma_g"], rv)))
        total_c = bls.g1_add(total_c, bls.g1_mul_fast(part, r))
        total_w = bls.g1_add(total_w, bls.g1_mul_fast(w, r))
    return total_w, total_c


@pytest.mark.parametrize("count", [3, 8])
def test_batch_algebra_matches_python_model(M, env, count):
    from pyref import bls12_377 as bls
    from pyref import marlin as P
    from simpleworks_amd import serialization as S
    vk = _parse_vk(S.serialize_verifying_key(env["vk"]))
    seed = bytes(range(7, 39))
    rng, twin = M.rng_from_seed(seed), M.rng_from_seed(seed)
    proofs = env["proofs"][:count]
    publics = env["publics"][:count]
    rc, ok, res, tw, tc = _batch(M, env["vk"], publics, proofs, rng, selftest=True)
    assert (rc, ok, res) == (0, 1, [1] * count)
    want_w, want_c = None, None
    for p in range(count):
        rands = []
        for _ in range(2):
            lo, hi = twin.next_u64(), twin.next_u64()
            rands.append((hi << 64) | lo)
        w, c = _model_pairing_inputs(vk, publics[p], P.deserialize_proof(proofs[p]), rands)
        want_w, want_c = bls.g1_add(want_w, w), bls.g1_add(want_c, c)
    assert tw == want_w
    assert tc == want_c


# ----------------------------------------------------------------------------------------------------------- generator, edges
def test_generator_position(M, env):
    key = bytes(range(32))
    rng, twin = M.rng_from_chacha(key, 40, 12), M.rng_from_chacha(key, 40, 12)
    rc, ok, res = _batch(M, env["vk"], env["publics"][:37], env["proofs"][:37], rng)
    assert (rc, ok) == (0, 1)
    for _ in range(74):
        twin.next_u64()
        twin.next_u64()
    assert rng.word_pos() == twin.word_pos() == 40 + 74 * 4


def test_empty_batch_and_bad_arguments(M, env):
    ctx = M.default_context()
    lib = ctx.lib
    rng = M.rng_from_chacha(bytes(32), 8, 12)
    ok = ctypes.c_int(-99)
    assert lib.swm_verify_proofs_batch(ctx.h, env["vk"].h, None, 2, None, None, 0, 0, rng.h, ctypes.byref(ok), None) == 0
    assert ok.value == 1
    assert rng.word_pos() == 8
    assert M.verify_proofs(env["vk"], [], [], rng) is True
    assert rng.word_pos() == 8
    pi, n_inputs, ptrs, lens, _keep = M._batch_args(env["publics"][:2], env["proofs"][:2])
    pi_p = pi.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    good = (ctx.h, env["vk"].h, pi_p, n_inputs, ptrs, lens, 2, 0, rng.h, ctypes.byref(ok), None)
    for k in (0, 1, 2, 4, 5, 8, 9):  # ctx, vk, public inputs, proofs, lens, rng, ok
        args = list(good)
        args[k] = None
        assert lib.swm_verify_proofs_batch(*args) == SWM_ERR_INVALID_ARG, k
    args = list(good)
    args[7] = 2  # unknown flag
    assert lib.swm_verify_proofs_batch(*args) == SWM_ERR_INVALID_ARG
    one_null = (ctypes.c_void_p * 2)(ptrs[0], None)
    args = list(good)
    args[4] = one_null
    assert lib.swm_verify_proofs_batch(*args) == SWM_ERR_INVALID_ARG
    assert rng.word_pos() == 8  # refused calls draw nothing
    assert lib.swm_verify_proofs_batch(*good) == 0 and ok.value == 1


def test_python_wrapper(M, env):
    vk = env["vk"]
    publics = [list(p) for p in env["publics"][:12]]
    proofs = [M.MarlinProof(d) for d in env["proofs"][:12]]
    assert M.verify_proofs(vk, publics, proofs, M.generate_rand()) is True
    assert M.verify_proofs(vk, publics, proofs, M.generate_rand(), per_proof=True) == (True, [1] * 12)
    publics[4][1] += 1
    proofs[7] = M.MarlinProof(proofs[7].data + b"\0")
    got = M.verify_proofs(vk, publics, proofs, M.generate_rand(), per_proof=True)
    rc, ok, res = _batch(M, vk, publics, [p.data for p in proofs], M.generate_rand())
    assert got == (False, res) and rc == 0 and ok == 0
    assert res == [1] * 4 + [0] + [1] * 2 + [SWM_ERR_SERIALIZATION] + [1] * 4
    assert M.verify_proofs(vk, publics, proofs, M.generate_rand()) is False

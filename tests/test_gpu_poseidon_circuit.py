"""The Poseidon hash circuit's witness synthesised on the GPU (csrc/poseidon_witness.hip: swm_poseidon_witness,
swm_poseidon_witness_dev, swm_poseidon_prove) against its specification, workloads.build_poseidon_hash run on the CPU: exact equality
of the whole witness vector in Montgomery limbs and of the public outputs, the device form's per-item refusals, and
generate_poseidon_proof against generate_proof on the builder's system, byte for byte.
The builder costs milliseconds per item at these sizes, so whole-witness equality is affordable everywhere."""
import os

import numpy as np
import pytest

import poseidon_model as P
from oracle_lib import golden

pytestmark = pytest.mark.gpu

R = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001
PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_params.json")


class _WitnessOnly:
    """The builder's vocabulary, keeping the assignment and dropping the rows."""

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


def le(h):
    return int.from_bytes(bytes.fromhex(h), "little")


def ints(a):
    return [int.from_bytes(r.tobytes(), "little") for r in np.asarray(a).reshape(-1, 32)]


def rows(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(len(values), 32).copy()


@pytest.fixture(scope="module")
def M():
    from simpleworks_amd import marlin
    return marlin


@pytest.fixture(scope="module")
def W():
    from simpleworks_amd import workloads
    return workloads


@pytest.fixture(scope="module")
def HASH():
    from simpleworks_amd import hash
    return hash


@pytest.fixture(scope="module")
def G():
    return golden("poseidon.json")


@pytest.fixture(scope="module")
def ref_params(HASH):
    return HASH.PoseidonParameters.from_json(PARAMS)


@pytest.fixture(scope="module")
def sponge(HASH, ref_params):
    s = HASH.PoseidonSponge(ref_params)
    yield s
    s.free()


@pytest.fixture(scope="module")
def circuits(HASH, sponge):
    made = {}

    def get(input_len=None, n_in=None, n_out=1):
        k = (input_len, n_in, n_out)
        if k not in made:
            made[k] = HASH.PoseidonCircuit(sponge, input_len=input_len, n_in=n_in, n_out=n_out)
        return made[k]
    yield get
    for c in made.values():
        c.free()


def _build(M, W, params, data=None, elements=None, n_out=1):
    """-> (the builder's witness as Montgomery limbs, its public outputs as ints)"""
    cs = _WitnessOnly()
    public = W.build_poseidon_hash(cs, params, data=data, elements=elements, n_out=n_out)
    assert public == cs.public
    return M._to_mont_limbs(cs.witness), public


@pytest.fixture(scope="module")
def oracle(M, W, ref_params):
    """bytes -> (witness limbs, [digest]) under the reference's parameters; built once per input."""
    seen = {}

    def get(data):
        data = bytes(data)
        if data not in seen:
            seen[data] = _build(M, W, ref_params, data=data)
        return seen[data]
    return get


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: %d witnesses differ, the first at %d" % (what, bad.size, bad[0])


def _check_bytes(oracle, circuit, msgs, items=None):
    """The whole witness of every item (or of `items`) and every digest equal the builder's."""
    witness, outputs = circuit.witness_many(msgs)
    assert witness.shape == (len(msgs), circuit.shape()[1], 4) and outputs.shape == (len(msgs), 1, 32)
    for i in (range(len(msgs)) if items is None else items):
        want, public = oracle(msgs[i])
        _same(witness[i], want, "item %d" % i)
        assert ints(outputs[i]) == public, i
    return witness, outputs


@pytest.mark.parametrize("length", [0, 11, 23, 24, 54, 55, 86])
def test_bytes_form_at_the_chunk_and_rate_boundaries(G, oracle, circuits, length):
    """8 + n = 31 | 32, 62 | 63 (two elements: the rate), 94: one to four elements, one and two permutations."""
    msgs = [P.poseidon_input(length, i) for i in range(3)]
    _, outputs = _check_bytes(oracle, circuits(input_len=length), msgs)
    have = [le(h) for h in G["bytes"][str(length)]]
    assert ints(outputs) == [have[min(i, len(have) - 1)] for i in range(3)]


def test_one_long_input(oracle, circuits):
    """1000 bytes: 33 elements, 17 permutations, 8000 bit witnesses written by the wave's second pass."""
    c = circuits(input_len=1000)
    assert c.shape() == (2, 8000 + 17 * 265, 8000 + 17 * 265 + 1)
    _check_bytes(oracle, c, [P.poseidon_input(1000, 0)])


@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
def test_batch_counts_at_the_lane_and_workgroup_edges(oracle, circuits, count):
    _check_bytes(oracle, circuits(input_len=11), [P.poseidon_input(11, i) for i in range(count)])


@pytest.mark.parametrize("count,chunk", [(7, 3), (3, 1)])
def test_bytes_form_across_a_chunk_seam(oracle, circuits, count, chunk):
    """The host form with its stage cap moved (swm_selftest_witness_stage): 7 items at a cap of 3 items' witness bytes + 5 go in
    chunks of 3, 3 and 1, 3 items at a cap one byte short of an item one by one.  11 bytes: the shortest input of this module at
    which items differ."""
    c = circuits(input_len=11)
    item = 32 * c.shape()[1]
    with c.ctx.selftest_witness_stage(3 * item + 5 if chunk == 3 else item - 1):
        _check_bytes(oracle, c, [P.poseidon_input(11, i) for i in range(count)])


def test_a_thousand_items_against_the_native_hash(oracle, sponge, circuits):
    msgs = [P.poseidon_input(55, i) for i in range(1000)]
    _, outputs = _check_bytes(oracle, circuits(input_len=55), msgs, items=(0, 63, 64, 999))
    a = np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(1000, 55)
    assert np.array_equal(outputs.reshape(1000, 32), sponge.hash_many(a))


@pytest.mark.parametrize("n_out", [1, 2, 3])
def test_elements_form_equals_the_builder_and_the_fixture(M, W, G, ref_params, circuits, n_out):
    for n_in in range(6):
        cases = [c for c in G["elements"] if len(c["in"]) == n_in]
        assert cases
        items = [[le(h) for h in c["in"]] for c in cases]
        c = circuits(n_in=n_in, n_out=n_out)
        witness, outputs = c.witness_many(rows([v for it in items for v in it]).reshape(len(items), n_in, 32))
        assert witness.shape == (len(items), c.shape()[1], 4)
        for i, item in enumerate(items):
            want, public = _build(M, W, ref_params, elements=item, n_out=n_out)
            _same(witness[i], want, "n_in %d item %d" % (n_in, i))
            assert ints(outputs[i]) == public == [le(h) for h in cases[i]["out"][:n_out]]


def test_adversarial_parameter_sets(M, W, HASH, G):
    """Every parameter set of the fixture's adversarial list (fill r - 1 / identity / reference, alpha 2 .. 65535 — m(alpha) from 1 to
    30 values per S-box — with and without partial rounds, two and eight full rounds) over items of r - 1 and random values, three
    outputs each: the lazy arithmetic's bounds with recording."""
    ref = P.load_params(PARAMS)
    items = [[le(h) for h in item] for item in G["adversarial_items"]]
    seen = set()
    for case in G["adversarial"]:
        full, partial, alpha = case["full_rounds"], case["partial_rounds"], case["alpha"]
        params = HASH.PoseidonParameters(*P.adversarial_params(case["fill"], full, partial, alpha, ref))
        seen.add((case["fill"], full, partial, alpha))
        s = HASH.PoseidonSponge(params)
        try:
            for item, out in zip(items, case["out"]):
                c = HASH.PoseidonCircuit(s, n_in=len(item), n_out=3)
                try:
                    witness, outputs = c.witness_many([item])
                finally:
                    c.free()
                want, public = _build(M, W, params, elements=item, n_out=3)
                _same(witness[0], want, str((case["fill"], full, partial, alpha, len(item))))
                assert ints(outputs[0]) == public == [le(h) for h in out]
        finally:
            s.free()
    for fill in ("r-1", "identity"):
        for alpha in (2, 3, 5, 17, 65535):
            assert {(fill, 8, 0, alpha), (fill, 2, 29, alpha), (fill, 2, 0, alpha), (fill, 8, 29, alpha)} <= seen


def test_device_form_reports_a_non_canonical_element_per_item(M, W, ref_params, circuits):
    from simpleworks_amd._lib import SwmError
    count, n_in, n_out = 130, 3, 2
    c = circuits(n_in=n_in, n_out=n_out)
    ctx, nw = c.ctx, c.shape()[1]
    items = [[P.fr("circuit status %d %d" % (i, k)) for k in range(n_in)] for i in range(count)]
    bad = {0: (0, R), 64: (2, (1 << 256) - 1), 129: (1, R + 1)}
    sent = [list(it) for it in items]
    for i, (pos, v) in bad.items():
        sent[i][pos] = v
    elems = rows([v for it in sent for v in it])
    d_in, d_w, d_out, d_st = ctx.alloc(elems.nbytes).upload(elems), ctx.alloc(count * nw * 32), ctx.alloc(count * n_out * 32), ctx.alloc(4 * count)
    d_w.upload(np.full(count * nw * 32, 0x5A, dtype=np.uint8))
    d_out.upload(np.full(count * n_out * 32, 0x5A, dtype=np.uint8))
    d_st.upload(np.full(count, 7, dtype=np.uint32))
    ctx.poseidon_witness_dev(c.h, d_in, count, d_w, d_out, d_st)
    ctx.synchronize()
    witness = d_w.download((count, nw, 4))
    outputs = d_out.download((count, n_out, 32), np.uint8)
    status = d_st.download((count,), np.uint32)
    assert [int(s) for s in status] == [1 if i in bad else 0 for i in range(count)]
    for i in range(count):
        if i in bad:
            assert not witness[i].any() and not outputs[i].any(), i
        else:
            want, public = _build(M, W, ref_params, elements=items[i], n_out=n_out)
            _same(witness[i], want, "item %d" % i)
            assert ints(outputs[i]) == public, i
    # without outputs and status: the same witnesses
    d_w.upload(np.full(count * nw * 32, 0x5A, dtype=np.uint8))
    ctx.poseidon_witness_dev(c.h, d_in, count, d_w, None, None)
    ctx.synchronize()
    assert np.array_equal(d_w.download((count, nw, 4)), witness)
    # the host form refuses the whole call and writes nothing
    out = np.full((count, n_out, 32), 0x5A, dtype=np.uint8)
    with pytest.raises(SwmError) as e:
        ctx.poseidon_witness(c.h, nw, n_out, elems.reshape(count, n_in, 32), out)
    assert e.value.code == -1 and "item 0" in str(e.value)
    assert (out == 0x5A).all(), "a refused call wrote to the output"
    # count = 0: SWM_OK, nothing launched, buffers may be NULL
    lib = ctx.lib
    assert lib.swm_poseidon_witness(ctx.h, c.h, None, 0, None, None) == 0
    assert lib.swm_poseidon_witness_dev(ctx.h, c.h, None, 0, None, None, None) == 0
    w0, o0 = c.witness_many(np.zeros((0, n_in, 32), dtype=np.uint8))
    assert w0.shape == (0, nw, 4) and o0.shape == (0, n_out, 32)
    for b in (d_in, d_w, d_out, d_st):
        b.free()


def test_create_refusals(HASH, sponge):
    from simpleworks_amd._lib import SwmError
    for kw in ({"input_len": 65537}, {"n_in": 4097}, {"n_in": 1, "n_out": 0}, {"n_in": 1, "n_out": 17}, {"input_len": 11, "n_out": 2}):
        with pytest.raises(SwmError) as e:
            HASH.PoseidonCircuit(sponge, **kw)
        assert e.value.code == -1, kw
    c = HASH.PoseidonCircuit(sponge, input_len=65536)
    assert c.shape() == (2, 804658, 804659)
    c.free()
    c.free()
    assert c.h is None


@pytest.mark.parametrize("length", [11, 55])
def test_proof_equals_the_builders(M, W, HASH, ref_params, circuits, length):
    """generate_poseidon_proof is byte-identical to generate_proof on the builder's system with the same rng state and verifies with
    the digest as the public input — and not with digest + 1; a circuit of another length does not match the key (-8)."""
    from simpleworks_amd import serialization as Ser
    data = P.poseidon_input(length, 0)
    assert length != 11 or data == b"Hello World"
    cs = M.MarlinInst._synthesize(W.PoseidonHashCircuit(ref_params, data=data))
    digest = cs.instance[1]
    assert digest == P.hash_bytes(P.load_params(PARAMS), data)
    packed = cs.pack()
    nnz = max(int(m[0][-1]) for m in packed.mats)
    srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, M.generate_rand())
    pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
    srs.free()
    try:
        want = M.generate_proof(cs, pk, M.generate_rand())
        got, outputs = M.generate_poseidon_proof(pk, circuits(input_len=length), data, M.generate_rand())
        assert outputs == [digest]
        assert got == Ser.serialize_proof(want)
        assert M.verify_proof(vk, [digest], M.MarlinProof(got), M.generate_rand())
        assert not M.verify_proof(vk, [(digest + 1) % R], M.MarlinProof(got), M.generate_rand())
        with pytest.raises(M.MarlinError) as e:
            M.generate_poseidon_proof(pk, circuits(input_len=length + 1), data + b"!", M.generate_rand())
        assert e.value.code == -8
        # the prover is as it was for the next caller: the device source does not outlive the call
        assert Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand())) == got
    finally:
        pk.free()

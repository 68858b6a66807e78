"""Integer programs on the GPU (csrc/program_witness.hip: swm_program_witness, swm_program_witness_dev, swm_program_prove,
swm_program_prove_many) against the circuit's specification, workloads.build_program, and the plain-integer semantics recorded in
tests/golden/program.json: the whole witness vector in Montgomery limbs, bit for bit, for every unit program and for the mixed
program at the wave and workgroup edges of a lane-per-item kernel; refused items; the device form; and the proofs, byte for byte
against the prover on the builder's system."""
import ctypes
import json
import os

import numpy as np
import pytest

import program_model as PM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "program.json")) as f:
    GOLDEN = json.load(f)
UNITS = PM.unit_programs()


@pytest.fixture(scope="module")
def M():
    from simpleworks_amd import marlin
    return marlin


@pytest.fixture(scope="module")
def W():
    from simpleworks_amd import workloads
    return workloads


@pytest.fixture(scope="module")
def PG():
    from simpleworks_amd import program
    return program


@pytest.fixture(scope="module")
def ctx(M):
    return M.default_context()


@pytest.fixture(scope="module")
def mixed(PG, ctx):
    c = PG.ProgramCircuit(PM.mixed_program(), ctx)
    yield c
    c.free()


@pytest.fixture(scope="module")
def model(M, W):
    """(tape, public, private) -> the builder's witness as Montgomery limbs; built once per execution."""
    seen = {}

    def get(tape, public, private):
        key = (tape, tuple(public), tuple(private))
        if key not in seen:
            cs = M.ConstraintSystem()
            W.build_program(cs, tape, public, private)
            seen[key] = M._to_mont_limbs(cs.witness)
        return seen[key]
    return get


def _run(PG, circuit, public, private):
    """swm_program_witness over buffers filled with 0xFF beforehand: (witness, outputs as values, status)."""
    rows = PG.pack_inputs(circuit.tape, public, private)
    count = rows.shape[0]
    witness = np.full((count, circuit.shape()[1], 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    outputs = np.full((count, circuit.layout["output_bytes"]), 0xFF, dtype=np.uint8)
    status = np.full(count, 0xFF, dtype=np.uint8)
    rc = circuit.ctx.lib.swm_program_witness(circuit.ctx.h, circuit.h, rows.ctypes.data if rows.size else None, count,
                                             witness.ctypes.data if witness.size else None, outputs.ctypes.data if outputs.size else None,
                                             status.ctypes.data)
    assert rc == 0, circuit.ctx.lib.swm_last_error(circuit.ctx.h)
    return witness, PG.unpack_outputs(circuit.tape, outputs), status


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=-1)).ravel()
        raise AssertionError("%s: %d of %d witnesses differ, the first at %d: got %s, want %s"
                             % (what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]]))


# ------------------------------------------------------------------------------------------------------------ witness parity
@pytest.mark.parametrize("name", sorted(UNITS))
def test_unit_program_witness_equals_the_builders(PG, ctx, model, name):
    """Every op at every width over the extremal operand pairs, one batch per program: the witnesses are the builder's, the outputs
    and status bytes the fixture's."""
    P, op, t, positions = UNITS[name]
    gold = GOLDEN["unit"][name]
    pairs = PM.extremal(PM.width(t))
    cases = PM.unit_cases(op, t, positions, pairs)
    assert PM.hexes(v for _, v, _ in cases) == " ".join(gold["outputs"].split()[:len(pairs)])
    assert "".join(str(s) for _, _, s in cases) == gold["status"][:len(pairs)]
    c = PG.ProgramCircuit(P, ctx)
    try:
        assert c.shape() == tuple(gold["counts"]) and c.tape.hex() == gold["tape"]
        witness, outputs, status = _run(PG, c, [[]] * len(cases), [p for p, _, _ in cases])
        assert outputs == [[v] for _, v, _ in cases]
        assert status.tolist() == [s for _, _, s in cases]
        for i, (private, _, _) in enumerate(cases):
            _same(witness[i], model(c.tape, [], private), "%s item %d %s" % (name, i, private))
    finally:
        c.free()


@pytest.mark.parametrize("count", (1, 63, 64, 65, 256, 257))
def test_mixed_program_batches(PG, mixed, model, count):
    """The wave and workgroup edges of a lane-per-item kernel; 1681 witnesses per item are no multiple of the expand kernel's 128."""
    gold = GOLDEN["mixed"]
    assert mixed.shape() == tuple(gold["counts"]) and mixed.shape()[1] % 128 != 0
    rows = PM.mixed_inputs(count)
    witness, outputs, status = _run(PG, mixed, [p for p, _ in rows], [s for _, s in rows])
    assert [PM.hexes(o) for o in outputs] == gold["outputs"][:count]
    assert "".join(str(s) for s in status) == gold["status"][:count] == "0" * count
    for i, (pub, priv) in enumerate(rows):
        _same(witness[i], model(mixed.tape, pub, priv), "item %d of %d" % (i, count))
    # the wrapper the callers use gives the same
    w2, o2, s2 = mixed.witness_many([p for p, _ in rows], [s for _, s in rows])
    assert np.array_equal(w2, witness) and o2 == outputs and np.array_equal(s2, status)


@pytest.mark.parametrize("count,chunk", [(7, 3), (3, 1)])
def test_mixed_program_across_a_chunk_seam(PG, mixed, model, count, chunk):
    """The host form with its stage cap moved (swm_selftest_witness_stage): 7 items at a cap of 3 items' witness bytes + 5 go in
    chunks of 3, 3 and 1, 3 items at a cap one byte short of an item one by one.  Item 1 underflows: its status lands on its own
    index whichever chunk holds it; witnesses, outputs and status are the one-chunk run's."""
    gold = GOLDEN["mixed"]
    item = 32 * mixed.shape()[1]
    rows = PM.mixed_inputs(count, underflow=(1,))
    with mixed.ctx.selftest_witness_stage(3 * item + 5 if chunk == 3 else item - 1):
        witness, outputs, status = _run(PG, mixed, [p for p, _ in rows], [s for _, s in rows])
    assert status.tolist() == [PM.UNDERFLOW if i == 1 else 0 for i in range(count)]
    assert [PM.hexes(o) for i, o in enumerate(outputs) if i != 1] == [gold["outputs"][i] for i in range(count) if i != 1]
    assert outputs == [PM.mixed_eval(pub, priv)[0] for pub, priv in rows]
    for i, (pub, priv) in enumerate(rows):
        _same(witness[i], model(mixed.tape, pub, priv), "item %d of %d" % (i, count))


def test_refused_items_set_their_status_alone(PG, mixed, model):
    """A batch of 65 in which item 31 underflows and item 64 divides by zero: only their status bytes are set, every other item is
    what it is in the batch without them, and their own witnesses are the builder's — the documented wrapped values."""
    gold = GOLDEN["mixed"]["refusals"]
    good = PM.mixed_inputs(65)
    bad = PM.mixed_inputs(65, underflow=(31,), div_zero=(64,))
    assert [i for i in range(65) if good[i] != bad[i]] == [31, 64]
    w_good, _, s_good = _run(PG, mixed, [p for p, _ in good], [s for _, s in good])
    w_bad, outputs, status = _run(PG, mixed, [p for p, _ in bad], [s for _, s in bad])
    assert not s_good.any()
    assert "".join(str(s) for s in status) == gold["status"] and [i for i in range(65) if status[i]] == [31, 64]
    assert (status[31], status[64]) == (PM.UNDERFLOW, PM.DIV_ZERO | PM.ASSERT)
    assert [PM.hexes(o) for o in outputs] == [gold["outputs"].get(str(i), GOLDEN["mixed"]["outputs"][i]) for i in range(65)]
    for i in range(65):
        if i in (31, 64):
            _same(w_bad[i], model(mixed.tape, *bad[i]), "refused item %d" % i)
        else:
            assert np.array_equal(w_bad[i], w_good[i]), i


def test_device_form_guard_empty_batch_and_alignment(PG, mixed, ctx, model):
    import torch
    count, guard = 65, 4096
    rows = PM.mixed_inputs(count, seed=5)
    a = PG.pack_inputs(mixed.tape, [p for p, _ in rows], [s for _, s in rows])
    nw, ob = mixed.shape()[1], mixed.layout["output_bytes"]
    d_in = torch.from_numpy(a).cuda()
    d_w = torch.full((count * nw * 32 + guard,), 0xFF, dtype=torch.uint8, device="cuda")
    d_out = torch.full((count * ob + guard,), 0xFF, dtype=torch.uint8, device="cuda")
    d_st = torch.full((count + guard,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    mixed.witness_dev(d_in.data_ptr(), count, d_w.data_ptr(), d_out.data_ptr(), d_st.data_ptr())
    ctx.synchronize()
    w = d_w.cpu().numpy()
    assert (w[count * nw * 32:] == 0xFF).all() and (d_out.cpu().numpy()[count * ob:] == 0xFF).all()
    st = d_st.cpu().numpy()
    assert not st[:count].any() and (st[count:] == 0xFF).all()
    witness = w[:count * nw * 32].view(np.uint64).reshape(count, nw, 4)
    for i, (pub, priv) in enumerate(rows):
        _same(witness[i], model(mixed.tape, pub, priv), "item %d" % i)
    outputs = PG.unpack_outputs(mixed.tape, d_out.cpu().numpy()[:count * ob].reshape(count, ob))
    assert outputs == [PM.mixed_eval(pub, priv)[0] for pub, priv in rows]
    # without a status buffer: the same witnesses
    d_w.fill_(0xFF)
    torch.cuda.synchronize()
    mixed.witness_dev(d_in.data_ptr(), count, d_w.data_ptr(), d_out.data_ptr(), None)
    ctx.synchronize()
    assert np.array_equal(d_w.cpu().numpy(), w)
    # an empty batch is a no-op, buffers may be NULL
    lib = ctx.lib
    assert lib.swm_program_witness_dev(ctx.h, mixed.h, None, 0, None, None, None) == 0
    assert lib.swm_program_witness(ctx.h, mixed.h, None, 0, None, None, None) == 0
    w0, o0, s0 = mixed.witness_many([], [])
    assert w0.shape == (0, nw, 4) and o0 == [] and s0.shape == (0,)
    ctx.synchronize()
    assert np.array_equal(d_w.cpu().numpy(), w)
    # a misaligned witness pointer is refused, and nothing is written
    assert lib.swm_program_witness_dev(ctx.h, mixed.h, d_in.data_ptr(), count, d_w.data_ptr() + 8, d_out.data_ptr(), d_st.data_ptr()) == -1
    assert lib.swm_program_witness_dev(ctx.h, mixed.h, d_in.data_ptr(), count, None, d_out.data_ptr(), d_st.data_ptr()) == -1
    ctx.synchronize()
    assert np.array_equal(d_w.cpu().numpy(), w)


def test_create_refuses_what_the_validator_refuses(PG, W, ctx):
    h = ctypes.c_void_p()
    tape = PM.test_circuit_program().tape()
    for bad in (tape[:-1], b"SWMPROG2" + tape[8:], W.program_header(3) + W.program_word("INPUT_PRIVATE", 5) * 2 + W.program_word("MUL", 5, 0, 1)):
        buf = (ctypes.c_uint8 * len(bad)).from_buffer_copy(bad)
        assert ctx.lib.swm_program_create(ctx.h, buf, len(bad), ctypes.byref(h)) == -1 and not h.value
    with pytest.raises(Exception):
        PG.ProgramCircuit(tape[:-1], ctx)


# ---------------------------------------------------------------------------------------------------------------- proofs
def _index(M, cs):
    packed = cs.pack()
    nnz = max(int(m[0][-1]) for m in packed.mats)
    srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, M.generate_rand())
    pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
    srs.free()
    return pk, vk


@pytest.fixture(scope="module")
def mixed_keys(M, W, mixed):
    pub, priv = PM.mixed_inputs(1)[0]
    cs, _ = W.program_circuit(mixed.tape, pub, priv)
    assert max(cs.num_constraints, len(cs.instance) + len(cs.witness)) <= 1 << 13
    pk, vk = _index(M, cs)
    yield pk, vk
    pk.free()


@pytest.fixture(scope="module")
def tc(M, W, PG, ctx):
    c = PG.ProgramCircuit(PM.test_circuit_program(), ctx)
    pk, vk = _index(M, W.test_circuit(0xA7, 0xA7))
    yield c, pk, vk
    pk.free()
    c.free()


def test_mixed_proof_equals_the_builders_and_verifies(M, W, mixed, mixed_keys):
    from simpleworks_amd import serialization as Ser
    pk, vk = mixed_keys
    pub, priv = PM.mixed_inputs(3)[2]
    cs, public = W.program_circuit(mixed.tape, pub, priv)
    want = Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand()))
    got, outputs = M.generate_program_proof(pk, mixed, pub, priv, M.generate_rand())
    assert got == want and outputs == PM.mixed_eval(pub, priv)[0]
    inputs = W.program_public_inputs(mixed.tape, pub, outputs)
    assert inputs == public
    assert M.verify_proof(vk, inputs, M.MarlinProof(got), M.generate_rand())
    for k in (len(inputs) - 1, 9, 0):   # a flipped output bit (the last and the first one) and a flipped public-input bit
        other = list(inputs)
        other[k] ^= 1
        assert not M.verify_proof(vk, other, M.MarlinProof(got), M.generate_rand())
    # the prover is as it was for the next caller: the device source does not outlive the call
    assert Ser.serialize_proof(M.generate_proof(cs, pk, M.generate_rand())) == got


def test_test_circuit_program_proof_is_the_test_circuits(M, W, tc):
    from simpleworks_amd import serialization as Ser
    c, pk, vk = tc
    for a in (0xA7, 0, 255):
        want = Ser.serialize_proof(M.generate_proof(W.test_circuit(a, a), pk, M.generate_rand()))
        got, outputs = M.generate_program_proof(pk, c, [], [a, a], M.generate_rand())
        assert got == want and outputs == []
        assert M.verify_proof(vk, [], M.MarlinProof(got), M.generate_rand())


def test_a_refused_item_is_unsatisfied(M, mixed, mixed_keys, tc):
    pk, _ = mixed_keys
    rows = PM.mixed_inputs(65, underflow=(31,), div_zero=(64,))
    for i in (31, 64):
        with pytest.raises(M.MarlinError) as e:
            M.generate_program_proof(pk, mixed, rows[i][0], rows[i][1], M.generate_rand())
        assert e.value.code == -5
    c, tpk, _ = tc
    with pytest.raises(M.MarlinError) as e:
        M.generate_program_proof(tpk, c, [], [3, 4], M.generate_rand())
    assert e.value.code == -5


def test_proofs_of_a_batch_with_one_refused_item(M, W, mixed, mixed_keys):
    pk, vk = mixed_keys
    rows = PM.mixed_inputs(4, underflow=(1,))
    proofs, outputs, status = M.generate_program_proofs(pk, mixed, [p for p, _ in rows], [s for _, s in rows], M.generate_rand())
    assert status == [0, PM.UNDERFLOW, 0, 0] and proofs[1] is None
    assert outputs == [PM.mixed_eval(pub, priv)[0] for pub, priv in rows]
    rng = M.generate_rand()
    for i in (0, 2, 3):   # the single calls, in order on one rng
        single, out = M.generate_program_proof(pk, mixed, rows[i][0], rows[i][1], rng)
        assert proofs[i] == single and out == outputs[i]
        assert M.verify_proof(vk, W.program_public_inputs(mixed.tape, rows[i][0], out), M.MarlinProof(single), M.generate_rand())
    assert M.generate_program_proofs(pk, mixed, [], [], M.generate_rand()) == ([], [], [])


def test_proofs_of_a_batch_across_chunk_seams(M, mixed, mixed_keys):
    """swm_program_prove_many with the stage cap one byte short of an item (swm_selftest_witness_stage): every item is a chunk of its
    own, and the proofs are those of three single calls from the same rng state."""
    pk, _ = mixed_keys
    rows = PM.mixed_inputs(3)
    assert pk.ctx is mixed.ctx      # the prover's context is the one whose cap moves
    with mixed.ctx.selftest_witness_stage(32 * mixed.shape()[1] - 1):
        proofs, outputs, status = M.generate_program_proofs(pk, mixed, [p for p, _ in rows], [s for _, s in rows], M.generate_rand())
    assert status == [0, 0, 0] and outputs == [PM.mixed_eval(pub, priv)[0] for pub, priv in rows]
    rng = M.generate_rand()
    for i in range(3):
        single, out = M.generate_program_proof(pk, mixed, rows[i][0], rows[i][1], rng)
        assert proofs[i] == single and len(single) > 0 and out == outputs[i]

"""Integer programs: the reference's gadget vocabulary as one circuit, its witnesses synthesised on the GPU (csrc/program_witness.hip
through include/swmarlin.h).

Caller-facing mirror of the reference's integer gadgets (src/gadgets/{uint8,uint16,uint32,uint64,uint128,boolean}.rs behind the
traits of src/gadgets/traits.rs), name for name: a register of a Program carries
    .and_ .or_ .xor .nand .nor                              BitwiseOperationGadget (`and`, `or` are Python keywords)
    .add .sub .mul .div                                     ArithmeticGadget
    .shift_left .shift_right .rotate_left .rotate_right     BitShiftGadget / BitRotationGadget, by a constant number of positions
    .compare(other, "gt" | "gte" | "lt" | "lte")            ComparisonGadget
    .is_eq .enforce_equal  and  Program.select              ark's EqGadget and CondSelectGadget::conditionally_select
plus .not_ (ark's Boolean::not, bit by bit).  Where the reference synthesises a constraint system per execution, a Program records a
TAPE once (format: csrc/host/program_shape.h; circuit: workloads.build_program) and ProgramCircuit runs batches of executions of it.
The proof entries are marlin.generate_program_proof / generate_program_proofs.  There is no CPU evaluation path here: the model of
the circuit, workloads.build_program, is the specification the tests hold the GPU to.
"""
import ctypes

import numpy as np

from . import workloads as W
from .marlin import default_context, program_circuit_shape

BOOL, U8, U16, U32, U64, U128 = range(6)


class Register:
    """One SSA register of a Program: an index and a type."""
    __slots__ = ("program", "index", "type")

    def __init__(self, program, index, type_):
        self.program, self.index, self.type = program, index, type_

    def _binary(self, op, other, result=None):
        if other.program is not self.program or other.type != self.type:
            raise ValueError("%s: operands of one program and one type" % op)
        return self.program._emit(op, self.type, self.index, other.index, result=self.type if result is None else result)

    def and_(self, other):
        return self._binary("AND", other)

    def or_(self, other):
        return self._binary("OR", other)

    def xor(self, other):
        return self._binary("XOR", other)

    def nand(self, other):
        return self._binary("NAND", other)

    def nor(self, other):
        return self._binary("NOR", other)

    def not_(self):
        return self.program._emit("NOT", self.type, self.index, result=self.type)

    def add(self, other):
        return self._binary("ADD", other)

    def sub(self, other):
        return self._binary("SUB", other)

    def mul(self, other):
        return self._binary("MUL", other)

    def div(self, other):
        return self._binary("DIV", other)

    def _shift(self, op, positions):
        return self.program._emit(op, self.type, self.index, imm=int(positions), result=self.type)

    def shift_left(self, positions):
        return self._shift("SHL", positions)

    def shift_right(self, positions):
        return self._shift("SHR", positions)

    def rotate_left(self, positions):
        return self._shift("ROTL", positions)

    def rotate_right(self, positions):
        return self._shift("ROTR", positions)

    def compare(self, other, ordering):
        """ComparisonGadget::compare: ordering "gt", "gte", "lt" or "lte"; the result is a BOOL register."""
        if ordering not in ("gt", "gte", "lt", "lte"):
            raise ValueError("compare: ordering %r" % (ordering,))
        return self._binary(ordering.upper(), other, result=BOOL)

    def is_eq(self, other):
        return self._binary("EQ", other, result=BOOL)

    def enforce_equal(self, other):
        self._binary("ASSERT_EQ", other, result=-1)


class Program:
    """A straight-line program under construction.  Inputs first (public, then private), then the ops; tape() is what the library
    reads.  The validator (workloads.program_parse, csrc/host/program_shape.h) has the last word: tape() raises what it refuses."""

    def __init__(self):
        self._words = []
        self._registers = 0

    def _emit(self, op, type_, a=0, b=0, c=0, imm=0, result=-1):
        if not 0 <= imm < 1 << 128:
            raise ValueError("%s: immediate %d" % (op, imm))
        self._words.append(W.program_word(op, type_, a, b, c, imm))
        if result < 0:
            return None
        self._registers += 1
        return Register(self, self._registers - 1, result)

    def public_input(self, type_):
        return self._emit("INPUT_PUBLIC", type_, result=type_)

    def private_input(self, type_):
        return self._emit("INPUT_PRIVATE", type_, result=type_)

    def constant(self, type_, value):
        return self._emit("CONST", type_, imm=int(value), result=type_)

    def select(self, condition, if_true, if_false):
        """conditionally_select(condition, if_true, if_false)."""
        if condition.type != BOOL or if_true.type != if_false.type or not condition.program is if_true.program is if_false.program is self:
            raise ValueError("select: a BOOL and two registers of one type, all of this program")
        return self._emit("SELECT", if_true.type, condition.index, if_true.index, if_false.index, result=if_true.type)

    def output(self, register):
        self._emit("OUTPUT", register.type, register.index)

    def tape(self):
        tape = W.program_header(len(self._words)) + b"".join(self._words)
        W.program_parse(tape)
        return tape


def pack_inputs(layout_or_program, public, private):
    """The input bytes of a batch: public[i] and private[i] are item i's values in declaration order -> uint8 [count, input_bytes]."""
    ins, _ = W.program_parse(layout_or_program)
    pub = [t for name, t, *_ in ins if name == "INPUT_PUBLIC"]
    priv = [t for name, t, *_ in ins if name == "INPUT_PRIVATE"]
    if len(public) != len(private):
        raise ValueError("as many public as private rows")
    rows = []
    for pv, sv in zip(public, private):
        if len(pv) != len(pub) or len(sv) != len(priv):
            raise ValueError("a program of %d public and %d private inputs" % (len(pub), len(priv)))
        rows.append(b"".join((int(v) & ((1 << W.program_type_width(t)) - 1)).to_bytes(W.program_type_bytes(t), "little")
                             for t, v in zip(pub + priv, list(pv) + list(sv))))
    n = sum(W.program_type_bytes(t) for t in pub + priv)
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), n).copy()


def unpack_outputs(program, outputs):
    """uint8 [count, output_bytes] -> per item the list of output values, in OUTPUT order."""
    ins, _ = W.program_parse(program)
    sizes = [W.program_type_bytes(t) for name, t, *_ in ins if name == "OUTPUT"]
    rows = []
    for row in np.asarray(outputs, dtype=np.uint8):
        raw, at, vals = row.tobytes(), 0, []
        for n in sizes:
            vals.append(int.from_bytes(raw[at:at + n], "little"))
            at += n
        rows.append(vals)
    return rows


class ProgramCircuit:
    """swm_program: a validated tape and its compiled plan, resident on the context's device.  Synthesises the witness vector of
    workloads.build_program for batches of executions without running the builder."""

    def __init__(self, program, ctx=None):
        self.tape = bytes(program.tape() if hasattr(program, "tape") else program)
        self._shape = program_circuit_shape(self.tape)   # refuses what the validator refuses
        self.layout = W.program_circuit_layout(self.tape)
        self.ctx = ctx or default_context()
        h = ctypes.c_void_p()
        buf = (ctypes.c_uint8 * len(self.tape)).from_buffer_copy(self.tape)
        self.ctx._check(self.ctx.lib.swm_program_create(self.ctx.h, buf, len(self.tape), ctypes.byref(h)), "swm_program_create")
        self.h = h

    def shape(self):
        """(num_instance, num_witness, num_constraints)."""
        return self._shape

    def witness_bytes(self, inputs):
        """inputs: uint8 [count, input_bytes] -> (witness uint64 [count, num_witness, 4], outputs uint8 [count, output_bytes],
        status uint8 [count]): swm_program_witness."""
        a = np.ascontiguousarray(inputs, dtype=np.uint8)
        if a.ndim != 2 or a.shape[1] != self.layout["input_bytes"]:
            raise ValueError("inputs: a (count, %d) uint8 array" % self.layout["input_bytes"])
        count = a.shape[0]
        witness = np.zeros((count, self._shape[1], 4), dtype=np.uint64)
        outputs = np.zeros((count, self.layout["output_bytes"]), dtype=np.uint8)
        status = np.zeros(count, dtype=np.uint8)
        self.ctx._check(self.ctx.lib.swm_program_witness(self.ctx.h, self.h, a.ctypes.data if a.size else None, count,
                                                         witness.ctypes.data if witness.size else None,
                                                         outputs.ctypes.data if outputs.size else None, status.ctypes.data),
                        "swm_program_witness")
        return witness, outputs, status

    def witness_many(self, public, private):
        """One pass (chunks above 1 GiB of witnesses) over the executions with the values public[i], private[i].  Returns (witness
        uint64 [count, num_witness, 4] Montgomery limbs, outputs: per item the list of output values, status uint8 [count]);
        workloads.program_public_inputs(program, public[i], outputs[i]) are an item's public inputs."""
        witness, outputs, status = self.witness_bytes(pack_inputs(self.tape, public, private))
        return witness, unpack_outputs(self.tape, outputs), status

    def witness_dev(self, d_inputs, count, d_witness, d_outputs=None, d_status=None):
        """swm_program_witness_dev on device pointers (ints or objects with .ptr)."""
        def ptr(b):
            return None if b is None else b if isinstance(b, int) else b.ptr
        self.ctx._check(self.ctx.lib.swm_program_witness_dev(self.ctx.h, self.h, ptr(d_inputs), count, ptr(d_witness), ptr(d_outputs),
                                                             ptr(d_status)), "swm_program_witness_dev")

    def free(self):
        if self.h:
            self.ctx.lib.swm_program_destroy(self.ctx.h, self.h)
            self.h = None

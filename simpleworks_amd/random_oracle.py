"""The Blake2s random oracle, computed on the GPU (csrc/blake2s.hip and csrc/blake2s_witness.hip through include/swmarlin.h).

Caller-facing mirror of the reference's RandomOracle for Blake2s (src/schnorr_signature/blake2s.rs and
examples/simple-payments/random_oracle/blake2s/mod.rs), name for name:
    RO::setup(rng)                      -> ()   (no parameters)
    RO::evaluate(&parameters, input)    -> [u8; 32], unkeyed BLAKE2s-256 of the input
plus evaluate_many, the batched form (one GPU lane per input), and Blake2sCircuit, which synthesises the witness of
workloads.build_blake2s_hash — the gadget side, ROGadget::evaluate of random_oracle/blake2s/constraints.rs — for batches of
inputs without running the builder.  The proof entry is marlin.generate_blake2s_proof.  There is no CPU evaluation path here.
"""
import numpy as np

from .marlin import blake2s_circuit_shape, default_context


def _rows(inputs, input_len=None):
    """uint8 [count, input_len] from an array of that shape or from equally long byte strings."""
    if isinstance(inputs, np.ndarray):
        a = np.ascontiguousarray(inputs, dtype=np.uint8)
    else:
        rows = [bytes(m) for m in inputs]
        if len({len(m) for m in rows}) > 1:
            raise ValueError("the inputs of one call have one length")
        n = len(rows[0]) if rows else (input_len or 0)
        a = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), n)
    if a.ndim != 2 or (input_len is not None and a.shape[1] != input_len):
        raise ValueError("inputs: a (count, input_len) uint8 array" + ("" if input_len is None else " with input_len %d" % input_len))
    return a


def evaluate_many(inputs, ctx=None):
    """inputs: uint8 [count, input_len] (or equally long byte strings) -> uint8 [count, 32]: RO::evaluate of each, one launch."""
    return (ctx or default_context()).blake2s_hash(_rows(inputs))


class RO:
    """blake2s::RO, the RandomOracle implementation: Parameters = (), Output = [u8; 32]."""

    @staticmethod
    def setup(rng=None):
        """RO::setup: nothing to sample."""
        return ()

    @staticmethod
    def evaluate(parameters, input, ctx=None):
        """RO::evaluate(&(), input) -> the 32 digest bytes."""
        if parameters != ():
            raise ValueError("the Blake2s random oracle has no parameters: pass RO.setup(rng)")
        a = np.frombuffer(bytes(input), dtype=np.uint8).reshape(1, -1)
        return evaluate_many(a, ctx)[0].tobytes()


class Blake2sCircuit:
    """The Blake2s hash circuit over input_len bytes: synthesises the witness vector of workloads.build_blake2s_hash for batches
    of inputs on the GPU, one workgroup per input.  No handle: the shape follows from input_len."""

    def __init__(self, input_len, ctx=None):
        self.input_len = int(input_len)
        self._shape = blake2s_circuit_shape(self.input_len)   # refuses input_len > 65536
        self.ctx = ctx or default_context()

    def shape(self):
        """(num_instance, num_witness, num_constraints)."""
        return self._shape

    def witness_many(self, inputs):
        """One launch (chunks above 1 GiB of witnesses).  Returns (witness uint64 [count, num_witness, 4] Montgomery limbs,
        digests uint8 [count, 32]); workloads.blake2s_public_inputs(digest) are an item's public inputs."""
        return self.ctx.blake2s_witness(self._shape[1], _rows(inputs, self.input_len))

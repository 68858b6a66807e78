"""Native Schnorr signatures on ed-on-BLS12-377, computed on the GPU (csrc/schnorr.hip through include/swmarlin.h).

Caller-facing mirror of src/schnorr_signature/schnorr.rs (SimpleSchnorr = Schnorr<EdwardsProjective>), name for name:
    :57-62     setup(rng)                          -> Parameters { generator = prime_subgroup_generator(), salt = None }
    :64-80     keygen(params, rng)                 -> (PublicKey, SecretKey { secret_key, public_key })
    :82-124    sign(params, sk, message, rng)      -> Signature { prover_response, verifier_challenge }
    :126-160   verify(params, pk, message, sig)    -> bool
as examples/schnorr-signature/main.rs:79-100 and examples/simple-payments call them, plus keygen_many / sign_many / verify_many,
the batched forms a payments-style caller wants: one GPU lane per key, signature or check.

Host side (this file): the random draws and the bookkeeping.  A scalar is drawn the way ark-ff 0.3's UniformRand does for a
256-bit field [U]: 32 bytes from the generator, the top 256 - 251 = 5 bits cleared, retried while >= the group order; the accepted
limbs are read as the Montgomery representation, so the value is limbs / 2^256 mod l.  keygen draws one scalar per key, sign one
per signature, in order, as the reference does.  That the generator below is arkworks' constant is [U]; it is on the curve and of
order l.  Every curve operation and every hash runs on the GPU; there is no CPU evaluation path here.
"""
import numpy as np

from .marlin import default_context

GROUP_ORDER = 2111115437357092606062206234695386632838870926408408195193685246394721360383   # l, 251 bits
GENERATOR = (4497879464030519973909970603271755437257548612157028181994697785683032656389,
             4357141146396347889246900916607623952598927460421559113092863576544024487809)
_MONT_RINV = pow(1 << 256, -1, GROUP_ORDER)


def rand_scalar(rng):
    """ScalarField::rand(rng) [U] (see the module docstring)."""
    while True:
        v = int.from_bytes(rng.fill_bytes(32), "little") & ((1 << 251) - 1)
        if v < GROUP_ORDER:
            return v * _MONT_RINV % GROUP_ORDER


def point_bytes(p):
    """to_bytes! of an affine point: x || y, 32 little-endian bytes each."""
    return p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")


def point_from_bytes(b):
    b = bytes(b)
    return int.from_bytes(b[:32], "little"), int.from_bytes(b[32:64], "little")


class Parameters:
    """schnorr::Parameters { generator, salt } with the generator's table resident on the GPU."""

    def __init__(self, generator=GENERATOR, salt=None, ctx=None):
        self.ctx = ctx or default_context()
        self.generator = generator
        self.salt = bytes(salt) if salt is not None else None
        self.h = self.ctx.schnorr_create(point_bytes(generator), self.salt)

    def free(self):
        if self.h:
            self.ctx.schnorr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class SecretKey:
    def __init__(self, secret_key, public_key):
        self.secret_key, self.public_key = secret_key, public_key


class Signature:
    def __init__(self, prover_response, verifier_challenge):
        self.prover_response, self.verifier_challenge = prover_response, bytes(verifier_challenge)

    def to_bytes(self):
        return self.prover_response.to_bytes(32, "little") + self.verifier_challenge

    @staticmethod
    def from_bytes(b):
        b = bytes(b)
        return Signature(int.from_bytes(b[:32], "little"), b[32:64])


class SchnorrCircuit:
    """The Schnorr verification circuit for messages of `msg_len` bytes under `params` (its generator and salt), resident on the
    GPU (swm_schnorr_circuit): synthesises the witness vector of workloads.build_schnorr_verification for batches of
    (public key, message, signature) without running the builder.  Refers to the Parameters: keep them alive."""

    def __init__(self, params, msg_len):
        self.ctx, self.params, self.msg_len = params.ctx, params, int(msg_len)
        self.h = self.ctx.schnorr_circuit_create(params.h, self.msg_len)

    def shape(self):
        """(num_instance, num_witness, num_constraints)."""
        from .marlin import schnorr_circuit_shape
        return schnorr_circuit_shape(self.msg_len, self.params.salt is not None)

    def witness_many(self, public_keys, messages, signatures):
        """public_keys uint8 [count, 64], messages uint8 [count, msg_len] (or byte strings of that length), signatures uint8
        [count, 64].  One launch per staged chunk.  Returns (witness uint64 [count, num_witness, 4] Montgomery limbs, ok bool
        [count]: the signature verifies in the circuit's sense, i.e. the witness satisfies it)."""
        pk = np.ascontiguousarray(public_keys, dtype=np.uint8).reshape(-1, 64)
        sig = np.ascontiguousarray(signatures, dtype=np.uint8).reshape(-1, 64)
        if not isinstance(messages, np.ndarray):
            if any(len(m) != self.msg_len for m in messages):
                raise ValueError("a message of this circuit has %d bytes" % self.msg_len)
            messages = np.frombuffer(b"".join(bytes(m) for m in messages), dtype=np.uint8)
        m = np.ascontiguousarray(messages, dtype=np.uint8).reshape(pk.shape[0], self.msg_len)
        witness, ok = self.ctx.schnorr_witness(self.h, self.shape()[1], pk, m, sig)
        return witness, ok != 0

    def free(self):
        if self.h:
            self.ctx.schnorr_circuit_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _scalars(values):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(len(values), 32)


def _by_length(messages):
    """messages: uint8 [count, msg_len], or a sequence of byte strings -> [(indices, uint8 [len(indices), msg_len])], one per length."""
    if isinstance(messages, np.ndarray):
        return [(np.arange(messages.shape[0]), messages)]
    groups = {}
    for i, m in enumerate(messages):
        groups.setdefault(len(m), []).append(i)
    return [(np.asarray(idx), np.frombuffer(b"".join(bytes(messages[i]) for i in idx), dtype=np.uint8).reshape(len(idx), ln))
            for ln, idx in groups.items()]


def setup(rng=None, ctx=None):
    """SignatureScheme::setup: the generator is fixed and there is no salt; like the reference, this draws nothing from rng."""
    return Parameters(GENERATOR, None, ctx)


def keygen_many(params, rng, count):
    """count keys -> (public keys uint8 [count, 64], secret keys uint8 [count, 32]); one draw per key."""
    sk = _scalars([rand_scalar(rng) for _ in range(count)])
    return params.ctx.schnorr_keygen(params.h, sk), sk


def sign_many(params, secret_keys, public_keys, messages, rng=None, nonces=None):
    """One signature per (secret key, public key, message) -> uint8 [count, 64] (prover_response || verifier_challenge).
    secret_keys uint8 [count, 32], public_keys uint8 [count, 64]; messages uint8 [count, msg_len] or a sequence of byte strings,
    which are grouped by length (one launch per length).  The nonces are drawn from rng, one per signature in order, unless given."""
    sk = np.ascontiguousarray(secret_keys, dtype=np.uint8).reshape(-1, 32)
    pk = np.ascontiguousarray(public_keys, dtype=np.uint8).reshape(-1, 64)
    k = _scalars([rand_scalar(rng) for _ in range(sk.shape[0])]) if nonces is None else np.ascontiguousarray(nonces, dtype=np.uint8).reshape(-1, 32)
    out = np.empty((sk.shape[0], 64), dtype=np.uint8)
    for idx, m in _by_length(messages):
        out[idx] = params.ctx.schnorr_sign(params.h, sk[idx], pk[idx], k[idx], m)
    return out


def verify_many(params, public_keys, messages, signatures):
    """-> bool [count]; arguments as in sign_many."""
    pk = np.ascontiguousarray(public_keys, dtype=np.uint8).reshape(-1, 64)
    sig = np.ascontiguousarray(signatures, dtype=np.uint8).reshape(-1, 64)
    ok = np.zeros(pk.shape[0], dtype=bool)
    for idx, m in _by_length(messages):
        ok[idx] = params.ctx.schnorr_verify(params.h, pk[idx], m, sig[idx]) != 0
    return ok


def keygen(params, rng):
    pk, sk = keygen_many(params, rng, 1)
    pk = point_from_bytes(pk[0].tobytes())
    return pk, SecretKey(int.from_bytes(sk[0].tobytes(), "little"), pk)


def sign(params, sk, message, rng):
    sig = sign_many(params, _scalars([sk.secret_key]), np.frombuffer(point_bytes(sk.public_key), dtype=np.uint8), [bytes(message)], rng)
    return Signature.from_bytes(sig[0].tobytes())


def verify(params, pk, message, sig):
    return bool(verify_many(params, np.frombuffer(point_bytes(pk), dtype=np.uint8), [bytes(message)],
                            np.frombuffer(sig.to_bytes(), dtype=np.uint8))[0])

"""Mirror of /root/reference/src/marlin/serialization.rs:5-45 (ark-serialize CanonicalSerialize byte strings)."""
import ctypes

from ._lib import load_library, _vp
from .marlin import MarlinError, MarlinProof, ProvingKey, VerifyingKey, _check, default_context


def serialize_proof(proof):
    return bytes(proof.data)


def deserialize_proof(bytes_proof):
    data = bytes(bytes_proof)
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    _check(load_library().swm_proof_validate(buf, len(data)), "Error deserializing proof")
    return MarlinProof(data)


def proof_recode(data, to_uncompressed):
    """swm_proof_recode: the proof between the compressed (CanonicalSerialize::serialize, what serialization.rs:5-17 moves) and
    the uncompressed (serialize_uncompressed, what swm_generate_proof_ex(SWM_PROOF_UNCOMPRESSED) writes) forms; checked parse."""
    data = bytes(data)
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    out = (ctypes.c_uint8 * 4096)()
    n = ctypes.c_size_t(0)
    _check(load_library().swm_proof_recode(buf, len(data), 1 if to_uncompressed else 0, out, len(out), ctypes.byref(n)),
           "Error recoding proof")
    return bytes(out[: n.value])


# swm_{pk,vk}_{serialize,deserialize}_ex: which of arkworks' three forms of a key (include/swmarlin.h)
KEY_UNCOMPRESSED = 1  # serialize_uncompressed / deserialize_uncompressed
KEY_UNCHECKED = 2     # readers, with KEY_UNCOMPRESSED: deserialize_unchecked — the caller vouches for the bytes


def _key_flags(uncompressed, unchecked=False):
    return (KEY_UNCOMPRESSED if uncompressed else 0) | (KEY_UNCHECKED if unchecked else 0)


def serialize_verifying_key(verifying_key, uncompressed=False):
    lib = load_library()
    flags = _key_flags(uncompressed)
    n = ctypes.c_size_t(0)
    _check(lib.swm_vk_serialize_ex(verifying_key.h, flags, None, 0, ctypes.byref(n)), "Error serializing verifying key")
    buf = (ctypes.c_uint8 * n.value)()
    _check(lib.swm_vk_serialize_ex(verifying_key.h, flags, buf, n.value, ctypes.byref(n)), "Error serializing verifying key")
    return bytes(buf)


def deserialize_verifying_key(bytes_verifying_key, uncompressed=False, unchecked=False):
    """unchecked (only with uncompressed; anything else is refused): deserialize_unchecked, for bytes this library wrote or a
    checked load accepted."""
    data = bytes(bytes_verifying_key)
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    h = _vp()
    rc = load_library().swm_vk_deserialize_ex(buf, len(data), _key_flags(uncompressed, unchecked), ctypes.byref(h))
    if rc != 0:
        raise MarlinError(rc, "Error deserializing verifying key")
    return VerifyingKey(h)


def serialize_proving_key(proving_key, uncompressed=False):
    ctx = proving_key.ctx
    flags = _key_flags(uncompressed)
    n = ctypes.c_size_t(0)
    _check(ctx.lib.swm_pk_serialize_ex(ctx.h, proving_key.h, flags, None, 0, ctypes.byref(n)), "Error serializing proving key", ctx)
    buf = (ctypes.c_uint8 * n.value)()
    _check(ctx.lib.swm_pk_serialize_ex(ctx.h, proving_key.h, flags, buf, n.value, ctypes.byref(n)), "Error serializing proving key", ctx)
    return bytes(buf)


def deserialize_proving_key(bytes_proving_key, ctx=None, uncompressed=False, unchecked=False):
    """uncompressed: the serialize_uncompressed form, its two power ranges decoded on the GPU and kept there.  unchecked (only with
    uncompressed): no curve or subgroup test — for bytes this library wrote or a checked load accepted, never for a peer's."""
    ctx = ctx or default_context()
    data = bytes(bytes_proving_key)
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    h = _vp()
    _check(ctx.lib.swm_pk_deserialize_ex(ctx.h, buf, len(data), _key_flags(uncompressed, unchecked), ctypes.byref(h)),
           "Error deserializing proving key", ctx)
    return ProvingKey(ctx, h)

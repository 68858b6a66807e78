"""Big-integer restatement of the reference's Schnorr scheme on ed-on-BLS12-377 (TEST INFRASTRUCTURE ONLY; lives under tests/
because oracle/ is frozen).

What the reference states (src/schnorr_signature/schnorr.rs, SimpleSchnorr = Schnorr<EdwardsProjective>):
    :57-62     setup: salt = None, generator = prime_subgroup_generator()
    :64-80     keygen: x = ScalarField::rand(rng), pk = x G
    :82-124    sign: k = ScalarField::rand(rng), R = k G, e = Blake2s([salt] || to_bytes![pk] || to_bytes![R] || message),
               s = k - from_le_bytes_mod_order(e) * x; signature = (s, e)
    :126-160   verify: R' = s G + from_le_bytes_mod_order(e) pk, accept iff Blake2s([salt] || pk || R' || message) == e
to_bytes! of a twisted Edwards affine point is x || y, 32 little-endian bytes each in standard form [U]; a scalar is 32
little-endian bytes.  Curve arithmetic is pyref.pedersen's affine unified law, the hash is hashlib's.
A scalar multiplication costs tens of milliseconds here: bulk cases come from tests/golden/schnorr.json, not from this file.
"""
import hashlib

from pyref.bls12_377 import R
from pyref.pedersen import ED_SUBGROUP_ORDER as L
from pyref.pedersen import ed_add, ed_mul, ed_on_curve

# ark-ed-on-bls12-377 prime-subgroup generator [U]; on the curve and of order L (asserted by the fixture's generator script)
GENERATOR = (4497879464030519973909970603271755437257548612157028181994697785683032656389,
             4357141146396347889246900916607623952598927460421559113092863576544024487809)
IDENTITY = (0, 1)
_MONT_RINV_L = pow(1 << 256, -1, L)


def point_bytes(p):
    return p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")


def point_from_bytes(b):
    """(x, y), or None when a coordinate is not canonical or the point is off the curve (no arkworks value holds either)."""
    x, y = int.from_bytes(b[:32], "little"), int.from_bytes(b[32:64], "little")
    if x >= R or y >= R or not ed_on_curve((x, y)):
        return None
    return x, y


def ed_neg(p):
    return (-p[0]) % R, p[1]


def hash_input(salt, pk, commitment, message):
    """schnorr.rs:98-104 / :146-152: every byte of the hash input."""
    return (bytes(salt) if salt is not None else b"") + point_bytes(pk) + point_bytes(commitment) + bytes(message)


def challenge(salt, pk, commitment, message):
    return hashlib.blake2s(hash_input(salt, pk, commitment, message), digest_size=32).digest()


def keygen(generator, secret):
    return ed_mul(generator, secret % L)


def sign(generator, salt, secret, pk, nonce, message):
    """-> 64 bytes: prover_response (32 LE) || verifier_challenge (schnorr.rs:43-46)."""
    e = challenge(salt, pk, ed_mul(generator, nonce), message)
    s = (nonce - int.from_bytes(e, "little") % L * secret) % L
    return s.to_bytes(32, "little") + e


def commitment(generator, pk, response, challenge_bytes):
    """schnorr.rs:140-143: s G + (e mod L) pk, for any on-curve pk (in the subgroup or not)."""
    e = int.from_bytes(challenge_bytes, "little") % L
    return ed_add(ed_mul(generator, response), ed_mul(pk, e))


def verify(generator, salt, pk_bytes, message, sig):
    pk = point_from_bytes(pk_bytes)
    s = int.from_bytes(sig[:32], "little")
    if pk is None or s >= L:
        return False
    return challenge(salt, pk, commitment(generator, pk, s, sig[32:64]), message) == bytes(sig[32:64])


def draw_scalar(rng):
    """ark-ff 0.3 UniformRand for Fp256 [U]: four u64 limbs from the generator (32 bytes of its stream), the top 256 - 251 = 5
    bits cleared, retried while >= L; the accepted limbs ARE the Montgomery representation (value = limbs / 2^256 mod L).
    rng: pyref.rng.ChaChaRng."""
    while True:
        v = sum(rng.next_u64() << (64 * i) for i in range(4)) & ((1 << 251) - 1)
        if v < L:
            return v * _MONT_RINV_L % L

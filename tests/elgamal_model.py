"""Big-integer restatement of ElGamal encryption on ed-on-BLS12-377 (TEST INFRASTRUCTURE ONLY; lives under tests/ because
oracle/ is frozen).

What the reference exercises (tests/encrypt.rs:11-28) of ark-crypto-primitives 0.3, encryption/elgamal/mod.rs [U],
ElGamal<EdwardsProjective>:
    setup(rng)            generator = C::rand(rng)                       a random point of the prime subgroup
    keygen(pp, rng)       sk = ScalarField::rand(rng); pk = sk generator
    Randomness::rand      ScalarField::rand(rng)
    encrypt(pp, pk, m, r) s = r pk; c1 = r generator; c2 = m + s         the ciphertext is (c1, c2)
    decrypt(pp, sk, c)    s = sk c1; m = c2 + (-s)
The curve functions are tests/schnorr_model.py's (pyref.pedersen's affine unified law), the draws pyref's: C::rand is
pyref.pedersen.ed_rand, ScalarField::rand schnorr_model.draw_scalar.  tests/encrypt.rs draws in the order generator, sk, message, r.
A scalar multiplication costs tens of milliseconds here: bulk cases come from tests/golden/elgamal.json, not from this file.
"""
from pyref.pedersen import ed_add, ed_mul, ed_rand

from schnorr_model import IDENTITY, draw_scalar, ed_neg, point_bytes, point_from_bytes  # noqa: F401  (the wire forms are Schnorr's)


def setup(rng):
    """-> the generator."""
    return ed_rand(rng)


def keygen(generator, rng):
    """-> (pk, sk)."""
    sk = draw_scalar(rng)
    return ed_mul(generator, sk), sk


def rand_plaintext(rng):
    """JubJub::rand(rng).into()."""
    return ed_rand(rng)


def rand_randomness(rng):
    return draw_scalar(rng)


def encrypt(generator, pk, message, r):
    """-> (c1, c2), for any on-curve pk and message (in the subgroup or not) and any integer r: mul is the integer multiple."""
    return ed_mul(generator, r), ed_add(message, ed_mul(pk, r))


def decrypt(sk, ciphertext):
    c1, c2 = ciphertext
    return ed_add(c2, ed_neg(ed_mul(c1, sk)))


def ciphertext_bytes(ciphertext):
    """c1.x || c1.y || c2.x || c2.y: the 128 bytes of the C ABI."""
    return point_bytes(ciphertext[0]) + point_bytes(ciphertext[1])

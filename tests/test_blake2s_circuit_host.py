"""CPU tests of the Blake2s hash circuit: its specification, workloads.build_blake2s_hash, evaluated row by row in Python integers on
inputs at every block boundary and on tampered assignments, the digest read from the assignment against hashlib (the outside
yardstick) and three known answers, and its SHAPE as the library states it without a GPU (swm_blake2s_circuit_shape,
csrc/host/blake2s_shape.h): the GPU witness synthesis (csrc/blake2s_witness.hip) lays its output out by these counts."""
import ctypes
import hashlib
import os
import shutil
import subprocess

import pytest

from simpleworks_amd import marlin as M, workloads as W
from simpleworks_amd._lib import load_library

R = W.R_MODULUS
LENGTHS = (0, 1, 31, 32, 55, 63, 64, 65, 127, 128, 129)
KNOWN = ((b"abc", "508c5e8c327c14e2e1a72ba34eeb452f37458b209ed63a294d999b4c86675982"),          # RFC 7693, appendix B
         (bytes([1] * 32), "5da8bcf5e934a097c5a5a62fa8dd942da80501ee8de6df858499c6181325e369"),  # the reference's unit test
         (b"", "69217a3079908094e11121d042354a7c1f55b6482ca1a51e1b250dfd1ed0eef9"))


def message(length, seed=0):
    """A fixed input of `length` bytes: no byte pattern repeats with the block or the word."""
    return bytes((37 * i + 11 * seed + (i >> 3) + 1) & 0xFF for i in range(length))


def _failing_rows(cs, instance=None, witness=None):
    """The row evaluator: every row a z * b z == c z in Python integers; returns the indices of the rows that fail."""
    z = {("i", k): v for k, v in enumerate(cs.instance if instance is None else instance)}
    z.update({("w", k): v for k, v in enumerate(cs.witness if witness is None else witness)})

    def ev(lc):
        return sum(c * z[v] for c, v in lc) % R
    return [i for i, (a, b, c) in enumerate(zip(*cs.rows)) if ev(a) * ev(b) % R != ev(c)]


def _shape(input_len):
    lib = load_library()
    ni, nw, nc = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = lib.swm_blake2s_circuit_shape(input_len, ctypes.byref(ni), ctypes.byref(nw), ctypes.byref(nc))
    return rc, (ni.value, nw.value, nc.value)


def _digest_of(cs, lay):
    """The 32 digest bytes read from the assignment: word i, bit j at digest + 64 i + j."""
    out = bytearray(32)
    for i in range(8):
        for j in range(32):
            bit = cs.witness[lay["digest"] + 64 * i + j]
            assert bit in (0, 1)
            out[4 * i + j // 8] |= bit << (j % 8)
    return bytes(out)


@pytest.fixture(scope="module")
def ones():
    """The reference's own case: [1u8; 32]."""
    return W.blake2s_hash_circuit(bytes([1] * 32))


@pytest.mark.parametrize("length", LENGTHS)
def test_shape_rows_and_digest(length):
    """The library's three counts and the layout's are the builder's, every row holds, and the digest in the assignment and in the
    instance is hashlib's."""
    data = message(length)
    cs, public = W.blake2s_hash_circuit(data)
    blocks = max(1, (length + 63) // 64)
    counts = (len(cs.instance), len(cs.witness), cs.num_constraints)
    assert counts == (3, 8 * length + 21472 * blocks, 8 * length + 21792 * blocks + 2)
    rc, got = _shape(length)
    assert rc == 0 and got == counts == M.blake2s_circuit_shape(length)
    lay = W.blake2s_circuit_layout(length)
    assert (lay["num_instance"], lay["num_witness"], lay["num_constraints"]) == counts
    assert lay["bits"] == 0 and lay["b2s"] == 8 * length and lay["blocks"] == blocks
    assert _failing_rows(cs) == []
    assert cs.witness[:8 * length] == [(byte >> k) & 1 for byte in data for k in range(8)]
    assert all(v in (0, 1) for v in cs.witness)
    want = hashlib.blake2s(data).digest()
    assert _digest_of(cs, lay) == want
    assert public == cs.instance[1:] == W.blake2s_public_inputs(want)
    assert public == [int.from_bytes(want[:16], "little"), int.from_bytes(want[16:], "little")] and max(public) < 1 << 128


def test_the_counts_the_issue_states():
    assert M.blake2s_circuit_shape(32) == (3, 21728, 22050)
    assert M.blake2s_circuit_shape(0) == (3, 21472, 21794)
    assert M.blake2s_circuit_shape(65536) == (3, 8 * 65536 + 21472 * 1024, 8 * 65536 + 21792 * 1024 + 2)


@pytest.mark.parametrize("data,digest", KNOWN)
def test_known_answers(data, digest):
    assert hashlib.blake2s(data).hexdigest() == digest
    cs, public = W.blake2s_hash_circuit(data)
    assert _digest_of(cs, W.blake2s_circuit_layout(len(data))).hex() == digest
    assert public == W.blake2s_public_inputs(bytes.fromhex(digest))
    assert _failing_rows(cs) == []


def test_the_shape_depends_on_the_length_alone(ones):
    """Nothing is folded into constants: all zero, all ones and a mixed input of one length give the same rows."""
    cs, _ = ones
    for data in (bytes(32), bytes([0xFF] * 32), message(32)):
        other, _ = W.blake2s_hash_circuit(data)
        assert other.rows == cs.rows


def test_a_flipped_message_bit_breaks_a_hash_row(ones):
    """The bit flipped in place, nothing recomputed: its booleanity row still holds, rows of the hash that read it do not.  The honest
    witness of the flipped input against the published digest: only the packing rows fail."""
    cs, public = ones
    witness = list(cs.witness)
    witness[8 * 5 + 3] ^= 1
    bad = _failing_rows(cs, witness=witness)
    assert bad and all(256 <= i < cs.num_constraints - 2 for i in bad)
    data = bytearray([1] * 32)
    data[5] ^= 1 << 3
    other, other_public = W.blake2s_hash_circuit(bytes(data))
    assert other.rows == cs.rows and other_public != public
    assert _failing_rows(cs, witness=other.witness) == [cs.num_constraints - 2, cs.num_constraints - 1]


def test_another_public_digest_breaks_its_packing_row_only(ones):
    cs, (lo, hi) = ones
    assert _failing_rows(cs, instance=[1, (lo + 1) % R, hi]) == [cs.num_constraints - 2]
    assert _failing_rows(cs, instance=[1, lo, (hi + 1) % R]) == [cs.num_constraints - 1]


def test_a_bit_of_two_fails_its_booleanity_row(ones):
    cs, _ = ones
    witness = list(cs.witness)
    witness[17] = 2
    bad = _failing_rows(cs, witness=witness)
    assert [i for i in bad if i < 256] == [17]


def test_limits():
    lib = load_library()
    n = ctypes.c_size_t(0)
    assert _shape(65536)[0] == 0
    for length in (65537, 1 << 40, (1 << 64) - 1):
        assert _shape(length)[0] == -1, length
    assert lib.swm_last_error(None).decode().startswith("blake2s_circuit_shape")
    assert lib.swm_blake2s_circuit_shape(32, None, ctypes.byref(n), ctypes.byref(n)) == -1
    assert lib.swm_blake2s_circuit_shape(32, ctypes.byref(n), None, ctypes.byref(n)) == -1
    assert lib.swm_blake2s_circuit_shape(32, ctypes.byref(n), ctypes.byref(n), None) == -1
    with pytest.raises(M.MarlinError) as e:
        M.blake2s_circuit_shape(65537)
    assert e.value.code == -1
    assert W.blake2s_circuit_layout(65536)["num_witness"] == 8 * 65536 + 21472 * 1024
    for length in (-1, 65537):
        with pytest.raises(ValueError):
            W.blake2s_circuit_layout(length)
    with pytest.raises(ValueError):
        W.build_blake2s_hash(M.ConstraintSystem(), bytes(65537))
    with pytest.raises(ValueError):
        W.blake2s_public_inputs(bytes(31))


def test_synthesizer_class(ones):
    cs, public = ones
    again = M.MarlinInst._synthesize(W.Blake2sHashCircuit([1] * 32))
    assert again.witness == cs.witness and again.rows == cs.rows and again.instance == [1] + public


def test_header_binding_and_ffi_declare_the_six_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ffi = open(os.path.join(root, "swmarlin-sys", "src", "ffi.rs")).read()
    hdr = open(os.path.join(root, "include", "swmarlin.h")).read()
    for name in ("swm_blake2s_hash", "swm_blake2s_hash_dev", "swm_blake2s_circuit_shape", "swm_blake2s_witness", "swm_blake2s_witness_dev",
                 "swm_blake2s_prove"):
        assert "pub fn %s(" % name in ffi and "%s(" % name in hdr
        assert hasattr(load_library(), name)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shape_under_asan_ubsan(tmp_path):
    """csrc/host/blake2s_shape.h — the counts, the offsets, the witness-to-recorded-word map and the message-word reader the kernels
    work by — against a brute-force walk and csrc/host/blake2s.h's digest, in a stand-alone program
    (tests/native/blake2s_shape_check.cpp) built with -fsanitize=address,undefined."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "blake2s_shape_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(root, "simpleworks_amd", "csrc"), os.path.join(root, "tests", "native", "blake2s_shape_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and ("asan" in out.stderr.lower() or "ubsan" in out.stderr.lower()) and "error:" not in out.stderr:
        pytest.skip("this g++ has no ASan / UBSan runtime")
    assert out.returncode == 0, out.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split() == ["ok", "202", "24"]   # input_len 0 .. 200 and 65536; six lengths in batches of 1 and 3

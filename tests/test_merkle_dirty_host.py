"""CPU tests of what the resident Merkle tree and the ledger decide on the host: the dirty set of a batch of updates
(csrc/host/merkle_dirty.h, which merkle_tree.hip turns into launches) against a brute-force model, and the byte strings of
simpleworks_amd/ledger.py (examples/simple-payments/account.rs:37-42, transaction.rs:197-199, ledger.rs:106-112)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_dirty_set_under_asan_ubsan(tmp_path):
    """tests/native/merkle_dirty_check.cpp, a stand-alone program built with -fsanitize=address,undefined: heights 2 .. 8, batches
    of 0 .. 2 n indices in the patterns of the GPU tests and at random with duplicates, an index >= n, the height bounds."""
    exe = str(tmp_path / "merkle_dirty_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "simpleworks_amd", "csrc"), os.path.join(ROOT, "tests", "native", "merkle_dirty_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and ("asan" in out.stderr.lower() or "ubsan" in out.stderr.lower()) and "error:" not in out.stderr:
        pytest.skip("this g++ has no ASan / UBSan runtime")
    assert out.returncode == 0, out.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) >= 4000


def test_account_leaf_is_72_bytes():
    """to_bytes![public_key, balance]: x || y, 32 little-endian bytes each, then the balance as 8: exactly the 576 bits of LeafWindow."""
    from simpleworks_amd import ledger as L
    from simpleworks_amd import hash as H
    x, y = 0x0102030405060708, (1 << 250) + 9
    leaf = L.AccountInformation((x, y), 0x1122334455667788).to_bytes_le()
    assert len(leaf) == 72 == L.LEAF_LEN and 8 * len(leaf) == H.LEAF_WINDOWS * H.WINDOW_SIZE
    assert leaf[:32] == x.to_bytes(32, "little") and leaf[32:64] == y.to_bytes(32, "little")
    assert leaf[64:] == bytes([0x88, 0x77, 0x66, 0x55, 0x44, 0x33, 0x22, 0x11])
    assert L.AccountInformation((x, y)).to_bytes_le()[64:] == bytes(8)


def test_transaction_message_is_10_bytes():
    """sender || recipient || amount: one byte, one byte, eight little-endian bytes — the message the code builds."""
    from simpleworks_amd import ledger as L
    msg = L.transaction_message(1, 2, 5)
    assert msg == bytes([1, 2, 5, 0, 0, 0, 0, 0, 0, 0]) and len(msg) == 10 == L.MESSAGE_LEN
    assert L.transaction_message(255, 0, (1 << 64) - 1) == bytes([255, 0]) + b"\xff" * 8
    tx = L.Transaction(3, 4, 0x0102, None)
    assert tx.message() == bytes([3, 4, 2, 1, 0, 0, 0, 0, 0, 0])
    with pytest.raises(ValueError):
        L.transaction_message(256, 0, 1)
    with pytest.raises(OverflowError):
        L.transaction_message(1, 2, 1 << 64)


def test_height_is_log2_of_the_account_count():
    """ark_std::log2 rounds up; ledger.rs:106-112 uses it as the tree's height, so 32 accounts give height 5 (16 leaves)."""
    from simpleworks_amd import ledger as L
    assert L.ark_log2(32) == 5 and L.ark_log2(33) == 6 and L.ark_log2(31) == 5
    assert [L.ark_log2(v) for v in (0, 1, 2, 3, 4, 5, 8, 9, 256)] == [0, 0, 1, 2, 2, 3, 3, 4, 8]
    with pytest.raises(ValueError):    # height 1: MerkleTree::blank has no such tree; refused before any GPU work
        L.State(2, None)

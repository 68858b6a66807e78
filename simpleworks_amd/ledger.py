"""The ledger of examples/simple-payments: accounts in a Pedersen Merkle tree that stays on the GPU, Schnorr-signed transfers,
and the four checks of Transaction::validate.

Caller-facing mirror of examples/simple-payments/{account,ledger,transaction}.rs, name for name:
    account.rs:12-19      AccountId(u8).to_bytes_le()                      one byte
    account.rs:37-42      AccountInformation.to_bytes_le()                 to_bytes![public_key, balance]: x || y || balance, 72 bytes
    ledger.rs:17-31       Amount(u64): to_bytes_le, checked_add, checked_sub
    ledger.rs:42-51       Parameters::sample(rng)                          Schnorr setup, leaf CRH setup, two-to-one CRH setup, one rng
    ledger.rs:105-121     State::new(num_accounts, &parameters)            MerkleTree::blank(.., log2(num_accounts))
    ledger.rs:131-193     register, sample_keys_and_register, update_balance, apply_transaction
    transaction.rs:148-185  Transaction::validate                          path, signature (+ proof), balance, recipient
    transaction.rs:188-207  Transaction::create                            sign(sender || recipient || amount)
plus validate_many, the batched form a block of transactions wants: one launch each for the signatures, the paths and the path
checks.

The tree is hash.DeviceMerkleTree (csrc/merkle_tree.hip): register and update_balance are tree.update, two launches each
whatever the height; the signature scheme is schnorr.py; the proof of the signature circuit is marlin.generate_schnorr_proof.
Both also exist PROVED (register_proved, update_balance_proved over either tree; a block through apply_updates over a Poseidon
account tree, workloads.build_account_update, and through apply_pedersen_updates over the Pedersen one,
workloads.build_pedersen_account_update), so that the proofs of a ledger chain from State::new's blank root.

Where this departs from the reference, on purpose:
  * The CRH shapes are those of src/merkle_tree/common.rs and hash.py — 144 and 128 windows of 4 bits.  ledger.rs:57-74 declares
    window types of its own with the two numbers the other way round (4 windows of 144 and of 128 bits); the resident table holds
    2^window_size rows per window and cannot take those.  Both hold 576 and 512 bits: a 72-byte leaf fills the leaf CRH exactly.
  * transaction.rs:96-119 runs universal_setup and index for EVERY signature it checks.  The circuit's shape depends on the
    message length alone, so the State derives the keys once, the first time a proof is wanted, and keeps them.
  * A signature that does not verify has no proof (the circuit is unsatisfied), so the prover is not called for it; the
    reference proves anyway and lets verify fail.  The answer, schnorr_verify && marlin_verify, is the same.
"""
import numpy as np

from . import hash as H
from . import schnorr

MESSAGE_LEN = 10     # sender (1) || recipient (1) || amount (8): what transaction.rs:101-103 and :197-199 build
LEAF_LEN = 72        # x || y || balance
U64_MAX = (1 << 64) - 1


def ark_log2(x):
    """ark_std::log2: ceil(log2(x)), 0 for x <= 1."""
    return 0 if x <= 1 else (int(x) - 1).bit_length()


def transaction_message(sender, recipient, amount):
    """The signed bytes.  (The comment at transaction.rs:99-100 lists the public keys too; the code does not add them.)"""
    return bytes([sender, recipient]) + int(amount).to_bytes(8, "little")


class Parameters:
    """ledger::Parameters { sig_params, leaf_crh_params, two_to_one_crh_params }, all three resident on the GPU."""

    def __init__(self, sig_params, leaf_crh, two_to_one_crh, poseidon=None):
        self.sig_params, self.leaf_crh, self.two_to_one_crh = sig_params, leaf_crh, two_to_one_crh
        self.leaf_crh_params, self.two_to_one_crh_params = leaf_crh, two_to_one_crh   # the reference's field names
        self.poseidon = poseidon     # a hash.PoseidonSponge, or None: what a State with account_tree="poseidon" hashes with

    @classmethod
    def sample(cls, rng, ctx=None, poseidon=None):
        """ledger.rs:42-51: the three setups draw from the one rng in this order (the Schnorr setup draws nothing).  poseidon: a
        hash.PoseidonParameters, kept as a resident PoseidonSponge (it draws nothing either)."""
        sig = schnorr.setup(rng, ctx)
        leaf = H.PedersenCRH.setup(rng, H.LEAF_WINDOWS, H.WINDOW_SIZE, ctx)
        inner = H.PedersenCRH.setup(rng, H.TWO_TO_ONE_WINDOWS, H.WINDOW_SIZE, ctx)
        return cls(sig, leaf, inner, H.PoseidonSponge(poseidon, sig.ctx) if poseidon is not None else None)

    def free(self):
        self.sig_params.free()
        self.leaf_crh.free()
        self.two_to_one_crh.free()
        if self.poseidon is not None:
            self.poseidon.free()


class AccountInformation:
    """account.rs:29-42: the public key (an affine point, as ints) and the balance."""

    def __init__(self, public_key, balance=0):
        self.public_key, self.balance = public_key, int(balance)

    def to_bytes_le(self):
        return schnorr.point_bytes(self.public_key) + self.balance.to_bytes(8, "little")


class PaymentCircuit:
    """The payment circuit over resident Schnorr and Poseidon parameters (swm_payment_circuit): synthesises the witness vector of
    workloads.build_payment for batches of payments without running the builder.  A payment is (message, signature, sender leaf,
    recipient leaf); the leaf indices are the message's first two bytes.  Refers to both parameter sets: keep them alive."""

    def __init__(self, sig_params, sponge, height):
        self.ctx, self.sig_params, self.sponge, self.height = sig_params.ctx, sig_params, sponge, height
        self.h = self.ctx.payment_circuit_create(sig_params.h, sponge.h, height)

    def shape(self):
        """(num_instance, num_witness, num_constraints)."""
        from .marlin import payment_circuit_shape
        return payment_circuit_shape(self.sponge.params, self.height, self.sig_params.salt is not None)

    @staticmethod
    def _columns(payments):
        cols = [np.frombuffer(b"".join(bytes(p[k]) for p in payments), dtype=np.uint8).reshape(len(payments), -1) for k in range(4)]
        if [c.shape[1] for c in cols] != [MESSAGE_LEN, 64, LEAF_LEN, LEAF_LEN]:
            raise ValueError("a payment is a %d-byte message, a 64-byte signature and two %d-byte leaves" % (MESSAGE_LEN, LEAF_LEN))
        return cols

    def witness_many(self, payments, sender_siblings, recipient_siblings):
        """No tree: the siblings per path bottom up, as hash.PoseidonMembershipCircuit.witness_many takes them.  Returns (witness
        uint64 [count, num_witness, 4] Montgomery limbs, flags uint8 [count], sender roots, recipient roots as ints)."""
        w, flags, rs, rr = self.ctx.payment_witness(self.h, self.shape()[1], self.height - 1, *self._columns(payments),
                                                    H._fr_rows(sender_siblings), H._fr_rows(recipient_siblings))
        return (w, flags, [int.from_bytes(r.tobytes(), "little") for r in rs], [int.from_bytes(r.tobytes(), "little") for r in rr])

    def witness_at(self, tree, payments):
        """The same against a hash.PoseidonMerkleTree that holds both leaves: (witness, flags)."""
        return self.ctx.payment_witness_at(self.h, tree.h, self.shape()[1], *self._columns(payments))

    def free(self):
        if self.h:
            self.ctx.payment_circuit_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PedersenPaymentCircuit:
    """The payment circuit over resident Schnorr parameters and the two Pedersen CRHs of the reference's account tree
    (swm_pedersen_payment_circuit): synthesises the witness vector of workloads.build_pedersen_payment for batches of payments
    without running the builder.  A payment is (message, signature, sender leaf, recipient leaf); the leaf indices are the message's
    first two bytes.  Refers to the three parameter sets: keep them alive."""

    def __init__(self, sig_params, leaf_crh, two_to_one_crh, height):
        self.ctx, self.sig_params, self.height = sig_params.ctx, sig_params, height
        self.leaf_crh, self.two_to_one_crh = leaf_crh, two_to_one_crh
        self.h = self.ctx.pedersen_payment_circuit_create(sig_params.h, leaf_crh.h, two_to_one_crh.h, height)

    def shape(self):
        """(num_instance, num_witness, num_constraints)."""
        from .marlin import pedersen_payment_circuit_shape
        return pedersen_payment_circuit_shape(self.height, self.sig_params.salt is not None)

    def witness_many(self, payments, sender_siblings, recipient_siblings):
        """No tree: the siblings per path bottom up, as ints.  Returns (witness uint64 [count, num_witness, 4] Montgomery limbs,
        flags uint8 [count], sender roots, recipient roots as ints)."""
        w, flags, rs, rr = self.ctx.pedersen_payment_witness(self.h, self.shape()[1], self.height - 1, *PaymentCircuit._columns(payments),
                                                             H._fr_rows(sender_siblings), H._fr_rows(recipient_siblings))
        return (w, flags, [int.from_bytes(r.tobytes(), "little") for r in rs], [int.from_bytes(r.tobytes(), "little") for r in rr])

    def witness_at(self, tree, payments):
        """The same against a hash.DeviceMerkleTree that holds both leaves: (witness, flags)."""
        return self.ctx.pedersen_payment_witness_at(self.h, tree.h, self.shape()[1], *PaymentCircuit._columns(payments))

    def free(self):
        if self.h:
            self.ctx.pedersen_payment_circuit_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class TransferCircuit:
    """The transfer circuit over resident Schnorr and Poseidon parameters (swm_transfer_circuit): synthesises the witness vector of
    workloads.build_transfer for a block of transfers applied in order, and advances the tree and the account table through the
    block.  A transfer is (message, signature).  Refers to both parameter sets: keep them alive."""

    def __init__(self, sig_params, sponge, height):
        self.ctx, self.sig_params, self.sponge, self.height = sig_params.ctx, sig_params, sponge, height
        self.h = self.ctx.transfer_circuit_create(sig_params.h, sponge.h, height)

    def shape(self):
        """(num_instance, num_witness, num_constraints)."""
        from .marlin import transfer_circuit_shape
        return transfer_circuit_shape(self.sponge.params, self.height, self.sig_params.salt is not None)

    def witness_at(self, tree, accounts, transfers):
        """Against a hash.PoseidonMerkleTree whose leaf level is the table `accounts` (2^L leaves of 72 bytes, all-zero = no
        account): (witness uint64 [count, num_witness, 4], accounts after the block as bytes, old roots, new roots as ints, flags
        uint8 [count], status uint32 [count]).  The tree is advanced."""
        acc = np.frombuffer(b"".join(bytes(a) for a in accounts), dtype=np.uint8).reshape(-1, LEAF_LEN)
        if acc.shape[0] != 1 << (self.height - 1):
            raise ValueError("the account table is 2^(height - 1) leaves of %d bytes" % LEAF_LEN)
        msgs = np.frombuffer(b"".join(bytes(t[0]) for t in transfers), dtype=np.uint8).reshape(len(transfers), -1)
        sigs = np.frombuffer(b"".join(bytes(t[1]) for t in transfers), dtype=np.uint8).reshape(len(transfers), -1)
        if msgs.shape[1] != MESSAGE_LEN or sigs.shape[1] != 64:
            raise ValueError("a transfer is a %d-byte message and a 64-byte signature" % MESSAGE_LEN)
        w, acc, old, new, flags, status = self.ctx.transfer_witness_at(self.h, tree.h, self.shape()[1], acc, msgs, sigs)
        ints = lambda rows: [int.from_bytes(r.tobytes(), "little") for r in rows]
        return w, [a.tobytes() for a in acc], ints(old), ints(new), flags, status

    def free(self):
        if self.h:
            self.ctx.transfer_circuit_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PedersenTransferCircuit:
    """The transfer circuit over resident Schnorr parameters and the two Pedersen CRHs of the reference's account tree
    (swm_pedersen_transfer_circuit): synthesises the witness vector of workloads.build_pedersen_transfer for a block of transfers
    applied in order, and advances the tree and the account table through the block.  A transfer is (message, signature).  Refers to
    the three parameter sets: keep them alive."""

    def __init__(self, sig_params, leaf_crh, two_to_one_crh, height):
        self.ctx, self.sig_params, self.height = sig_params.ctx, sig_params, height
        self.leaf_crh, self.two_to_one_crh = leaf_crh, two_to_one_crh
        self.h = self.ctx.pedersen_transfer_circuit_create(sig_params.h, leaf_crh.h, two_to_one_crh.h, height)

    def shape(self):
        """(num_instance, num_witness, num_constraints)."""
        from .marlin import pedersen_transfer_circuit_shape
        return pedersen_transfer_circuit_shape(self.height, self.sig_params.salt is not None)

    def witness_at(self, tree, accounts, transfers, fill=None):
        """TransferCircuit.witness_at against a hash.DeviceMerkleTree whose leaf level is the table `accounts`: the same results.
        The tree is advanced."""
        acc = np.frombuffer(b"".join(bytes(a) for a in accounts), dtype=np.uint8).reshape(-1, LEAF_LEN)
        if acc.shape[0] != 1 << (self.height - 1):
            raise ValueError("the account table is 2^(height - 1) leaves of %d bytes" % LEAF_LEN)
        msgs = np.frombuffer(b"".join(bytes(t[0]) for t in transfers), dtype=np.uint8).reshape(len(transfers), -1)
        sigs = np.frombuffer(b"".join(bytes(t[1]) for t in transfers), dtype=np.uint8).reshape(len(transfers), -1)
        if msgs.shape[1] != MESSAGE_LEN or sigs.shape[1] != 64:
            raise ValueError("a transfer is a %d-byte message and a 64-byte signature" % MESSAGE_LEN)
        w, acc, old, new, flags, status = self.ctx.pedersen_transfer_witness_at(self.h, tree.h, self.shape()[1], acc, msgs, sigs, fill)
        ints = lambda rows: [int.from_bytes(r.tobytes(), "little") for r in rows]
        return w, [a.tobytes() for a in acc], ints(old), ints(new), flags, status

    def free(self):
        if self.h:
            self.ctx.pedersen_transfer_circuit_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class AccountUpdateCircuit:
    """The account-update circuit over resident Poseidon parameters (swm_account_update_circuit): synthesises the witness vector of
    workloads.build_account_update for a block of registrations and balance updates applied in order, and advances the tree and the
    account table through the block.  An operation is (id, kind, 64 key bytes, balance): kind 0 sets a balance (the key bytes are
    not read), kind 1 registers key || balance.  Refers to the parameter set: keep it alive."""

    def __init__(self, sponge, height):
        self.ctx, self.sponge, self.height = sponge.ctx, sponge, height
        self.h = self.ctx.account_update_circuit_create(sponge.h, height)

    def shape(self):
        """(num_instance, num_witness, num_constraints)."""
        from .marlin import account_update_circuit_shape
        return account_update_circuit_shape(self.sponge.params, self.height)

    def witness_at(self, tree, accounts, ops, guard=0):
        """Against a hash.PoseidonMerkleTree whose leaf level is the table `accounts` (2^L leaves of 72 bytes, all-zero = no
        account): (witness uint64 [count, num_witness, 4] — with guard > 0 the flat [count * num_witness + guard, 4], the guard
        elements 0xFF bytes as before the call —, accounts after the block as bytes, old roots, new roots as ints, flags uint8
        [count] (bit 0: applied), status uint32 [count]).  The tree is advanced; a refused operation's witness is all zero."""
        acc = np.frombuffer(b"".join(bytes(a) for a in accounts), dtype=np.uint8).reshape(-1, LEAF_LEN)
        if acc.shape[0] != 1 << (self.height - 1):
            raise ValueError("the account table is 2^(height - 1) leaves of %d bytes" % LEAF_LEN)
        ops = [(int(i), int(k), bytes(key), int(b)) for i, k, key, b in ops]
        if any(not 0 <= i <= 255 or len(key) != 64 or not 0 <= b <= U64_MAX for i, _, key, b in ops):
            raise ValueError("an operation is (id as one byte, kind, 64 key bytes, balance as u64)")
        n, nw = len(ops), self.shape()[1]
        keys = np.frombuffer(b"".join(o[2] for o in ops), dtype=np.uint8).reshape(n, 64)
        w, acc, old, new, flags, status = getattr(self.ctx, self._witness_entry)(
            self.h, tree.h, nw, acc, np.array([o[0] for o in ops], dtype=np.uint8), np.array([o[1] for o in ops], dtype=np.uint8), keys,
            np.array([o[3] for o in ops], dtype=np.uint64), guard)
        ints = lambda rows: [int.from_bytes(r.tobytes(), "little") for r in rows]
        return (w if guard else w.reshape(n, nw, 4)), [a.tobytes() for a in acc], ints(old), ints(new), flags, status

    _witness_entry = "account_update_witness_at"

    def free(self):
        if self.h:
            self.ctx.account_update_circuit_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PedersenAccountUpdateCircuit(AccountUpdateCircuit):
    """The account-update circuit over the two Pedersen CRHs of the reference's account tree (swm_pedersen_account_update_circuit):
    synthesises the witness vector of workloads.build_pedersen_account_update for a block of registrations and balance updates
    applied in order, and advances the tree (a hash.DeviceMerkleTree with 72-byte leaves) and the account table through the block.
    The operations and the results are AccountUpdateCircuit's.  Refers to the two parameter sets: keep them alive."""

    def __init__(self, leaf_crh, two_to_one_crh, height):
        self.ctx, self.height = leaf_crh.ctx, height
        self.leaf_crh, self.two_to_one_crh = leaf_crh, two_to_one_crh
        self.h = self.ctx.pedersen_account_update_circuit_create(leaf_crh.h, two_to_one_crh.h, height)

    def shape(self):
        """(num_instance, num_witness, num_constraints)."""
        from .marlin import pedersen_account_update_circuit_shape
        return pedersen_account_update_circuit_shape(self.height)

    _witness_entry = "pedersen_account_update_witness_at"

    def free(self):
        if self.h:
            self.ctx.pedersen_account_update_circuit_destroy(self.h)
            self.h = None


class RollupCircuit(TransferCircuit):
    """The rollup of `transfers` transfers over resident Schnorr and Poseidon parameters: ONE vector (workloads.build_rollup's) for a
    block applied in order, all or nothing.  There is no handle of its own: it is a swm_transfer_circuit and a count."""

    def __init__(self, sig_params, sponge, height, transfers):
        super().__init__(sig_params, sponge, height)
        self.transfers = int(transfers)

    def transfer_shape(self):
        return TransferCircuit.shape(self)

    def shape(self):
        """(num_instance, num_witness, num_constraints) of the block."""
        from .marlin import rollup_circuit_shape
        return rollup_circuit_shape(self.sponge.params, self.height, self.transfers, self.sig_params.salt is not None)

    _witness_entry = "rollup_witness_at"

    def witness_at(self, tree, accounts, transfers, guard=0, fill=None):
        """Against a tree whose leaf level is the table `accounts`: (witness uint64 [num_witness + guard, 4], accounts after the block
        as bytes, old root, new root as ints, flags uint8 [count], status uint32 [count], applied).  A block with a refused transfer
        is rolled back: applied False, the tree and the accounts as they were, new root = old root."""
        acc = np.frombuffer(b"".join(bytes(a) for a in accounts), dtype=np.uint8).reshape(-1, LEAF_LEN)
        if acc.shape[0] != 1 << (self.height - 1):
            raise ValueError("the account table is 2^(height - 1) leaves of %d bytes" % LEAF_LEN)
        if len(transfers) != self.transfers:
            raise ValueError("a block of this circuit is %d transfers" % self.transfers)
        msgs = np.frombuffer(b"".join(bytes(t[0]) for t in transfers), dtype=np.uint8).reshape(len(transfers), -1)
        sigs = np.frombuffer(b"".join(bytes(t[1]) for t in transfers), dtype=np.uint8).reshape(len(transfers), -1)
        if msgs.shape[1] != MESSAGE_LEN or sigs.shape[1] != 64:
            raise ValueError("a transfer is a %d-byte message and a 64-byte signature" % MESSAGE_LEN)
        w, acc, old, new, flags, status, applied = getattr(self.ctx, self._witness_entry)(self.h, tree.h, self.shape()[1], acc, msgs, sigs,
                                                                                          guard, fill)
        return (w, [a.tobytes() for a in acc], int.from_bytes(old.tobytes(), "little"), int.from_bytes(new.tobytes(), "little"), flags,
                status, applied)


class PedersenRollupCircuit(PedersenTransferCircuit):
    """RollupCircuit over the reference's Pedersen account tree (workloads.build_pedersen_rollup's vector): a
    swm_pedersen_transfer_circuit and a count."""

    def __init__(self, sig_params, leaf_crh, two_to_one_crh, height, transfers):
        super().__init__(sig_params, leaf_crh, two_to_one_crh, height)
        self.transfers = int(transfers)

    def transfer_shape(self):
        return PedersenTransferCircuit.shape(self)

    def shape(self):
        """(num_instance, num_witness, num_constraints) of the block."""
        from .marlin import pedersen_rollup_circuit_shape
        return pedersen_rollup_circuit_shape(self.height, self.transfers, self.sig_params.salt is not None)

    _witness_entry = "pedersen_rollup_witness_at"
    witness_at = RollupCircuit.witness_at


class State:
    """ledger::State.  The account tree is a hash.DeviceMerkleTree, or with account_tree="poseidon" a hash.PoseidonMerkleTree over
    parameters.poseidon; ids are AccountId(u8), the first one handed out is 1."""

    def __init__(self, num_accounts, parameters, account_tree="pedersen"):
        """ledger.rs:106-112 hands ark_std::log2(num_accounts) to MerkleTree::blank as the HEIGHT, and arkworks' height counts the
        leaf level: 32 accounts give height 5 and 2^4 = 16 leaves.  Mirrored as it stands.  Registering past the last leaf
        raises (the reference panics in tree.update: "should exist")."""
        self.parameters = parameters
        height = ark_log2(num_accounts)
        if height < 2:
            raise ValueError("State: %d accounts give a tree of height %d (MerkleTree::blank needs 2)" % (num_accounts, height))
        if account_tree not in ("pedersen", "poseidon"):
            raise ValueError("State: account_tree is \"pedersen\" or \"poseidon\"")
        self.account_tree = account_tree
        if account_tree == "poseidon":
            if parameters.poseidon is None:
                raise ValueError("State: a Poseidon account tree needs Parameters.sample(.., poseidon=...)")
            if height > 9:
                raise ValueError("State: a Poseidon account tree has at most 256 leaves (an account id is one byte)")
            self.account_merkle_tree = H.PoseidonMerkleTree.blank(parameters.poseidon, height, LEAF_LEN)
        else:
            self.account_merkle_tree = H.DeviceMerkleTree.blank(parameters.leaf_crh, parameters.two_to_one_crh, height, LEAF_LEN)
        self.next_available_account = 1
        self.id_to_account_info = {}
        self.pub_key_to_id = {}
        self._proof_keys = None      # (SchnorrCircuit, proving key, verifying key), derived once
        self._payment_keys = None    # (PaymentCircuit, proving key, verifying key), the same for a Poseidon account tree
        self._transfer_keys = None   # (TransferCircuit, proving key, verifying key), the same
        self._pedersen_payment_keys = None   # (PedersenPaymentCircuit, proving key, verifying key), for a Pedersen account tree
        self._pedersen_transfer_keys = None  # (PedersenTransferCircuit, proving key, verifying key), the same
        self._update_keys = None     # (AccountUpdateCircuit, proving key, verifying key), for a Poseidon account tree
        self._update_circuit = None  # the circuit alone (no keys are needed to apply a block unproved)
        self._pedersen_update_keys = None     # (PedersenAccountUpdateCircuit, proving key, verifying key), for a Pedersen account tree
        self._pedersen_update_circuit = None  # the circuit alone
        self._rollup_keys = {}       # transfers per block -> (RollupCircuit or PedersenRollupCircuit, proving key, verifying key)
        self._rollup_circuits = {}   # transfers per block -> the circuit alone (no keys are needed to apply a block unproved)
        self._rollup_transfer_system = None  # the ONE packed transfer system every block size is relabelled from

    def root(self):
        return self.account_merkle_tree.root()

    def register(self, public_key):
        """-> the new account's id, or None when the u8 ids have run out.  The initial balance is 0."""
        acc = self.next_available_account
        if acc is None:
            return None
        if acc >= 1 << (self.account_merkle_tree.height() - 1):
            raise IndexError("register: account %d is past the last leaf of the account tree" % acc)
        info = AccountInformation(public_key, 0)
        self.pub_key_to_id[public_key] = acc
        self.account_merkle_tree.update(acc, info.to_bytes_le())
        self.id_to_account_info[acc] = info
        self.next_available_account = acc + 1 if acc < 255 else None     # checked_increment
        return acc

    def sample_keys_and_register(self, ledger_params, rng):
        """-> (id, public key, secret key), or None."""
        pub_key, secret_key = schnorr.keygen(ledger_params.sig_params, rng)
        acc = self.register(pub_key)
        return None if acc is None else (acc, pub_key, secret_key)

    def update_balance(self, acc, new_amount):
        """-> True, or None when there is no such account."""
        info = self.id_to_account_info.get(acc)
        if info is None:
            return None
        info.balance = int(new_amount)
        self.account_merkle_tree.update(acc, info.to_bytes_le())
        return True

    def apply_transaction(self, pp, tx, rng, prove=True):
        """-> True when tx is valid and has been applied, else None (ledger.rs:176-193): two tree.update, four launches."""
        try:
            if not tx.validate(pp, self, rng, prove):
                return None
        except KeyError:
            return None
        sender, recipient = self.id_to_account_info.get(tx.sender), self.id_to_account_info.get(tx.recipient)
        if sender is None or recipient is None:
            return None
        if tx.amount > sender.balance or recipient.balance + tx.amount > U64_MAX:     # checked_sub, checked_add
            return None
        new_sender, new_recipient = sender.balance - tx.amount, recipient.balance + tx.amount
        self.update_balance(tx.sender, new_sender)
        self.update_balance(tx.recipient, new_recipient)
        return True

    def proof_keys(self, rng):
        """The signature circuit (10-byte messages, this ledger's salt) with its Marlin keys: a universal setup sized for the
        circuit and one index, the first time they are asked for."""
        if self._proof_keys is None:
            from . import marlin as M
            from . import workloads as W
            sig = self.parameters.sig_params
            cs, _ = W.schnorr_verification_circuit(sig.generator, sig.salt, None, bytes(MESSAGE_LEN), bytes(64))
            packed = cs.pack()
            nnz = max(int(m[0][-1]) for m in packed.mats)
            srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, rng, sig.ctx)
            try:
                pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
            finally:
                srs.free()
            self._proof_keys = (schnorr.SchnorrCircuit(sig, MESSAGE_LEN), pk, vk)
        return self._proof_keys

    def payment_keys(self, rng):
        """The payment circuit (this ledger's parameters and tree height) with its Marlin keys, derived once as proof_keys derives
        the signature circuit's.  The matrices depend on the shape alone: any payment's system indexes them."""
        if self.account_tree != "poseidon":
            raise ValueError("payment_keys: the payment circuit is over a Poseidon account tree")
        if self._payment_keys is None:
            from . import marlin as M
            from . import workloads as W
            sig, sponge = self.parameters.sig_params, self.parameters.poseidon
            height = self.account_merkle_tree.height()
            leaf = AccountInformation(sig.generator, 0).to_bytes_le()
            cs, _ = W.payment_circuit(sponge.params, height, bytes(MESSAGE_LEN), bytes(64), leaf, [0] * (height - 1), leaf,
                                      [0] * (height - 1), sig.generator, sig.salt)
            packed = cs.pack()
            nnz = max(int(m[0][-1]) for m in packed.mats)
            srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, rng, sig.ctx)
            try:
                pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
            finally:
                srs.free()
            self._payment_keys = (PaymentCircuit(sig, sponge, height), pk, vk)
        return self._payment_keys

    def pedersen_payment_keys(self, rng):
        """The payment circuit over this ledger's Pedersen account tree (its parameters and tree height) with its Marlin keys,
        derived once as payment_keys derives the Poseidon form's."""
        if self.account_tree != "pedersen":
            raise ValueError("pedersen_payment_keys: the Pedersen payment circuit is over a Pedersen account tree")
        if self._pedersen_payment_keys is None:
            from . import marlin as M
            from . import workloads as W
            sig, leaf_crh, inner_crh = self.parameters.sig_params, self.parameters.leaf_crh, self.parameters.two_to_one_crh
            height = self.account_merkle_tree.height()
            params = W.MerkleParams(generators=(leaf_crh.generators, inner_crh.generators))
            leaf = AccountInformation(sig.generator, 0).to_bytes_le()
            cs, _ = W.pedersen_payment_circuit(params, height, bytes(MESSAGE_LEN), bytes(64), leaf, [0] * (height - 1), leaf,
                                               [0] * (height - 1), sig.generator, sig.salt, root=0)
            packed = cs.pack()
            nnz = max(int(m[0][-1]) for m in packed.mats)
            srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, rng, sig.ctx)
            try:
                pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
            finally:
                srs.free()
            self._pedersen_payment_keys = (PedersenPaymentCircuit(sig, leaf_crh, inner_crh, height), pk, vk)
        return self._pedersen_payment_keys

    def transfer_keys(self, rng):
        """The transfer circuit (this ledger's parameters and tree height) with its Marlin keys, derived once as payment_keys
        derives the payment circuit's."""
        if self.account_tree != "poseidon":
            raise ValueError("transfer_keys: the transfer circuit is over a Poseidon account tree")
        if self._transfer_keys is None:
            from . import marlin as M
            from . import workloads as W
            sig, sponge = self.parameters.sig_params, self.parameters.poseidon
            height = self.account_merkle_tree.height()
            leaf = AccountInformation(sig.generator, 0).to_bytes_le()
            cs, _ = W.transfer_circuit(sponge.params, height, bytes(MESSAGE_LEN), bytes(64), leaf, [0] * (height - 1), leaf,
                                       [0] * (height - 1), sig.generator, sig.salt)
            packed = cs.pack()
            nnz = max(int(m[0][-1]) for m in packed.mats)
            srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, rng, sig.ctx)
            try:
                pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
            finally:
                srs.free()
            self._transfer_keys = (TransferCircuit(sig, sponge, height), pk, vk)
        return self._transfer_keys

    def pedersen_transfer_keys(self, rng):
        """The transfer circuit over this ledger's Pedersen account tree (its parameters and tree height) with its Marlin keys,
        derived once as pedersen_payment_keys derives the payment circuit's."""
        if self.account_tree != "pedersen":
            raise ValueError("pedersen_transfer_keys: the Pedersen transfer circuit is over a Pedersen account tree")
        if self._pedersen_transfer_keys is None:
            from . import marlin as M
            from . import workloads as W
            sig, leaf_crh, inner_crh = self.parameters.sig_params, self.parameters.leaf_crh, self.parameters.two_to_one_crh
            height = self.account_merkle_tree.height()
            params = W.MerkleParams(generators=(leaf_crh.generators, inner_crh.generators))
            leaf = AccountInformation(sig.generator, 0).to_bytes_le()
            cs, _ = W.pedersen_transfer_circuit(params, height, bytes(MESSAGE_LEN), bytes(64), leaf, [0] * (height - 1), leaf,
                                                [0] * (height - 1), sig.generator, sig.salt, old_root=0, new_root=0, r1=0)
            packed = cs.pack()
            nnz = max(int(m[0][-1]) for m in packed.mats)
            srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, rng, sig.ctx)
            try:
                pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
            finally:
                srs.free()
            self._pedersen_transfer_keys = (PedersenTransferCircuit(sig, leaf_crh, inner_crh, height), pk, vk)
        return self._pedersen_transfer_keys

    def update_keys(self, rng):
        """The account-update circuit (this ledger's Poseidon parameters and tree height) with its Marlin keys, derived once as
        transfer_keys derives the transfer circuit's: one key serves registrations and balance updates."""
        if self.account_tree != "poseidon":
            raise ValueError("update_keys: the account-update circuit is over a Poseidon account tree")
        if self._update_keys is None:
            from . import marlin as M
            from . import workloads as W
            sponge = self.parameters.poseidon
            height = self.account_merkle_tree.height()
            cs, _ = W.account_update_circuit(sponge.params, height, 0, self.parameters.sig_params.generator, 0, 0, 1, [0] * (height - 1))
            packed = cs.pack()
            nnz = max(int(m[0][-1]) for m in packed.mats)
            srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, rng, sponge.ctx)
            try:
                pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
            finally:
                srs.free()
            self._update_keys = (AccountUpdateCircuit(sponge, height), pk, vk)
        return self._update_keys

    def pedersen_update_keys(self, rng):
        """The account-update circuit over this ledger's Pedersen account tree (its two CRHs and tree height) with its Marlin keys,
        derived once as update_keys derives the Poseidon form's: one key serves registrations and balance updates."""
        if self.account_tree != "pedersen":
            raise ValueError("pedersen_update_keys: the Pedersen account-update circuit is over a Pedersen account tree")
        if self._pedersen_update_keys is None:
            from . import marlin as M
            from . import workloads as W
            leaf_crh, inner_crh = self.parameters.leaf_crh, self.parameters.two_to_one_crh
            height = self.account_merkle_tree.height()
            params = W.MerkleParams(generators=(leaf_crh.generators, inner_crh.generators))
            cs, _ = W.pedersen_account_update_circuit(params, height, 0, self.parameters.sig_params.generator, 0, 0, 1, [0] * (height - 1),
                                                      old_root=0, new_root=0)
            packed = cs.pack()
            nnz = max(int(m[0][-1]) for m in packed.mats)
            srs = M.MarlinInst.universal_setup(cs.num_constraints, len(cs.instance) + len(cs.witness), nnz, rng, leaf_crh.ctx)
            try:
                pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
            finally:
                srs.free()
            self._pedersen_update_keys = (PedersenAccountUpdateCircuit(leaf_crh, inner_crh, height), pk, vk)
        return self._pedersen_update_keys

    def apply_updates(self, pp, ops, rng, prove=True):
        """A block of registrations and balance updates applied in order, each one proved: one witness pass on the GPU advances the
        account tree through the whole block, then (with prove) one proof per applied operation under update_keys(rng), whose public
        inputs are workloads.account_update_public_inputs (old_root, new_root, id, key_x, key_y, old_balance, new_balance, fresh).
        An operation is ("register", id, public key) — the initial balance is 0, as State::register's — or ("balance", id, amount).
        A Poseidon state only.  -> a list of (applied, proof or None, public inputs), one per operation; a refused operation (an
        occupied or out-of-range id, an account that does not exist, a key that is not canonical) leaves the state as it was and
        publishes equal roots.  next_available_account, pub_key_to_id and id_to_account_info follow the applied operations."""
        if self.account_tree != "poseidon":
            raise ValueError("apply_updates: the account-update circuit is over a Poseidon account tree")
        return self._apply_update_block(ops, rng, prove, False)

    def apply_pedersen_updates(self, pp, ops, rng, prove=True):
        """apply_updates over this ledger's Pedersen account tree (workloads.build_pedersen_account_update): the same operations and
        the same results, the proofs under pedersen_update_keys(rng); verify_update with pedersen_update_keys(rng)[2] serves.  A
        Pedersen state only."""
        if self.account_tree != "pedersen":
            raise ValueError("apply_pedersen_updates: the Pedersen account-update circuit is over a Pedersen account tree")
        return self._apply_update_block(ops, rng, prove, True)

    def _apply_update_block(self, ops, rng, prove, pedersen):
        from . import marlin as M
        ops = list(ops)
        if not ops:
            return []
        block = []
        for what, acc, value in ops:
            if what == "register":
                block.append((int(acc), 1, schnorr.point_bytes(value), 0))
            elif what == "balance":
                block.append((int(acc), 0, bytes(64), int(value)))
            else:
                raise ValueError("apply_updates: an operation is (\"register\", id, public key) or (\"balance\", id, amount)")
        tree = self.account_merkle_tree
        table = self.account_table()
        if prove:
            circuit, pk, _ = self.pedersen_update_keys(rng) if pedersen else self.update_keys(rng)
            prover = M.generate_pedersen_account_update_proofs if pedersen else M.generate_account_update_proofs
            proofs, public, flags, _, _ = prover(pk, circuit, tree, table, block, rng)
        else:
            if pedersen:
                if self._pedersen_update_keys is not None:
                    circuit = self._pedersen_update_keys[0]
                else:
                    if self._pedersen_update_circuit is None:
                        self._pedersen_update_circuit = PedersenAccountUpdateCircuit(self.parameters.leaf_crh, self.parameters.two_to_one_crh,
                                                                                     tree.height())
                    circuit = self._pedersen_update_circuit
            elif self._update_keys is not None:
                circuit = self._update_keys[0]
            else:
                if self._update_circuit is None:
                    self._update_circuit = AccountUpdateCircuit(self.parameters.poseidon, tree.height())
                circuit = self._update_circuit
            _, _, old, new, flags, _ = circuit.witness_at(tree, table, block)
            proofs, public = [None] * len(ops), []
            for op, o, n, f in zip(block, old, new, flags):
                public.append(M._account_update_public(table, op, o, n))
                if f & 1:
                    table[op[0]] = (op[2] if op[1] else table[op[0]][:64]) + op[3].to_bytes(8, "little")
        for (what, acc, value), f in zip(ops, flags):
            if not f & 1:
                continue
            if what == "register":
                self.pub_key_to_id[value] = acc
                self.id_to_account_info[acc] = AccountInformation(value, 0)
                if self.next_available_account is not None and acc >= self.next_available_account:
                    self.next_available_account = acc + 1 if acc < 255 else None     # checked_increment
            else:
                self.id_to_account_info[acc].balance = int(value)
        return [(bool(f & 1), proof, pub) for f, proof, pub in zip(flags, proofs, public)]

    def register_proved(self, public_key, rng):
        """register with its proof: -> (the new account's id, proof bytes, public inputs), or None when the u8 ids have run out.
        IndexError past the last leaf, as register."""
        acc = self.next_available_account
        if acc is None:
            return None
        if acc >= 1 << (self.account_merkle_tree.height() - 1):
            raise IndexError("register: account %d is past the last leaf of the account tree" % acc)
        applied, proof, public = self._apply_update_block([("register", acc, public_key)], rng, True, self.account_tree == "pedersen")[0]
        if not applied:
            raise ValueError("register_proved: the registration of account %d was refused" % acc)
        return acc, proof, public

    def update_balance_proved(self, acc, new_amount, rng):
        """update_balance with its proof: -> (proof bytes, public inputs), or None when there is no such account."""
        if acc not in self.id_to_account_info:
            return None
        applied, proof, public = self._apply_update_block([("balance", acc, new_amount)], rng, True, self.account_tree == "pedersen")[0]
        if not applied:
            raise ValueError("update_balance_proved: the update of account %d was refused" % acc)
        return proof, public

    def account_table(self):
        """All 2^L leaves of the account tree as the state holds them, 72 bytes each; all-zero where there is no account."""
        blank = bytes(LEAF_LEN)
        return [self.id_to_account_info[i].to_bytes_le() if i in self.id_to_account_info else blank
                for i in range(1 << (self.account_merkle_tree.height() - 1))]

    def apply_transactions(self, pp, txs, rng, prove=True):
        """A block of transactions applied in order, the state transition of each proved: one witness pass on the GPU advances the
        account tree through the whole block, then (with prove) one proof per applied transaction, whose public inputs are
        (old_root, new_root, sender, recipient, amount).  A Poseidon state only (a Pedersen state: apply_pedersen_transactions).
        -> a list of (applied, proof or None, public inputs), one per transaction; a refused transaction leaves the state as it
        was and publishes equal roots.  Unlike apply_transaction, a payment to oneself is refused (the circuit reads it as a no-op,
        apply_transaction adds the amount)."""
        if self.account_tree != "poseidon":
            raise ValueError("apply_transactions: the transfer circuit is over a Poseidon account tree")
        return self._apply_block(txs, rng, prove)

    def apply_pedersen_transactions(self, pp, txs, rng, prove=True):
        """apply_transactions over the default Pedersen account tree, through the Pedersen transfer circuit
        (workloads.build_pedersen_transfer): the same results; verify_transfer with pedersen_transfer_keys(rng)[2] serves.  A
        Pedersen state only.  Besides a payment to oneself, a payment to an id without an account is refused."""
        if self.account_tree != "pedersen":
            raise ValueError("apply_pedersen_transactions: the Pedersen transfer circuit is over a Pedersen account tree")
        return self._apply_block(txs, rng, prove)

    def _apply_block(self, txs, rng, prove):
        from . import marlin as M
        from . import workloads as W
        txs = list(txs)
        if not txs:
            return []
        pedersen = self.account_tree == "pedersen"
        circuit, pk, _ = self.pedersen_transfer_keys(rng) if pedersen else self.transfer_keys(rng)
        block = [(tx.message(), tx.signature.to_bytes()) for tx in txs]
        tree = self.account_merkle_tree
        if prove:
            prover = M.generate_pedersen_transfer_proofs if pedersen else M.generate_transfer_proofs
            proofs, public, flags, _, table = prover(pk, circuit, tree, self.account_table(), block, rng)
        else:
            _, table, old, new, flags, _ = circuit.witness_at(tree, self.account_table(), block)
            proofs = [None] * len(txs)
            public = [W.transfer_public_inputs(o, n, m) for o, n, (m, _) in zip(old, new, block)]
        for i, info in self.id_to_account_info.items():
            info.balance = int.from_bytes(table[i][64:], "little")
        return [(bool(f & 16), proof, pub) for f, proof, pub in zip(flags, proofs, public)]

    def _rollup_circuit(self, n):
        n = int(n)
        if n not in self._rollup_circuits:
            sig, height = self.parameters.sig_params, self.account_merkle_tree.height()
            if self.account_tree == "pedersen":
                self._rollup_circuits[n] = PedersenRollupCircuit(sig, self.parameters.leaf_crh, self.parameters.two_to_one_crh, height, n)
            else:
                self._rollup_circuits[n] = RollupCircuit(sig, self.parameters.poseidon, height, n)
        return self._rollup_circuits[n]

    def _rollup_keys_for(self, n, rng):
        from . import marlin as M
        from . import workloads as W
        n = int(n)
        if not 1 <= n <= W.ROLLUP_MAX_TRANSFERS:
            raise ValueError("rollup_keys: 1 <= transfers <= %d" % W.ROLLUP_MAX_TRANSFERS)
        if n not in self._rollup_keys:
            sig = self.parameters.sig_params
            height = self.account_merkle_tree.height()
            if self._rollup_transfer_system is None:
                leaf = AccountInformation(sig.generator, 0).to_bytes_le()
                if self.account_tree == "pedersen":
                    params = W.MerkleParams(generators=(self.parameters.leaf_crh.generators, self.parameters.two_to_one_crh.generators))
                    cs, _ = W.pedersen_transfer_circuit(params, height, bytes(MESSAGE_LEN), bytes(64), leaf, [0] * (height - 1), leaf,
                                                        [0] * (height - 1), sig.generator, sig.salt, old_root=0, new_root=0, r1=0)
                else:
                    cs, _ = W.transfer_circuit(self.parameters.poseidon.params, height, bytes(MESSAGE_LEN), bytes(64), leaf,
                                               [0] * (height - 1), leaf, [0] * (height - 1), sig.generator, sig.salt)
                self._rollup_transfer_system = cs.pack()
            packed = W.rollup_system(self._rollup_transfer_system, n)     # no builder per section
            nnz = max(int(m[0][-1]) for m in packed.mats)
            srs = M.MarlinInst.universal_setup(packed.num_constraints, packed.instance.shape[0] + packed.witness.shape[0], nnz, rng, sig.ctx)
            try:
                pk, vk = M.MarlinInst.index_from_constraint_system(srs, packed)
            finally:
                srs.free()
            self._rollup_keys[n] = (self._rollup_circuit(n), pk, vk)
        return self._rollup_keys[n]

    def rollup_keys(self, n, rng):
        """The rollup of n transfers over this ledger's Poseidon account tree with its Marlin keys, derived once per n: ONE transfer
        system is built and relabelled n times (workloads.rollup_system), so the keys of a block cost the builder one transfer."""
        if self.account_tree != "poseidon":
            raise ValueError("rollup_keys: the rollup circuit is over a Poseidon account tree (a Pedersen state: pedersen_rollup_keys)")
        return self._rollup_keys_for(n, rng)

    def pedersen_rollup_keys(self, n, rng):
        """rollup_keys over this ledger's Pedersen account tree."""
        if self.account_tree != "pedersen":
            raise ValueError("pedersen_rollup_keys: the Pedersen rollup circuit is over a Pedersen account tree")
        return self._rollup_keys_for(n, rng)

    def apply_rollup(self, pp, txs, rng, prove=True):
        """A block of transactions applied in order, ALL OR NOTHING, and (with prove) ONE proof that the root before the block
        becomes the root after it, under rollup_keys(len(txs), rng) / pedersen_rollup_keys: the block has exactly as many transfers
        as the key.  -> (applied, proof or None, public inputs): workloads.rollup_public_inputs(old_root, new_root, messages).  A
        block with a refused transaction is rolled back: applied False, no proof, the state as it was, equal roots.  As under
        apply_transactions a payment to oneself is refused."""
        from . import marlin as M
        from . import workloads as W
        txs = list(txs)
        if not txs:
            raise ValueError("apply_rollup: an empty block")
        pedersen = self.account_tree == "pedersen"
        block = [(tx.message(), tx.signature.to_bytes()) for tx in txs]
        tree = self.account_merkle_tree
        if prove:
            circuit, pk, _ = self._rollup_keys_for(len(txs), rng)
            prover = M.generate_pedersen_rollup_proof if pedersen else M.generate_rollup_proof
            proof, public, _, _, table, applied = prover(pk, circuit, tree, self.account_table(), block, rng)
        else:
            _, table, old, new, _, _, applied = self._rollup_circuit(len(txs)).witness_at(tree, self.account_table(), block)
            proof, public = None, W.rollup_public_inputs(old, new, [m for m, _ in block])
        if applied:
            for i, info in self.id_to_account_info.items():
                info.balance = int.from_bytes(table[i][64:], "little")
        return applied, proof, public

    def free(self):
        for keys in (self._proof_keys, self._payment_keys, self._transfer_keys, self._pedersen_payment_keys, self._pedersen_transfer_keys,
                     self._update_keys, self._pedersen_update_keys):
            if keys is not None:
                keys[0].free()
                keys[1].free()
        self._proof_keys = self._payment_keys = self._transfer_keys = self._pedersen_payment_keys = self._pedersen_transfer_keys = None
        self._update_keys = self._pedersen_update_keys = None
        for name in ("_update_circuit", "_pedersen_update_circuit"):
            if getattr(self, name) is not None:
                getattr(self, name).free()
                setattr(self, name, None)
        for _, pk, _ in self._rollup_keys.values():
            pk.free()
        for circuit in self._rollup_circuits.values():
            circuit.free()
        self._rollup_keys, self._rollup_circuits, self._rollup_transfer_system = {}, {}, None
        self.account_merkle_tree.free()


def _prove_signature(state, public_key, message, signature, rng):
    """transaction.rs:108-126 with the State's keys: the proof of the signature circuit, then its verification."""
    from . import marlin as M
    circuit, pk, vk = state.proof_keys(rng)
    proof = M.generate_schnorr_proof(pk, circuit, public_key, message, signature.to_bytes(), rng)
    return M.verify_proof(vk, [], M.MarlinProof(proof), rng)


def verify_payment(vk, public_inputs, proof, rng):
    """The verifier of a payment proof: public_inputs = [root, sender, recipient, amount] (workloads.payment_public_inputs)."""
    from . import marlin as M
    return M.verify_proof(vk, [int(v) for v in public_inputs], proof if isinstance(proof, M.MarlinProof) else M.MarlinProof(proof), rng)


def verify_transfer(vk, public_inputs, proof, rng):
    """The verifier of a transfer proof over either account tree: public_inputs = [old_root, new_root, sender, recipient, amount]
    (workloads.transfer_public_inputs = pedersen_transfer_public_inputs)."""
    from . import marlin as M
    return M.verify_proof(vk, [int(v) for v in public_inputs], proof if isinstance(proof, M.MarlinProof) else M.MarlinProof(proof), rng)


def verify_update(vk, public_inputs, proof, rng):
    """The verifier of an account-update proof: public_inputs = [old_root, new_root, id, key_x, key_y, old_balance, new_balance, fresh]
    (workloads.account_update_public_inputs), vk that of State.update_keys or, over a Pedersen account tree, State.pedersen_update_keys."""
    from . import marlin as M
    return M.verify_proof(vk, [int(v) for v in public_inputs], proof if isinstance(proof, M.MarlinProof) else M.MarlinProof(proof), rng)


def verify_rollup(vk, public_inputs, proof, rng):
    """The verifier of a rollup proof over either account tree: public_inputs = [old_root, new_root, sender_0, recipient_0, amount_0,
    ...] (workloads.rollup_public_inputs), vk that of a block of as many transfers."""
    from . import marlin as M
    return M.verify_proof(vk, [int(v) for v in public_inputs], proof if isinstance(proof, M.MarlinProof) else M.MarlinProof(proof), rng)


def _payment_leaves(state, tx):
    """(sender leaf, recipient leaf) as the state holds them, or None when the recipient has no account."""
    recipient = state.id_to_account_info.get(tx.recipient)
    if recipient is None:
        return None
    return state.id_to_account_info[tx.sender].to_bytes_le(), recipient.to_bytes_le()


class Transaction:
    """transaction.rs:74-85: sender, recipient, amount and the sender's signature over the three."""

    def __init__(self, sender, recipient, amount, signature):
        self.sender, self.recipient, self.amount, self.signature = int(sender), int(recipient), int(amount), signature

    def message(self):
        return transaction_message(self.sender, self.recipient, self.amount)

    @staticmethod
    def create(parameters, sender, recipient, amount, sender_sk, rng):
        """A (possibly invalid) transaction: whoever holds sender_sk signs."""
        sig = schnorr.sign(parameters.sig_params, sender_sk, transaction_message(sender, recipient, amount), rng)
        return Transaction(sender, recipient, amount, sig)

    def prove_payment(self, parameters, state, rng):
        """-> (proof bytes, public inputs) of the payment circuit against a state with a Poseidon account tree, as it stands now.
        KeyError when sender or recipient has no account; MarlinError (SWM_ERR_UNSATISFIED) when the payment is not valid."""
        from . import marlin as M
        from . import workloads as W
        if self.sender not in state.id_to_account_info or self.recipient not in state.id_to_account_info:
            raise KeyError("sender or recipient not found")
        circuit, pk, _ = state.payment_keys(rng)
        tree = state.account_merkle_tree
        sender_leaf, recipient_leaf = _payment_leaves(state, self)
        public = W.payment_public_inputs(tree.root(), self.message())
        proof = M.generate_payment_proof(pk, circuit, tree, self.message(), self.signature.to_bytes(), sender_leaf, recipient_leaf, rng)
        return proof, public

    def prove_pedersen_payment(self, parameters, state, rng):
        """-> (proof bytes, public inputs) of the payment circuit against a state with a Pedersen account tree (the default one), as
        it stands now.  KeyError when sender or recipient has no account; MarlinError (SWM_ERR_UNSATISFIED) when the payment is not
        valid.  verify_payment serves: the public input order is the Poseidon form's."""
        from . import marlin as M
        from . import workloads as W
        if self.sender not in state.id_to_account_info or self.recipient not in state.id_to_account_info:
            raise KeyError("sender or recipient not found")
        circuit, pk, _ = state.pedersen_payment_keys(rng)
        tree = state.account_merkle_tree
        sender_leaf, recipient_leaf = _payment_leaves(state, self)
        public = W.pedersen_payment_public_inputs(tree.root(), self.message())
        proof = M.generate_pedersen_payment_proof(pk, circuit, tree, self.message(), self.signature.to_bytes(), sender_leaf, recipient_leaf,
                                                  rng)
        return proof, public

    def validate(self, parameters, state, rng, prove=True):
        """transaction.rs:148-185.  KeyError when the sender has no account (the reference's Err).  Otherwise the conjunction of
          1. the sender's leaf is in the account tree: generate_proofs, then verify_paths against the root;
          2. the signature verifies under the sender's key — and, with prove, the Marlin proof of the signature circuit is made
             and accepted;
          3. the amount is within the sender's balance;
          4. the recipient has an account."""
        info = state.id_to_account_info.get(self.sender)
        if info is None:
            raise KeyError("sender not found")
        tree = state.account_merkle_tree
        path = tree.generate_proofs([self.sender])
        poseidon = state.account_tree == "poseidon"
        if poseidon:
            result = bool(H.verify_poseidon_paths(parameters.poseidon, tree.height(), tree.root(), [info.to_bytes_le()], [self.sender],
                                                  path)[0])
        else:
            result = bool(H.verify_paths(parameters.leaf_crh, parameters.two_to_one_crh, tree.height(), tree.root(), [info.to_bytes_le()],
                                         [self.sender], path)[0])
        sig_ok = schnorr.verify(parameters.sig_params, info.public_key, self.message(), self.signature)
        if poseidon and prove:
            # the one proof states all four checks: made only for a payment that passes them (an invalid one has no proof)
            if result and sig_ok and self.amount <= info.balance and self.recipient in state.id_to_account_info:
                proof, public = self.prove_payment(parameters, state, rng)
                sig_ok = verify_payment(state.payment_keys(rng)[2], public, proof, rng)
        elif sig_ok and prove:
            sig_ok = _prove_signature(state, info.public_key, self.message(), self.signature, rng)
        result &= sig_ok
        result &= self.amount <= info.balance
        result &= self.recipient in state.id_to_account_info
        return result


def validate_many(parameters, state, txs, rng=None, prove=False):
    """Transaction.validate for a block of transactions against ONE state (none of them applied): a list of booleans.  One launch
    each for schnorr.verify_many, generate_proofs and verify_paths over the whole block; with prove, one proof per verifying
    signature after that.  A transaction whose sender has no account is False here."""
    known = [i for i, tx in enumerate(txs) if tx.sender in state.id_to_account_info]
    out = [False] * len(txs)
    if not known:
        return out
    infos = [state.id_to_account_info[txs[i].sender] for i in known]
    senders = [txs[i].sender for i in known]
    tree = state.account_merkle_tree
    paths = tree.generate_proofs(senders)
    poseidon = state.account_tree == "poseidon"
    if poseidon:
        in_tree = H.verify_poseidon_paths(parameters.poseidon, tree.height(), tree.root(), [info.to_bytes_le() for info in infos], senders,
                                          paths)
    else:
        in_tree = H.verify_paths(parameters.leaf_crh, parameters.two_to_one_crh, tree.height(), tree.root(),
                                 [info.to_bytes_le() for info in infos], senders, paths)
    keys = np.frombuffer(b"".join(schnorr.point_bytes(info.public_key) for info in infos), dtype=np.uint8).reshape(-1, 64)
    msgs = np.frombuffer(b"".join(txs[i].message() for i in known), dtype=np.uint8).reshape(-1, MESSAGE_LEN)
    sigs = np.frombuffer(b"".join(txs[i].signature.to_bytes() for i in known), dtype=np.uint8).reshape(-1, 64)
    signed = schnorr.verify_many(parameters.sig_params, keys, msgs, sigs)
    proved = {}
    if poseidon and prove:
        # one witness pass and one prover call per payment that passes the native checks
        from . import marlin as M
        from . import workloads as W
        circuit, pk, vk = state.payment_keys(rng)
        good = [k for k, i in enumerate(known) if in_tree[k] and signed[k] and txs[i].amount <= infos[k].balance
                and txs[i].recipient in state.id_to_account_info]
        block = [(txs[known[k]].message(), txs[known[k]].signature.to_bytes()) + _payment_leaves(state, txs[known[k]]) for k in good]
        proofs, _ = M.generate_payment_proofs(pk, circuit, tree, block, rng)
        root = tree.root()
        for k, proof in zip(good, proofs):
            proved[k] = proof is not None and verify_payment(vk, W.payment_public_inputs(root, txs[known[k]].message()), proof, rng)
    for k, i in enumerate(known):
        tx, sig_ok = txs[i], bool(signed[k])
        if poseidon and prove:
            sig_ok = sig_ok and proved.get(k, False)
        elif sig_ok and prove:
            sig_ok = _prove_signature(state, infos[k].public_key, tx.message(), tx.signature, rng)
        out[i] = bool(in_tree[k]) and sig_ok and tx.amount <= infos[k].balance and tx.recipient in state.id_to_account_info
    return out


def prove_pedersen_payments(parameters, state, txs, rng):
    """The block form of Transaction.prove_pedersen_payment against ONE state with a Pedersen account tree (none of the transactions
    applied): one witness pass for the block, then one prover call per payment that is valid.  -> a list with (proof bytes, public
    inputs) per transaction, None where it has no proof: sender or recipient without an account, a signature that does not verify,
    an amount above the balance."""
    from . import marlin as M
    from . import workloads as W
    txs = list(txs)
    circuit, pk, _ = state.pedersen_payment_keys(rng)
    known = [i for i, tx in enumerate(txs) if tx.sender in state.id_to_account_info and tx.recipient in state.id_to_account_info]
    out = [None] * len(txs)
    if not known:
        return out
    tree = state.account_merkle_tree
    block = [(txs[i].message(), txs[i].signature.to_bytes()) + _payment_leaves(state, txs[i]) for i in known]
    proofs, _ = M.generate_pedersen_payment_proofs(pk, circuit, tree, block, rng)
    root = tree.root()
    for i, proof in zip(known, proofs):
        if proof is not None:
            out[i] = (proof, W.pedersen_payment_public_inputs(root, txs[i].message()))
    return out

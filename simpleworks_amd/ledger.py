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

    def __init__(self, sig_params, leaf_crh, two_to_one_crh):
        self.sig_params, self.leaf_crh, self.two_to_one_crh = sig_params, leaf_crh, two_to_one_crh
        self.leaf_crh_params, self.two_to_one_crh_params = leaf_crh, two_to_one_crh   # the reference's field names

    @classmethod
    def sample(cls, rng, ctx=None):
        """ledger.rs:42-51: the three setups draw from the one rng in this order (the Schnorr setup draws nothing)."""
        sig = schnorr.setup(rng, ctx)
        leaf = H.PedersenCRH.setup(rng, H.LEAF_WINDOWS, H.WINDOW_SIZE, ctx)
        inner = H.PedersenCRH.setup(rng, H.TWO_TO_ONE_WINDOWS, H.WINDOW_SIZE, ctx)
        return cls(sig, leaf, inner)

    def free(self):
        self.sig_params.free()
        self.leaf_crh.free()
        self.two_to_one_crh.free()


class AccountInformation:
    """account.rs:29-42: the public key (an affine point, as ints) and the balance."""

    def __init__(self, public_key, balance=0):
        self.public_key, self.balance = public_key, int(balance)

    def to_bytes_le(self):
        return schnorr.point_bytes(self.public_key) + self.balance.to_bytes(8, "little")


class State:
    """ledger::State.  The account tree is a hash.DeviceMerkleTree; ids are AccountId(u8), the first one handed out is 1."""

    def __init__(self, num_accounts, parameters):
        """ledger.rs:106-112 hands ark_std::log2(num_accounts) to MerkleTree::blank as the HEIGHT, and arkworks' height counts the
        leaf level: 32 accounts give height 5 and 2^4 = 16 leaves.  Mirrored as it stands.  Registering past the last leaf
        raises (the reference panics in tree.update: "should exist")."""
        self.parameters = parameters
        height = ark_log2(num_accounts)
        if height < 2:
            raise ValueError("State: %d accounts give a tree of height %d (MerkleTree::blank needs 2)" % (num_accounts, height))
        self.account_merkle_tree = H.DeviceMerkleTree.blank(parameters.leaf_crh, parameters.two_to_one_crh, height, LEAF_LEN)
        self.next_available_account = 1
        self.id_to_account_info = {}
        self.pub_key_to_id = {}
        self._proof_keys = None      # (SchnorrCircuit, proving key, verifying key), derived once

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

    def free(self):
        if self._proof_keys is not None:
            self._proof_keys[0].free()
            self._proof_keys[1].free()
            self._proof_keys = None
        self.account_merkle_tree.free()


def _prove_signature(state, public_key, message, signature, rng):
    """transaction.rs:108-126 with the State's keys: the proof of the signature circuit, then its verification."""
    from . import marlin as M
    circuit, pk, vk = state.proof_keys(rng)
    proof = M.generate_schnorr_proof(pk, circuit, public_key, message, signature.to_bytes(), rng)
    return M.verify_proof(vk, [], M.MarlinProof(proof), rng)


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
        result = bool(H.verify_paths(parameters.leaf_crh, parameters.two_to_one_crh, tree.height(), tree.root(), [info.to_bytes_le()],
                                     [self.sender], path)[0])
        sig_ok = schnorr.verify(parameters.sig_params, info.public_key, self.message(), self.signature)
        if sig_ok and prove:
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
    in_tree = H.verify_paths(parameters.leaf_crh, parameters.two_to_one_crh, tree.height(), tree.root(),
                             [info.to_bytes_le() for info in infos], senders, paths)
    keys = np.frombuffer(b"".join(schnorr.point_bytes(info.public_key) for info in infos), dtype=np.uint8).reshape(-1, 64)
    msgs = np.frombuffer(b"".join(txs[i].message() for i in known), dtype=np.uint8).reshape(-1, MESSAGE_LEN)
    sigs = np.frombuffer(b"".join(txs[i].signature.to_bytes() for i in known), dtype=np.uint8).reshape(-1, 64)
    signed = schnorr.verify_many(parameters.sig_params, keys, msgs, sigs)
    for k, i in enumerate(known):
        tx, sig_ok = txs[i], bool(signed[k])
        if sig_ok and prove:
            sig_ok = _prove_signature(state, infos[k].public_key, tx.message(), tx.signature, rng)
        out[i] = bool(in_tree[k]) and sig_ok and tx.amount <= infos[k].balance and tx.recipient in state.id_to_account_info
    return out

"""Big-integer model of a payment over a Pedersen account tree (TEST INFRASTRUCTURE ONLY), on top of tests/schnorr_model.py and the
Pedersen hash of simpleworks_amd.workloads (pedersen_hash_bits over MerkleParams' generators): a small ledger whose accounts sit
where the caller puts them, and payments with the inputs of workloads.build_pedersen_payment.  A leaf without an account is blank:
its digest is zero, as in MerkleTree::blank."""
import schnorr_model as S
from simpleworks_amd import workloads as W

MSG_LEN, LEAF_LEN = 10, 72


def message(sender, recipient, amount):
    return bytes([sender, recipient]) + amount.to_bytes(8, "little")


def leaf(secret, balance):
    return S.point_bytes(S.keygen(S.GENERATOR, secret)) + balance.to_bytes(8, "little")


def leaf_digest(params, data):
    return W.pedersen_hash_bits([(byte >> i) & 1 for byte in data for i in range(8)], params.leaf_gens)


def tree(params, height, leaves):
    """leaves: index -> bytes (any length up to 72).  -> the levels of the tree, levels[-1][0] the root."""
    levels = [[leaf_digest(params, leaves[i]) if i in leaves else 0 for i in range(1 << (height - 1))]]
    while len(levels[-1]) > 1:
        prev = levels[-1]
        levels.append([params.inner_hash(prev[2 * i], prev[2 * i + 1]) for i in range(len(prev) // 2)])
    return levels


def path(levels, index):
    return [levels[l][(index >> l) ^ 1] for l in range(len(levels) - 1)]


def payment(levels, leaves, secret, sender, recipient, amount, salt=None, nonce=987654321, flip_signature=False, paths=None):
    """A payment from the account at `sender` (whose secret key is `secret`) against the tree `levels` over `leaves`.  paths: (root,
    sender's path, recipient's path) from elsewhere, instead of `levels`."""
    if paths is None:
        paths = (levels[-1][0], path(levels, sender), path(levels, recipient))
    msg = message(sender, recipient, amount)
    sig = bytearray(S.sign(S.GENERATOR, salt, secret, S.keygen(S.GENERATOR, secret), nonce, msg))
    if flip_signature:
        sig[3] ^= 0x10
    balance = int.from_bytes(leaves[sender][64:], "little")
    flag = (1 if S.verify(S.GENERATOR, salt, leaves[sender][:64], msg, bytes(sig)) else 0) | (2 if amount <= balance else 0)
    return {"message": msg, "signature": bytes(sig), "sender_leaf": leaves[sender], "recipient_leaf": leaves[recipient],
            "sender_path": list(paths[1]), "recipient_path": list(paths[2]), "public": [paths[0], sender, recipient, amount], "flag": flag}


def build(params, height, p, salt=None, root=None, cs=None, **changed):
    """workloads.build_pedersen_payment over the payment `p` (with some of its fields `changed`) -> (cs, public inputs)."""
    q = dict(p, **changed)
    cs = W.ConstraintSystem() if cs is None else cs
    public = W.build_pedersen_payment(cs, S.GENERATOR, salt, params, height, q["message"], q["signature"], q["sender_leaf"],
                                      q["sender_path"], q["recipient_leaf"], q["recipient_path"], root)
    return cs, public

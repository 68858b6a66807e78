"""Big-integer model of a payment over a Poseidon account tree (TEST INFRASTRUCTURE ONLY), on top of tests/schnorr_model.py and
tests/poseidon_tree_model.py: a small ledger, a list of payments that covers every outcome of Transaction::validate, and for each
payment what the payment circuit publishes and the flag byte the library reports (bit 0: the signature verifies, bit 1: amount <=
balance).  tests/golden/gen_golden_payment.py writes it out as tests/golden/payment.json; the tests hold the model to the fixture
and the library to both."""
import poseidon_tree_model as T
import schnorr_model as S

MSG_LEN, LEAF_LEN = 10, 72
U64_MAX = (1 << 64) - 1
SECRETS = {1: 1234567, 2: 1234584, 3: 1234601}         # account id -> secret key
BALANCES = {1: 1000, 2: 5, 3: U64_MAX}
BLANK_ID = 5                                            # an id inside every tree of height >= 4 that has no account
# name, sender, recipient, amount, what is wrong with it
PAYMENTS = [("valid", 1, 2, 300, None),
            ("amount zero", 1, 2, 0, None),
            ("whole balance", 2, 1, 5, None),
            ("balance 2^64 - 1", 3, 1, U64_MAX - 7, None),
            ("overdraft by 1", 2, 1, 6, "overdraft"),
            ("flipped signature", 1, 2, 300, "signature"),
            ("blank recipient", 1, BLANK_ID, 300, "recipient"),
            ("to oneself", 1, 1, 10, None),
            ("overdraft to oneself", 1, 1, 1001, "overdraft")]      # the last two fit a tree of height 2


def message(sender, recipient, amount):
    return bytes([sender, recipient]) + amount.to_bytes(8, "little")


def leaf(public_key, balance):
    return S.point_bytes(public_key) + balance.to_bytes(8, "little")


def ledger(params, height, salt=None):
    """-> (leaves: id -> 72 bytes, levels of the tree): accounts 1, 2, 3 in a tree whose other leaves are blank (digest zero)."""
    keys = {i: S.keygen(S.GENERATOR, sk) for i, sk in SECRETS.items()}
    leaves = {i: leaf(keys[i], BALANCES[i]) for i in keys if i < 1 << (height - 1)}
    levels = [[T.HL(params, leaves[i]) if i in leaves else 0 for i in range(1 << (height - 1))]]
    while len(levels[-1]) > 1:
        prev = levels[-1]
        levels.append([T.H2(params, prev[2 * i], prev[2 * i + 1]) for i in range(len(prev) // 2)])
    return leaves, levels


def payments(params, height, salt=None, which=PAYMENTS):
    """The payments of `which` against ledger(params, height): dicts with the inputs of the circuit, the public inputs the circuit
    publishes (the tree's root, sender, recipient, amount) and the flag byte."""
    leaves, levels = ledger(params, height, salt)
    root = levels[-1][0]
    out = []
    for k, (name, sender, recipient, amount, wrong) in enumerate(which):
        if max(sender, recipient) >> (height - 1):
            continue
        msg = message(sender, recipient, amount)
        key = S.keygen(S.GENERATOR, SECRETS[sender])
        sig = bytearray(S.sign(S.GENERATOR, salt, SECRETS[sender], key, 987654321 + k, msg))
        if wrong == "signature":
            sig[3] ^= 0x10
        sig = bytes(sig)
        recipient_leaf = leaves.get(recipient, bytes(LEAF_LEN))   # a blank leaf holds nothing: any 72 bytes fail its membership
        flag = (1 if S.verify(S.GENERATOR, salt, leaves[sender][:64], msg, sig) else 0) | (2 if amount <= BALANCES[sender] else 0)
        out.append({"name": name, "wrong": wrong, "message": msg, "signature": sig, "sender_leaf": leaves[sender],
                    "recipient_leaf": recipient_leaf, "sender_path": T.path(levels, sender), "recipient_path": T.path(levels, recipient),
                    "public": [root, sender, recipient, amount], "flag": flag})
    return out

"""Big-integer model of a block of transfers over a Poseidon account tree (TEST INFRASTRUCTURE ONLY), on top of
tests/payment_model.py and tests/poseidon_tree_model.py: a small ledger, a block of transfers applied IN ORDER, and for each
transfer the inputs of the transfer circuit (the sender's leaf and path in the tree before it, the recipient's in the intermediate
tree), the flag byte and status word the library reports, the root pair it publishes and the account table after it.
tests/golden/gen_golden_transfer.py writes it out as tests/golden/transfer.json.

flag byte: 1 the signature verifies, 2 amount <= balance, 4 rbalance + amount < 2^64, 8 both leaves hold an account, 16 applied.
status:    1 the sender's key is no point of the curve (a blank sender), 4 an id at or above 2^L, 8 sender == recipient.
A transfer is applied exactly when flag bits 0 .. 3 are set and the status is zero; a refused one leaves table and tree as they
were and publishes new_root = old_root."""
import payment_model as PM
import poseidon_tree_model as T
import schnorr_model as S

MSG_LEN, LEAF_LEN = PM.MSG_LEN, PM.LEAF_LEN
U64_MAX = PM.U64_MAX
SIG_OK, BALANCE_OK, SUM_OK, ACCOUNTS_OK, APPLIED = 1, 2, 4, 8, 16
ST_KEY, ST_ID, ST_SELF = 1, 4, 8
BLANK_ID = 5
TOP = "top"          # stands for the id 2^(L-1): its path meets that of id 1 at the top level


def secret(i):
    return 1234567 + 17 * i


def accounts(height):
    """id -> balance: ids 0 .. 3 and 2^(L-1), as far as the tree holds them."""
    n = 1 << (height - 1)
    out = {i: b for i, b in ((0, 50), (1, 1000), (2, 5), (3, U64_MAX - 300)) if i < n}
    if n // 2 >= 4:
        out[n // 2] = 7
    return out


# name, sender, recipient, amount, what is wrong with it.  In this order at height >= 4: every amount is what its name says.
TRANSFERS = [("meet at level 0", 2, 3, 1, None),                # the sender to the left
             ("sender to the right", 3, 2, 1, None),
             ("meet at the top level", 1, TOP, 10, None),
             ("amount zero", 1, 2, 0, None),
             ("whole balance", 2, 1, 5, None),
             ("sum 2^64 - 1", 1, 3, 300, None),
             ("overflow by 1", 1, 3, 1, "overflow"),
             ("overdraft by 1", 2, 1, 1, "overdraft"),
             ("flipped signature", 1, 2, 3, "signature"),
             ("blank recipient", 1, BLANK_ID, 3, "recipient"),
             ("to oneself", 1, 1, 10, "self"),
             ("id out of range", 1, "out", 1, "id"),             # 2^L + 2: the path of id 2
             ("zero to one", 0, 1, 50, None),                     # these two fit a tree of height 2
             ("one to zero", 1, 0, 1, None),
             ("after the refusals", TOP, 1, 17, None)]
CHAIN = [("one to two", 1, 2, 600, None), ("two to three", 2, 3, 200, None), ("refused in the middle", 3, 1, 1, "signature"),
         ("overdrawn in the middle", 2, 1, 406, "overdraft"), ("three to one", 3, 1, 100, None), ("two to one", 2, 1, 405, None)]


def _tree(params, table, height):
    levels = [[T.HL(params, leaf) if any(leaf) else 0 for leaf in table]]
    while len(levels[-1]) > 1:
        levels.append(T._up(params, levels[-1]))
    return levels


def _set(params, levels, index, digest):
    levels = [list(level) for level in levels]
    levels[0][index] = digest
    for l in range(1, len(levels)):
        index >>= 1
        levels[l][index] = T.H2(params, levels[l - 1][2 * index], levels[l - 1][2 * index + 1])
    return levels


def ledger(params, height, balances=None):
    """-> (table: 2^L leaves of 72 bytes, all-zero = no account; the tree's levels).  balances: id -> balance, instead of
    accounts(height)'s for those ids."""
    table = [bytes(LEAF_LEN)] * (1 << (height - 1))
    for i, balance in accounts(height).items():
        table[i] = PM.leaf(S.keygen(S.GENERATOR, secret(i)), (balances or {}).get(i, balance))
    return table, _tree(params, table, height)


def transfers(params, height, salt=None, which=TRANSFERS, balances=None):
    """The block `which` against ledger(params, height, balances), in order.  -> (initial table, transfers, final table, final levels); a
    transfer is a dict with the circuit's inputs, "public" = [old_root, new_root, sender, recipient, amount], "r1" (the intermediate
    root), "flag", "status", "applied" and "table" (the table after it).  Transfers whose ids the tree does not hold are left
    out, but for the one that is about that."""
    levels_n = height - 1
    n = 1 << levels_n
    table, levels = ledger(params, height, balances)
    first = list(table)
    out = []
    for k, (name, sender, recipient, amount, wrong) in enumerate(which):
        sender = n // 2 if sender == TOP else sender
        recipient = n // 2 if recipient == TOP else n + 2 if recipient == "out" else recipient
        if sender >= n or (recipient >= n and wrong != "id") or recipient > 255 or (TOP in which[k][1:3] and n // 2 < 4):
            continue
        msg = PM.message(sender, recipient, amount)
        s, r = sender & (n - 1), recipient & (n - 1)
        sk = secret(sender)
        sig = bytearray(S.sign(S.GENERATOR, salt, sk, S.keygen(S.GENERATOR, sk), 987654321 + k, msg))
        if wrong == "signature":
            sig[3] ^= 0x10
        sig = bytes(sig)
        sender_leaf = table[s]
        balance = int.from_bytes(sender_leaf[64:], "little")
        debited = sender_leaf[:64] + ((balance - amount) % (1 << 64)).to_bytes(8, "little")
        table1 = list(table)
        table1[s] = debited
        levels1 = _set(params, levels, s, T.HL(params, debited))
        recipient_leaf = table1[r]
        rbalance = int.from_bytes(recipient_leaf[64:], "little")
        credited = recipient_leaf[:64] + ((rbalance + amount) % (1 << 64)).to_bytes(8, "little")
        table2 = list(table1)
        table2[r] = credited
        levels2 = _set(params, levels1, r, T.HL(params, credited))
        key_ok = any(sender_leaf)        # a blank leaf's key (0, 0) is no point of the curve
        flag = (SIG_OK if key_ok and S.verify(S.GENERATOR, salt, sender_leaf[:64], msg, sig) else 0) | (BALANCE_OK if amount <= balance else 0) \
            | (SUM_OK if rbalance + amount <= U64_MAX else 0) | (ACCOUNTS_OK if any(sender_leaf) and any(table[r]) else 0)
        status = (0 if key_ok else ST_KEY) | (ST_ID if max(sender, recipient) >= n else 0) | (ST_SELF if sender == recipient else 0)
        applied = flag == 15 and status == 0
        old_root = levels[-1][0]
        t = {"name": name, "wrong": wrong, "message": msg, "signature": sig, "sender_leaf": sender_leaf, "recipient_leaf": recipient_leaf,
             "sender_path": T.path(levels, s), "recipient_path": T.path(levels1, r), "old_recipient_path": T.path(levels, r),
             "r1": levels1[-1][0], "walked_new_root": levels2[-1][0], "flag": flag | (APPLIED if applied else 0), "status": status,
             "applied": applied}
        if applied:
            table, levels = table2, levels2
        t["public"] = [old_root, levels[-1][0], sender, recipient, amount]
        t["table"] = list(table)
        out.append(t)
    return first, out, table, levels

"""Big-integer model of a block of transfers over a Pedersen account tree (TEST INFRASTRUCTURE ONLY): tests/transfer_model.py's
block advance — the same ledger, the same named transfers, the same flag byte and status word, the same applied / refused decision
— over the tree of tests/pedersen_payment_model.py (W.MerkleParams integers, a blank leaf's digest is zero).  For each transfer:
the inputs of workloads.build_pedersen_transfer (the sender's leaf and path in the tree before it, the recipient's in the
intermediate tree), the four walks (sender old, sender new, recipient in the tree of R1, recipient new: digests cur_0 .. cur_L over
two sibling arrays), the root pair it publishes and the account table after it.

flag byte: 1 the signature verifies, 2 amount <= balance, 4 rbalance + amount < 2^64, 8 both leaves hold an account, 16 applied.
status:    1 the sender's key is no point of the curve (a blank sender), 4 an id at or above 2^L, 8 sender == recipient.
A transfer is applied exactly when flag bits 0 .. 3 are set and the status is zero; a refused one leaves table and tree as they
were and publishes new_root = old_root."""
import pedersen_payment_model as PM
import schnorr_model as S
import transfer_model as TM

MSG_LEN, LEAF_LEN = PM.MSG_LEN, PM.LEAF_LEN
U64_MAX = TM.U64_MAX
SIG_OK, BALANCE_OK, SUM_OK, ACCOUNTS_OK, APPLIED = TM.SIG_OK, TM.BALANCE_OK, TM.SUM_OK, TM.ACCOUNTS_OK, TM.APPLIED
ST_KEY, ST_ID, ST_SELF = TM.ST_KEY, TM.ST_ID, TM.ST_SELF
BLANK_ID, TOP = TM.BLANK_ID, TM.TOP
TRANSFERS, CHAIN = TM.TRANSFERS, TM.CHAIN
secret, accounts = TM.secret, TM.accounts
# the ring 1 -> 2 -> 3 -> 1: every account is credited and then debited by the next transfer
RING = [("one to two", 1, 2, 7, None), ("two to three", 2, 3, 9, None), ("three to one", 3, 1, 11, None)]


def digest(params, leaf):
    """The tree's digest of a table entry: an all-zero entry is a blank leaf."""
    return PM.leaf_digest(params, leaf) if any(leaf) else 0


def ledger(params, height, balances=None):
    """-> (table: 2^L leaves of 72 bytes, all-zero = no account; the tree's levels).  balances: id -> balance, instead of
    accounts(height)'s for those ids."""
    table = [bytes(LEAF_LEN)] * (1 << (height - 1))
    for i, balance in accounts(height).items():
        table[i] = PM.leaf(secret(i), (balances or {}).get(i, balance))
    levels = [[digest(params, leaf) for leaf in table]]
    zero = {}        # a tree of height 9 is mostly blank: each pair of children is hashed once
    while len(levels[-1]) > 1:
        prev = levels[-1]
        up = []
        for i in range(len(prev) // 2):
            pair = (prev[2 * i], prev[2 * i + 1])
            if pair not in zero:
                zero[pair] = params.inner_hash(*pair)
            up.append(zero[pair])
        levels.append(up)
    return table, levels


def walk(params, leaf_digest_v, index, siblings):
    """The digests cur_0 .. cur_L of a leaf digest walked up `siblings`."""
    curs = [leaf_digest_v]
    for l, s in enumerate(siblings):
        c = curs[-1]
        curs.append(params.inner_hash(s, c) if (index >> l) & 1 else params.inner_hash(c, s))
    return curs


def _set(levels, index, curs):
    """The tree with the walk `curs` of leaf `index` written in."""
    levels = [list(level) for level in levels]
    for l, c in enumerate(curs):
        levels[l][index >> l] = c
    return levels


def transfers(params, height, salt=None, which=TRANSFERS, balances=None):
    """The block `which` against ledger(params, height, balances), in order.  -> (initial table, transfers, final table, final levels); a
    transfer is a dict with the circuit's inputs, "public" = [old_root, new_root, sender, recipient, amount], "r1" (the intermediate
    root), "walks" (the four digest arrays), "flag", "status", "applied" and "table" (the table after it).  Transfers whose ids the
    tree does not hold are left out, but for the one that is about that."""
    n = 1 << (height - 1)
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
        sender_path = PM.path(levels, s)
        sender_old = walk(params, levels[0][s], s, sender_path)
        sender_new = walk(params, PM.leaf_digest(params, debited), s, sender_path)
        table1 = list(table)
        table1[s] = debited
        levels1 = _set(levels, s, sender_new)
        recipient_leaf = table1[r]
        rbalance = int.from_bytes(recipient_leaf[64:], "little")
        credited = recipient_leaf[:64] + ((rbalance + amount) % (1 << 64)).to_bytes(8, "little")
        recipient_path = PM.path(levels1, r)
        recipient_mid = walk(params, levels1[0][r], r, recipient_path)
        recipient_new = walk(params, PM.leaf_digest(params, credited), r, recipient_path)
        table2 = list(table1)
        table2[r] = credited
        levels2 = _set(levels1, r, recipient_new)
        assert sender_old[-1] == levels[-1][0] and recipient_mid[-1] == sender_new[-1]
        key_ok = any(sender_leaf)        # a blank leaf's key (0, 0) is no point of the curve
        flag = (SIG_OK if key_ok and S.verify(S.GENERATOR, salt, sender_leaf[:64], msg, sig) else 0) | (BALANCE_OK if amount <= balance else 0) \
            | (SUM_OK if rbalance + amount <= U64_MAX else 0) | (ACCOUNTS_OK if any(sender_leaf) and any(table[r]) else 0)
        status = (0 if key_ok else ST_KEY) | (ST_ID if max(sender, recipient) >= n else 0) | (ST_SELF if sender == recipient else 0)
        applied = flag == 15 and status == 0
        old_root = levels[-1][0]
        t = {"name": name, "wrong": wrong, "message": msg, "signature": sig, "sender_leaf": sender_leaf, "recipient_leaf": recipient_leaf,
             "debited_leaf": debited, "credited_leaf": credited, "sender_path": sender_path, "recipient_path": recipient_path,
             "old_recipient_path": PM.path(levels, r), "r1": sender_new[-1], "walked_new_root": recipient_new[-1],
             "walks": {"sender_old": sender_old, "sender_new": sender_new, "recipient_mid": recipient_mid, "recipient_new": recipient_new},
             "flag": flag | (APPLIED if applied else 0), "status": status, "applied": applied}
        if applied:
            table, levels = table2, levels2
        t["public"] = [old_root, levels[-1][0], sender, recipient, amount]
        t["table"] = list(table)
        out.append(t)
    return first, out, table, levels


def build(params, height, t, salt=None, cs=None, **kw):
    """workloads.build_pedersen_transfer over the transfer `t` -> (cs, public inputs).  kw: old_root, new_root, r1."""
    from simpleworks_amd import workloads as W
    cs = W.ConstraintSystem() if cs is None else cs
    public = W.build_pedersen_transfer(cs, S.GENERATOR, salt, params, height, t["message"], t["signature"], t["sender_leaf"],
                                       t["sender_path"], t["recipient_leaf"], t["recipient_path"], **kw)
    return cs, public

"""Big-integer model of a block of account updates over a Pedersen account tree (TEST INFRASTRUCTURE ONLY): the block advance of
tests/account_update_model.py — the same operations, the same decision, flag and status word — over the tree of
tests/pedersen_payment_model.py (W.MerkleParams integers; a blank leaf's digest is zero, the Pedersen hash of 72 zero bytes, so the
blank leaf is a member like any other).  For each operation: the inputs of workloads.build_pedersen_account_update (id, key, the two
balances, fresh, the leaf's path in the tree before it), the two walks (the old path's digests cur_0 .. cur_L, gathered; the new
leaf's, hashed), the old and the new leaf bytes, the root pair it publishes and the account table after it.

An operation is (id, kind, 64 key bytes, balance): kind 0 sets the balance of the account at id (the key bytes are not read), kind
1 registers key || balance there.
status: 1 a registration's key coordinate is >= r, 2 id >= 2^L (alone), 4 registration of an occupied leaf, 8 balance update of a
blank leaf, 16 a registration whose leaf would be all-zero.  Applied (flag bit 0) exactly when the status is zero; a refused
operation leaves table and tree as they were and publishes new_root = old_root."""
import account_update_model as AM
import pedersen_payment_model as PM
import pedersen_transfer_model as TM

R = AM.R
LEAF_LEN = AM.LEAF_LEN
U64_MAX = AM.U64_MAX
SET, REGISTER = AM.SET, AM.REGISTER
ST_KEY, ST_ID, ST_OCCUPIED, ST_BLANK, ST_ZERO = AM.ST_KEY, AM.ST_ID, AM.ST_OCCUPIED, AM.ST_BLANK, AM.ST_ZERO
APPLIED = 1
NO_KEY = AM.NO_KEY
key, refusals, block_of = AM.key, AM.refusals, AM.block_of


def dependences(height):
    """account_update_model.dependences with the sibling pair at leaves 0 and 1, so that it serves height 3 too: a registration
    followed by a balance update of the same leaf; the leftmost and the rightmost leaf; two sibling leaves, the second's sibling being
    the first's new digest; a balance raised, lowered, and lowered to zero."""
    last = (1 << (height - 1)) - 1
    ops = [(last, REGISTER, key(last), 0), (last, SET, NO_KEY, 500), (0, REGISTER, key(0), 7)]
    if height > 2:
        ops += [(1, REGISTER, key(1), 0), (1, SET, NO_KEY, U64_MAX), (0, SET, NO_KEY, 9)]
    ops += [(last, SET, NO_KEY, 499), (0, SET, NO_KEY, 0)]
    return ops


def blank(params, height):
    """-> (table, levels) of State::new over the Pedersen tree: every leaf digest is zero."""
    return [bytes(LEAF_LEN)] * (1 << (height - 1)), PM.tree(params, height, {})


def apply(params, height, table, levels, ops):
    """The block `ops` against (table, levels), in order.  -> (operations, final table, final levels); an operation is a dict with the
    circuit's inputs ("id", "key" as two ints, "old_balance", "new_balance", "fresh", "path"), "old_root", "new_root", "status",
    "flag", "applied", "op" (as given), "old_leaf" (72 zero bytes for a registration), "new_leaf", "walks" ("old": the gathered
    digests, "new": the new leaf's walk; for a refused operation the old path twice) and "table" (the table after it)."""
    n = 1 << (height - 1)
    table = list(table)
    out = []
    for op in ops:
        index, kind, key_bytes, balance = op
        m = index & (n - 1)
        leaf = table[m]
        held = any(leaf)
        kb = bytes(key_bytes) if kind == REGISTER else leaf[:64]
        old_balance = 0 if kind == REGISTER else int.from_bytes(leaf[64:], "little")
        old_leaf = bytes(LEAF_LEN) if kind == REGISTER else leaf
        new_leaf = kb + balance.to_bytes(8, "little")
        x, y = int.from_bytes(kb[:32], "little"), int.from_bytes(kb[32:], "little")
        if index >= n:
            status = ST_ID
        elif kind == REGISTER:
            status = (ST_KEY if x >= R or y >= R else 0) | (ST_OCCUPIED if held else 0) | (0 if any(new_leaf) else ST_ZERO)
        else:
            status = 0 if held else ST_BLANK
        applied = status == 0
        path = PM.path(levels, m)
        old_walk = [levels[l][m >> l] for l in range(height)]
        t = {"op": op, "id": index, "key": (x, y), "old_balance": old_balance, "new_balance": balance, "fresh": kind, "path": path,
             "old_root": levels[-1][0], "status": status, "flag": APPLIED if applied else 0, "applied": applied, "old_leaf": old_leaf,
             "new_leaf": new_leaf, "walks": {"old": old_walk, "new": old_walk}}
        if applied:
            new_walk = TM.walk(params, PM.leaf_digest(params, new_leaf), m, path)
            t["walks"] = {"old": old_walk, "new": new_walk}
            table[m] = new_leaf
            levels = TM._set(levels, m, new_walk)
        t["new_root"] = levels[-1][0]
        t["table"] = list(table)
        out.append(t)
    return out, table, levels


def build(params, height, t, **kw):
    """workloads.pedersen_account_update_circuit over the operation `t` -> (cs, public inputs).  kw: any argument of the builder."""
    from simpleworks_amd import workloads as W
    args = dict(index=t["id"], key=t["key"], old_balance=t["old_balance"], new_balance=t["new_balance"], fresh=t["fresh"], siblings=t["path"])
    args.update(kw)
    return W.pedersen_account_update_circuit(params, height, **args)

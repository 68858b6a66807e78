"""Big-integer model of a block of account updates over a Poseidon account tree (TEST INFRASTRUCTURE ONLY), on top of
tests/poseidon_tree_model.py: a table of 2^L leaves of 72 bytes (all-zero = no account, level-0 node = the zero digest), a block of
registrations and balance updates applied IN ORDER, and for each operation the inputs of the account-update circuit
(workloads.build_account_update: id, key, the two balances, fresh, the leaf's path in the tree before it), the status word and the
flag the library reports, the root pair it publishes and the table after it.  tests/golden/gen_golden_account_update.py writes a
block out as tests/golden/account_update.json.

An operation is (id, kind, 64 key bytes, balance): kind 0 sets the balance of the account at id (the key bytes are not read), kind
1 registers key || balance there.
status: 1 a registration's key coordinate is >= r, 2 id >= 2^L (alone), 4 registration of an occupied leaf, 8 balance update of a
blank leaf, 16 a registration whose leaf would be all-zero.  Applied exactly when the status is zero; a refused operation leaves
table and tree as they were and publishes new_root = old_root."""
import poseidon_tree_model as T
import schnorr_model as S

R = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001
LEAF_LEN = 72
U64_MAX = (1 << 64) - 1
SET, REGISTER = 0, 1
ST_KEY, ST_ID, ST_OCCUPIED, ST_BLANK, ST_ZERO = 1, 2, 4, 8, 16
NO_KEY = bytes(64)


def key(i):
    """64 bytes: the public key of the i-th test account."""
    return S.point_bytes(S.keygen(S.GENERATOR, 1234567 + 17 * i))


def blank(params, height):
    """-> (table, levels) of State::new."""
    return [bytes(LEAF_LEN)] * (1 << (height - 1)), T.blank(params, height)


def _set(params, levels, index, digest):
    levels = [list(level) for level in levels]
    levels[0][index] = digest
    for l in range(1, len(levels)):
        index >>= 1
        levels[l][index] = T.H2(params, levels[l - 1][2 * index], levels[l - 1][2 * index + 1])
    return levels


def apply(params, height, table, levels, ops):
    """The block `ops` against (table, levels), in order.  -> (operations, final table, final levels); an operation is a dict with the
    circuit's inputs ("id", "key" as two ints, "old_balance", "new_balance", "fresh", "path"), "old_root", "new_root", "status",
    "applied", "op" (as given) and "table" (the table after it)."""
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
        new_leaf = kb + balance.to_bytes(8, "little")
        x, y = int.from_bytes(kb[:32], "little"), int.from_bytes(kb[32:], "little")
        if index >= n:
            status = ST_ID
        elif kind == REGISTER:
            status = (ST_KEY if x >= R or y >= R else 0) | (ST_OCCUPIED if held else 0) | (0 if any(new_leaf) else ST_ZERO)
        else:
            status = 0 if held else ST_BLANK
        applied = status == 0
        t = {"op": op, "id": index, "key": (x, y), "old_balance": old_balance, "new_balance": balance, "fresh": kind,
             "path": T.path(levels, m), "old_root": levels[-1][0], "status": status, "applied": applied, "new_leaf": new_leaf}
        if applied:
            table[m] = new_leaf
            levels = _set(params, levels, m, T.HL(params, new_leaf))
        t["new_root"] = levels[-1][0]
        t["table"] = list(table)
        out.append(t)
    return out, table, levels


def dependences(height):
    """A block from the blank tree that hits the advance kernel's dependences: a registration followed by a balance update of the same
    leaf; two sibling leaves, the second's sibling being the first's new digest; the leftmost and the rightmost leaf; a balance
    lowered; a registration with a balance of its own."""
    last = (1 << (height - 1)) - 1
    ops = [(last, REGISTER, key(last), 0), (last, SET, NO_KEY, 500),                  # register, then fund the same leaf
           (0, REGISTER, key(0), 7)]                                                  # the leftmost leaf, a balance of its own
    if height > 2:
        ops += [(2, REGISTER, key(2), 0), (3, REGISTER, key(3), 0), (3, SET, NO_KEY, U64_MAX), (2, SET, NO_KEY, 9)]     # siblings
    ops += [(last, SET, NO_KEY, 499), (0, SET, NO_KEY, 0)]                             # lowered; lowered to zero: not blank, the key stays
    return ops


def refusals(height):
    """(name, operation, status) of each refusal, against a tree that holds account 1 (height >= 3) or 0."""
    n = 1 << (height - 1)
    held, free = (1, 2) if n > 2 else (0, 1)
    big = (R).to_bytes(32, "little")
    return held, [("key not canonical", (free, REGISTER, key(5)[:32] + big, 0), ST_KEY),
                  ("key x not canonical", (free, REGISTER, big + key(5)[32:], 3), ST_KEY),
                  ("id out of range", (n + free, REGISTER, key(5), 0), ST_ID),
                  ("id out of range, update", (n + held, SET, NO_KEY, 4), ST_ID),
                  ("occupied", (held, REGISTER, key(6), 0), ST_OCCUPIED),
                  ("blank", (free, SET, NO_KEY, 10), ST_BLANK),
                  ("all-zero leaf", (free, REGISTER, NO_KEY, 0), ST_ZERO)]


def block_of(count, height=4):
    """`count` operations among the leaves of a small tree whose outcomes depend on their order: every leaf is registered the first
    time it comes up and funded after that; items 9 and 63 (count > 63, height 4) are refused: a second registration."""
    n = 1 << (height - 1)
    ops, seen = [], set()
    for k in range(count):
        leaf = (5 * k + k // n) % n
        if k in (9, 63) and leaf in seen:
            ops.append((leaf, REGISTER, key(leaf), 1))
        elif leaf in seen:
            ops.append((leaf, SET, NO_KEY, 1000 * k + leaf))
        else:
            seen.add(leaf)
            ops.append((leaf, REGISTER, key(leaf), k % 3))
    return ops

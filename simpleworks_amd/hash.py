"""Native Pedersen hash, Pedersen Merkle tree, Poseidon sponge and Poseidon Merkle tree, computed on the GPU (csrc/pedersen.hip,
csrc/merkle_tree.hip, csrc/poseidon.hip and csrc/poseidon_tree.hip through include/swmarlin.h).

Caller-facing mirror of what the reference reaches through ark-crypto-primitives 0.3:
    src/hash/mod.rs:13-28                           pedersen_hash(input): LeafWindow 144 x 4, parameters from a fresh test_rng
    src/merkle_tree/simple_merkle_tree.rs:43-49     <LeafHash as CRH>::setup(&mut rng), <TwoToOneHash as TwoToOneCRH>::setup(&mut rng),
                                                    MerkleTree::<MerkleConfig>::new(&leaf_crh_params, &two_to_one_crh_params, leaves)
    src/merkle_tree/simple_merkle_tree.rs:99-103    tree.generate_proof(leaf_index), tree.root()
    src/merkle_tree/common.rs:11-30                 the two window shapes
    examples/simple-payments/ledger.rs:106-173      MerkleTree::blank, tree.update, tree.root (DeviceMerkleTree: the tree stays on
                                                    the GPU between calls)
    examples/simple-payments/transaction.rs:163-173 tree.generate_proof, Path::verify (generate_proofs, verify_paths)
and through ark-sponge 0.3:
    src/hash/mod.rs:30-43                           poseidon2_hash(input): PoseidonSponge<Fq>, absorb the bytes, squeeze one element
PoseidonMerkleTree, verify_poseidon_paths and PoseidonMembershipCircuit have no counterpart in the reference: a Merkle tree over that
sponge with DeviceMerkleTree's calls, and the witness of its membership circuit.

Host side (this file): sampling the parameters — CRH::setup is a few hundred curve operations, done with Python integers the
way ark-ec samples a twisted Edwards point [U] — and the tree's bookkeeping.  Every hash runs on the GPU; there is no CPU
evaluation path here (the checker lives under oracle/).
"""
import json

import numpy as np

from ._lib import poseidon_pack_bytes  # noqa: F401  (the sponge's byte-to-element rule on the host)
from .marlin import (R_MODULUS, default_context, generate_rand, merkle_circuit_shape, poseidon_circuit_shape,
                     poseidon_membership_circuit_shape)

ED_D = 3021            # ed-on-BLS12-377: -x^2 + y^2 = 1 + 3021 x^2 y^2 over BLS12-377 Fr
ED_COFACTOR = 4
LEAF_WINDOWS, TWO_TO_ONE_WINDOWS, WINDOW_SIZE = 144, 128, 4   # src/merkle_tree/common.rs:16-30, src/hash/mod.rs:16-19
_MONT_RINV = pow(1 << 256, -1, R_MODULUS)


def ed_add(p, q):
    """Unified affine addition (a = -1)."""
    x1, y1 = p
    x2, y2 = q
    t = ED_D * x1 % R_MODULUS * x2 % R_MODULUS * y1 % R_MODULUS * y2 % R_MODULUS
    x3 = (x1 * y2 + y1 * x2) * pow(1 + t, -1, R_MODULUS) % R_MODULUS
    y3 = (y1 * y2 + x1 * x2) * pow(1 - t, -1, R_MODULUS) % R_MODULUS
    return x3, y3


def fr_sqrt(v):
    """Tonelli-Shanks in Fr (two-adicity 47); None for a non-residue."""
    v %= R_MODULUS
    if v == 0:
        return 0
    if pow(v, (R_MODULUS - 1) // 2, R_MODULUS) != 1:
        return None
    q = (R_MODULUS - 1) >> 47
    m, c, t, r = 47, pow(22, q, R_MODULUS), pow(v, q, R_MODULUS), pow(v, (q + 1) // 2, R_MODULUS)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % R_MODULUS
            i += 1
        b = pow(c, 1 << (m - i - 1), R_MODULUS)
        m, c = i, b * b % R_MODULUS
        t, r = t * c % R_MODULUS, r * b % R_MODULUS
    return r


def _rand_fr(rng):
    """ark-ff UniformRand for Fr: the accepted limbs are the Montgomery representation (swm_rng_rand_fr returns them)."""
    limbs = rng.rand_fr_mont()
    return sum(int(l) << (64 * i) for i, l in enumerate(limbs)) * _MONT_RINV % R_MODULUS


def _gen_bool(rng):
    """rand 0.8 Standard for bool: the sign bit of next_u32 (fill_bytes(4) consumes exactly that word)."""
    return rng.fill_bytes(4)[3] >> 7 == 1


def ed_rand(rng):
    """ark-ec 0.3 twisted_edwards_extended, Distribution<GroupProjective<P>> for Standard [U]: x = Fq::rand, greatest =
    rng.gen(), y from get_point_from_x (y^2 = (a x^2 - 1) / (d x^2 - 1), the root with (y < -y) ^ greatest), then
    scale_by_cofactor; repeat while x is not an abscissa of the curve."""
    while True:
        x = _rand_fr(rng)
        greatest = _gen_bool(rng)
        x2 = x * x % R_MODULUS
        den = (ED_D * x2 - 1) % R_MODULUS
        if den == 0:
            continue
        y = fr_sqrt((-x2 - 1) * pow(den, -1, R_MODULUS))
        if y is None:
            continue
        negy = (-y) % R_MODULUS
        y = y if (y < negy) ^ greatest else negy
        p = (x, y)
        for _ in range(2):  # cofactor 4
            p = ed_add(p, p)
        return p


def pedersen_setup(rng, num_windows, window_size=WINDOW_SIZE):
    """pedersen::CRH::setup -> Parameters.generators [U]: per window a random point and its doublings."""
    gens = []
    for _ in range(num_windows):
        base = ed_rand(rng)
        row = []
        for _ in range(window_size):
            row.append(base)
            base = ed_add(base, base)
        gens.append(row)
    return gens


class PedersenCRH:
    """PedersenCRHCompressor<EdwardsProjective, TECompressor, W> with its Parameters resident on the GPU."""

    def __init__(self, generators, ctx=None):
        self.ctx = ctx or default_context()
        self.generators = generators
        self.num_windows, self.window_size = len(generators), len(generators[0])
        raw = b"".join(x.to_bytes(32, "little") + y.to_bytes(32, "little") for row in generators for x, y in row)
        self.h = self.ctx.pedersen_create(raw, self.num_windows, self.window_size)

    @classmethod
    def setup(cls, rng, num_windows, window_size=WINDOW_SIZE, ctx=None):
        return cls(pedersen_setup(rng, num_windows, window_size), ctx)

    def evaluate_many(self, inputs):
        """inputs: uint8 [count, input_len] -> uint8 [count, 32] (CRH::evaluate + to_bytes! of each digest)."""
        return self.ctx.pedersen_hash(self.h, inputs)

    def evaluate(self, data):
        """CRH::evaluate(&params, input) -> Fq (as an integer)."""
        a = np.frombuffer(bytes(data), dtype=np.uint8).reshape(1, -1)
        return int.from_bytes(self.evaluate_many(a)[0].tobytes(), "little")

    def free(self):
        if self.h:
            self.ctx.pedersen_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def pedersen_hash(data, ctx=None):
    """src/hash/mod.rs:23-28: parameters from a fresh test_rng (144 windows of 4 bits), then evaluate."""
    crh = PedersenCRH.setup(generate_rand(), LEAF_WINDOWS, WINDOW_SIZE, ctx)
    try:
        return crh.evaluate(data)
    finally:
        crh.free()


def _leaf_bytes(leaves):
    rows = [bytes([v]) if isinstance(v, (int, np.integer)) else bytes(v) for v in leaves]   # to_bytes![leaf]; u8 -> one byte
    if len({len(r) for r in rows}) != 1:
        raise ValueError("leaves must serialise to the same number of bytes")
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1)


class MerkleTree:
    """ark_crypto_primitives::merkle_tree::MerkleTree over (LeafHash, TwoToOneHash): built by swm_merkle_tree_build."""

    def __init__(self, levels):
        self.levels = levels          # levels[0] = leaf digests ... levels[-1] = [root], uint8 [count, 32] each

    @staticmethod
    def new(leaf_crh, two_to_one_crh, leaves):
        a = _leaf_bytes(leaves)
        nodes = leaf_crh.ctx.merkle_tree_build(leaf_crh.h, two_to_one_crh.h, a)
        levels, off, cnt = [], 0, a.shape[0]
        while cnt >= 1:
            levels.append(nodes[off:off + cnt])
            off += cnt
            cnt >>= 1
        return MerkleTree(levels)

    def height(self):
        """tree.height() of ark-crypto-primitives: levels including the leaves."""
        return len(self.levels)

    def node(self, level, index):
        return int.from_bytes(self.levels[level][index].tobytes(), "little")

    def root(self):
        return self.node(len(self.levels) - 1, 0)

    def generate_proof(self, index):
        """Path of leaf `index`: the sibling digest at every level, bottom up (leaf sibling first), as integers."""
        if not 0 <= index < len(self.levels[0]):
            raise IndexError("leaf index out of range")
        return [self.node(lvl, (index >> lvl) ^ 1) for lvl in range(len(self.levels) - 1)]

    def int_levels(self):
        return [[int.from_bytes(r.tobytes(), "little") for r in lvl] for lvl in self.levels]


class DeviceMerkleTree:
    """ark_crypto_primitives::merkle_tree::MerkleTree over (LeafHash, TwoToOneHash) that stays on the GPU (swm_merkle_tree): the
    account tree of examples/simple-payments/ledger.rs.  blank / new / update / root / generate_proof carry arkworks' names and
    meaning [U]; update_many and generate_proofs are the batched forms (one call each).  Refers to the two PedersenCRH: keep them
    alive."""

    def __init__(self, leaf_crh, two_to_one_crh, handle, height, leaf_len):
        self.ctx = leaf_crh.ctx
        self.leaf_crh, self.two_to_one_crh = leaf_crh, two_to_one_crh
        self.h, self._height, self.leaf_len = handle, height, leaf_len

    @staticmethod
    def blank(leaf_crh, two_to_one_crh, height, leaf_len):
        """MerkleTree::blank: 2^(height - 1) leaves whose digests are 32 zero bytes (the hash of nothing); `height` counts the leaf
        level.  leaf_len: the bytes of every leaf that update() will write."""
        h = leaf_crh.ctx.merkle_tree_create_blank(leaf_crh.h, two_to_one_crh.h, height, leaf_len)
        return DeviceMerkleTree(leaf_crh, two_to_one_crh, h, height, leaf_len)

    @staticmethod
    def new(leaf_crh, two_to_one_crh, leaves):
        a = _leaf_bytes(leaves)
        h = leaf_crh.ctx.merkle_tree_create_from_leaves(leaf_crh.h, two_to_one_crh.h, a)
        return DeviceMerkleTree(leaf_crh, two_to_one_crh, h, a.shape[0].bit_length(), a.shape[1])

    def update(self, index, leaf):
        """tree.update(index, &leaf)."""
        self.update_many([index], [leaf])

    def update_many(self, indices, leaves):
        """The updates in order, in one call: a repeated index keeps its last leaf, every ancestor is hashed once."""
        indices = [int(i) for i in indices]
        if len(indices) != len(leaves):
            raise ValueError("one leaf per index")
        if indices:
            self.ctx.merkle_tree_update(self.h, np.asarray(indices, dtype=np.uint64), _leaf_bytes(leaves))

    def root(self):
        return int.from_bytes(self.ctx.merkle_tree_root(self.h).tobytes(), "little")

    def height(self):
        """tree.height() of ark-crypto-primitives: levels including the leaves."""
        return self._height

    def generate_proofs(self, indices):
        """-> uint8 [count, height - 1, 32]: per leaf the sibling digests bottom up, the form MerkleCircuit.witness_many and
        verify_paths take.  One launch."""
        return self.ctx.merkle_tree_paths(self.h, self._height - 1, np.asarray([int(i) for i in indices], dtype=np.uint64))

    def generate_proof(self, index):
        """Path of leaf `index`, as MerkleTree.generate_proof returns it: the siblings bottom up, as integers."""
        if not 0 <= index < 1 << (self._height - 1):
            raise IndexError("leaf index out of range")
        return [int.from_bytes(s.tobytes(), "little") for s in self.generate_proofs([index])[0]]

    def to_merkle_tree(self):
        """Downloads every node into a MerkleTree."""
        nodes = self.ctx.merkle_tree_nodes(self.h)
        levels, off, cnt = [], 0, 1 << (self._height - 1)
        while cnt >= 1:
            levels.append(nodes[off:off + cnt])
            off += cnt
            cnt >>= 1
        return MerkleTree(levels)

    def free(self):
        if self.h:
            self.ctx.merkle_tree_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def verify_paths(leaf_crh, two_to_one_crh, height, roots, leaves, indices, siblings):
    """Path::verify(&leaf_params, &two_to_one_params, &root, &leaf) for a batch, in one launch and without a tree
    (swm_merkle_verify_paths).  roots: one root for all paths (an int or 32 bytes) or one per path (a sequence of those, or uint8
    [count, 32]); leaves: as MerkleTree.new takes them; siblings: per path the siblings bottom up (ints, 32-byte strings, or uint8
    [count, height - 1, 32]).  Returns ok, bool [count]; a sibling or root that is no canonical field element, or an index beyond the
    leaves, is not ok."""
    def one(r):
        return bytes(r) if isinstance(r, (bytes, bytearray, np.ndarray)) else int(r).to_bytes(32, "little")
    if isinstance(roots, np.ndarray):
        r = np.ascontiguousarray(roots, dtype=np.uint8)
    elif isinstance(roots, (list, tuple)):
        r = np.frombuffer(b"".join(one(x) for x in roots), dtype=np.uint8).reshape(len(roots), 32)
    else:
        r = np.frombuffer(one(roots), dtype=np.uint8)
    idx = np.asarray([int(i) for i in indices], dtype=np.uint64)
    sib = _fr_rows(siblings)
    if not idx.shape[0]:
        return np.zeros(0, dtype=bool)
    ok, _ = leaf_crh.ctx.merkle_verify_paths(leaf_crh.h, two_to_one_crh.h, height, r, _leaf_bytes(leaves), idx, sib)
    return ok != 0


class MerkleCircuit:
    """The membership circuit of a tree of `height` levels over (LeafHash, TwoToOneHash), resident on the GPU
    (swm_merkle_circuit): synthesises the witness vector of workloads.build_merkle_membership (256-bit digests) for batches of
    (leaf, leaf index, authentication path) without running the builder.  Refers to the two PedersenCRH: keep them alive."""

    def __init__(self, leaf_crh, two_to_one_crh, height, gadget_byte_ops=0):
        self.ctx = leaf_crh.ctx
        self.leaf_crh, self.two_to_one_crh = leaf_crh, two_to_one_crh
        self.height, self.gadget_byte_ops = height, gadget_byte_ops
        self.h = self.ctx.merkle_circuit_create(leaf_crh.h, two_to_one_crh.h, height, gadget_byte_ops)

    def shape(self):
        """(num_instance, num_witness, num_constraints)."""
        return merkle_circuit_shape(self.height, self.gadget_byte_ops)

    def witness_many(self, leaves, indices, siblings):
        """leaves: u8 values; indices: leaf indices; siblings: per path the sibling digests bottom up, as ints or as 32
        little-endian bytes each.  One launch.  Returns (witness uint64 [count, num_witness, 4] Montgomery limbs, roots as ints)."""
        levels = self.height - 1
        rows = []
        for path in siblings:
            if len(path) != levels:
                raise ValueError("a path of this circuit has %d siblings" % levels)
            rows.append(b"".join(bytes(s) if isinstance(s, (bytes, bytearray, np.ndarray)) else int(s).to_bytes(32, "little") for s in path))
        sib = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), levels, 32)
        witness, roots = self.ctx.merkle_witness(self.h, self.shape()[1], np.asarray(list(leaves), dtype=np.uint8),
                                                 np.asarray(list(indices), dtype=np.uint64), sib)
        return witness, [int.from_bytes(r.tobytes(), "little") for r in roots]

    def free(self):
        if self.h:
            self.ctx.merkle_circuit_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PoseidonParameters:
    """ark_sponge::poseidon::PoseidonParameters<Fq> as PoseidonParameters::new(full_rounds, partial_rounds, alpha, mds, ark) builds
    it [U]: rate 2, capacity 1, a 3 x 3 matrix and full_rounds + partial_rounds rows of three round keys.  Entries are integers,
    reduced mod r here as F::from_str reduces the decimal strings of src/hash/helpers.rs.  The values are the caller's: this package
    restates no constant table."""

    def __init__(self, full_rounds, partial_rounds, alpha, mds, ark):
        self.full_rounds, self.partial_rounds, self.alpha = int(full_rounds), int(partial_rounds), int(alpha)
        self.mds = [[int(v) % R_MODULUS for v in row] for row in mds]
        self.ark = [[int(v) % R_MODULUS for v in row] for row in ark]
        if len(self.mds) != 3 or any(len(row) != 3 for row in self.mds):
            raise ValueError("mds must be 3 x 3 (rate 2 + capacity 1)")
        if len(self.ark) != self.full_rounds + self.partial_rounds or any(len(row) != 3 for row in self.ark):
            raise ValueError("ark must hold full_rounds + partial_rounds rows of 3 entries")

    @classmethod
    def from_json(cls, path):
        """{"full_rounds", "partial_rounds", "alpha", "mds": 3 x 3, "ark": rounds x 3}, entries as decimal strings or integers."""
        with open(path) as f:
            d = json.load(f)
        return cls(d["full_rounds"], d["partial_rounds"], d["alpha"], d["mds"], d["ark"])


def _fr_rows(items):
    """items: a uint8 array [count, n_in, 32], or a sequence of equally long sequences of ints / 32-byte strings."""
    if isinstance(items, np.ndarray):
        return np.ascontiguousarray(items, dtype=np.uint8)
    rows = [b"".join(bytes(e) if isinstance(e, (bytes, bytearray, np.ndarray)) else int(e).to_bytes(32, "little") for e in item)
            for item in items]
    if len({len(r) for r in rows}) > 1:
        raise ValueError("the items of one call hold the same number of elements")
    n_in = len(rows[0]) // 32 if rows else 0
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), n_in, 32)


class PoseidonSponge:
    """PoseidonSponge<Fq> with its parameters resident on the GPU (swm_poseidon): every call absorbs into a fresh sponge per item
    and squeezes, one GPU lane per item."""

    def __init__(self, params, ctx=None):
        self.ctx = ctx or default_context()
        self.params = params
        mds = b"".join(v.to_bytes(32, "little") for row in params.mds for v in row)
        ark = b"".join(v.to_bytes(32, "little") for row in params.ark for v in row)
        self.h = self.ctx.poseidon_create(params.full_rounds, params.partial_rounds, params.alpha, mds, ark)

    def hash_many(self, inputs):
        """inputs: uint8 [count, input_len] -> uint8 [count, 32]: absorb(&input) and squeeze_native_field_elements(1) of each,
        as 32 little-endian bytes."""
        return self.ctx.poseidon_hash_bytes(self.h, inputs)

    def hash_elements_many(self, items, n_out=1):
        """items: per item the same number of field elements (ints or 32 little-endian bytes each; or uint8 [count, n_in, 32])
        -> uint8 [count, n_out, 32].  Two elements in and one out is a two-to-one compression."""
        return self.ctx.poseidon_hash_fr(self.h, _fr_rows(items), n_out)

    def free(self):
        if self.h:
            self.ctx.poseidon_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PoseidonCircuit:
    """The Poseidon hash circuit over a resident sponge (swm_poseidon_circuit): synthesises the witness vector of
    workloads.build_poseidon_hash for batches of inputs without running the builder, one GPU lane per input.  input_len: the bytes
    form (n_out = 1, the digest is the public input); n_in: the elements form.  Refers to the PoseidonSponge: keep it alive."""

    def __init__(self, sponge, input_len=None, n_in=None, n_out=1):
        if (input_len is None) == (n_in is None):
            raise ValueError("either input_len (bytes form) or n_in (elements form)")
        self.ctx, self.sponge = sponge.ctx, sponge
        self.bytes_form, self.input_len, self.n_in, self.n_out = n_in is None, input_len, n_in, n_out
        self.h = self.ctx.poseidon_circuit_create(sponge.h, self.bytes_form, input_len if self.bytes_form else n_in, n_out)

    def shape(self):
        """(num_instance, num_witness, num_constraints)."""
        return poseidon_circuit_shape(self.sponge.params, self.input_len, self.n_in, self.n_out)

    def pack_inputs(self, inputs):
        """bytes form: equally long byte strings or uint8 [count, input_len]; elements form: as PoseidonSponge.hash_elements_many."""
        if not self.bytes_form:
            a = _fr_rows(inputs)
            if a.shape[0] == 0:
                a = a.reshape(0, self.n_in, 32)
            if a.shape[1] != self.n_in:
                raise ValueError("an item of this circuit holds %d elements" % self.n_in)
            return a
        if isinstance(inputs, np.ndarray):
            a = np.ascontiguousarray(inputs, dtype=np.uint8)
        else:
            rows = [bytes(m) for m in inputs]
            if any(len(m) != self.input_len for m in rows):
                raise ValueError("an input of this circuit is %d bytes long" % self.input_len)
            a = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), self.input_len)
        if a.ndim != 2 or a.shape[1] != self.input_len:
            raise ValueError("an input of this circuit is %d bytes long" % self.input_len)
        return a.reshape(a.shape[0], self.input_len)

    def witness_many(self, inputs):
        """One launch (chunks above 1 GiB of witnesses).  Returns (witness uint64 [count, num_witness, 4], outputs uint8 [count, n_out, 32]): the
        public inputs as canonical little-endian bytes)."""
        return self.ctx.poseidon_witness(self.h, self.shape()[1], self.n_out, self.pack_inputs(inputs))

    def free(self):
        if self.h:
            self.ctx.poseidon_circuit_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PoseidonMerkleTree:
    """A Merkle tree over a PoseidonSponge that stays on the GPU (swm_poseidon_tree): leaf digest = the byte sponge of the leaf
    (poseidon2_hash), inner node = the two-to-one form, hash_elements_many([a, b], 1).  The calls carry DeviceMerkleTree's names and
    meaning.  Refers to the PoseidonSponge: keep it alive."""

    def __init__(self, sponge, handle, height, leaf_len):
        self.ctx, self.sponge = sponge.ctx, sponge
        self.h, self._height, self.leaf_len = handle, height, leaf_len

    @staticmethod
    def blank(sponge, height, leaf_len):
        """2^(height - 1) leaves whose digests are 32 zero bytes (the hash of nothing); `height` counts the leaf level.  leaf_len: the
        bytes of every leaf that update() will write."""
        return PoseidonMerkleTree(sponge, sponge.ctx.poseidon_tree_create_blank(sponge.h, height, leaf_len), height, leaf_len)

    @staticmethod
    def new(sponge, leaves):
        a = _leaf_bytes(leaves)
        return PoseidonMerkleTree(sponge, sponge.ctx.poseidon_tree_create_from_leaves(sponge.h, a), a.shape[0].bit_length(), a.shape[1])

    def update(self, index, leaf):
        self.update_many([index], [leaf])

    def update_many(self, indices, leaves):
        """The updates in order, in one call: a repeated index keeps its last leaf, every ancestor is hashed once."""
        indices = [int(i) for i in indices]
        if len(indices) != len(leaves):
            raise ValueError("one leaf per index")
        if indices:
            self.ctx.poseidon_tree_update(self.h, np.asarray(indices, dtype=np.uint64), _leaf_bytes(leaves))

    def root(self):
        return int.from_bytes(self.ctx.poseidon_tree_root(self.h).tobytes(), "little")

    def height(self):
        """Levels including the leaves."""
        return self._height

    def generate_proofs(self, indices):
        """-> uint8 [count, height - 1, 32]: per leaf the sibling digests bottom up, the form PoseidonMembershipCircuit.witness_many
        and verify_poseidon_paths take.  One launch."""
        return self.ctx.poseidon_tree_paths(self.h, self._height - 1, np.asarray([int(i) for i in indices], dtype=np.uint64))

    def generate_proof(self, index):
        """Path of leaf `index`: the siblings bottom up, as integers."""
        if not 0 <= index < 1 << (self._height - 1):
            raise IndexError("leaf index out of range")
        return [int.from_bytes(s.tobytes(), "little") for s in self.generate_proofs([index])[0]]

    def to_merkle_tree(self):
        """Downloads every node into a MerkleTree."""
        nodes = self.ctx.poseidon_tree_nodes(self.h)
        levels, off, cnt = [], 0, 1 << (self._height - 1)
        while cnt >= 1:
            levels.append(nodes[off:off + cnt])
            off += cnt
            cnt >>= 1
        return MerkleTree(levels)

    def free(self):
        if self.h:
            self.ctx.poseidon_tree_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _root_rows(roots):
    def one(r):
        return bytes(r) if isinstance(r, (bytes, bytearray, np.ndarray)) else int(r).to_bytes(32, "little")
    if isinstance(roots, np.ndarray):
        return np.ascontiguousarray(roots, dtype=np.uint8)
    if isinstance(roots, (list, tuple)):
        return np.frombuffer(b"".join(one(x) for x in roots), dtype=np.uint8).reshape(len(roots), 32)
    return np.frombuffer(one(roots), dtype=np.uint8)


def verify_poseidon_paths(sponge, height, roots, leaves, indices, siblings, with_status=False):
    """verify_paths for a Poseidon tree (swm_poseidon_verify_paths): one launch, no tree.  Arguments as verify_paths.  Returns ok, bool
    [count] (with_status: also the status words: 0 computed, 1 a sibling or root >= r, 2 an index beyond the leaves)."""
    idx = np.asarray([int(i) for i in indices], dtype=np.uint64)
    if not idx.shape[0]:
        return (np.zeros(0, dtype=bool), np.zeros(0, dtype=np.uint32)) if with_status else np.zeros(0, dtype=bool)
    ok, status = sponge.ctx.poseidon_verify_paths(sponge.h, height, _root_rows(roots), _leaf_bytes(leaves), idx, _fr_rows(siblings))
    return (ok != 0, status) if with_status else ok != 0


class PoseidonMembershipCircuit:
    """The membership circuit over a Poseidon Merkle tree of `height` levels with leaves of leaf_len bytes, resident on the GPU
    (swm_poseidon_tree_circuit): synthesises the witness vector of workloads.build_poseidon_membership for batches of (leaf, leaf
    index, authentication path) without running the builder.  Refers to the PoseidonSponge: keep it alive."""

    def __init__(self, sponge, height, leaf_len):
        self.ctx, self.sponge = sponge.ctx, sponge
        self.height, self.leaf_len = height, leaf_len
        self.h = self.ctx.poseidon_tree_circuit_create(sponge.h, height, leaf_len)

    def shape(self):
        """(num_instance, num_witness, num_constraints)."""
        return poseidon_membership_circuit_shape(self.sponge.params, self.height, self.leaf_len)

    def witness_many(self, leaves, indices, siblings):
        """leaves: as PoseidonMerkleTree.new takes them; siblings: per path the sibling digests bottom up.  Returns (witness uint64
        [count, num_witness, 4] Montgomery limbs, roots as ints)."""
        witness, roots = self.ctx.poseidon_tree_witness(self.h, self.shape()[1], _leaf_bytes(leaves),
                                                        np.asarray([int(i) for i in indices], dtype=np.uint64), _fr_rows(siblings))
        return witness, [int.from_bytes(r.tobytes(), "little") for r in roots]

    def witness_at(self, tree, leaves, indices):
        """The same for leaves that a PoseidonMerkleTree holds: siblings and running digests are read from its nodes on the device."""
        return self.ctx.poseidon_tree_witness_at(self.h, tree.h, self.shape()[1], _leaf_bytes(leaves),
                                                 np.asarray([int(i) for i in indices], dtype=np.uint64))

    def free(self):
        if self.h:
            self.ctx.poseidon_tree_circuit_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def poseidon2_hash(data, params, ctx=None):
    """src/hash/mod.rs:32-43: a sponge over `params` (the reference takes helpers::poseidon_parameters_for_test()), absorb the
    bytes, the first squeezed element -> Fq (as an integer)."""
    sponge = PoseidonSponge(params, ctx)
    try:
        a = np.frombuffer(bytes(data), dtype=np.uint8).reshape(1, -1)
        return int.from_bytes(sponge.hash_many(a)[0].tobytes(), "little")
    finally:
        sponge.free()

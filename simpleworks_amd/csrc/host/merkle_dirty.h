// merkle_dirty.h — which nodes a batch of leaf updates dirties (merkle_tree.hip).  Plain C++, no GPU headers: checked on its own
// against a brute-force model under ASan / UBSan (tests/native/merkle_dirty_check.cpp).
//
// arkworks' MerkleTree::update(i, leaf) [U] rehashes leaf i and its height - 1 ancestors.  k updates applied in order leave the
// tree that ONE pass leaves which hashes, per touched leaf, the LAST leaf written to it, and then every ancestor of a touched
// leaf once, level by level: a node depends on its two children only.  From (height, indices) this header lists exactly that
// work: the level-0 jobs (leaf index, position in the batch of its last writer) and, per two-to-one level, the sorted unique
// parents.  Parent p of level l + 1 hashes nodes 2 p and 2 p + 1 of level l; the lists never grow going up.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace swm {

static constexpr size_t MT_MIN_HEIGHT = 2, MT_MAX_HEIGHT = 31;  // arkworks' height counts the leaf level: 2 .. 2^30 leaves

struct MerkleDirtyLeaf {
    uint32_t index;  // the leaf
    uint32_t src;    // position in the batch of the last update of that leaf
};
struct MerkleDirty {
    std::vector<MerkleDirtyLeaf> leaves;         // by ascending index, one per touched leaf
    std::vector<std::vector<uint32_t>> parents;  // [l], l < height - 1: nodes of level l + 1 to recompute, ascending, unique
};

inline bool merkle_height_ok(size_t height) { return height >= MT_MIN_HEIGHT && height <= MT_MAX_HEIGHT; }
// first node of level l in the node array (n leaf digests | n / 2 | ... | root), n = 2^levels leaves
inline size_t merkle_level_offset(size_t levels, size_t l) { return ((size_t)2 << levels) - (((size_t)2 << levels) >> l); }

enum MerkleDirtyStatus { MT_DIRTY_OK = 0, MT_DIRTY_BAD_HEIGHT = 1, MT_DIRTY_BAD_INDEX = 2, MT_DIRTY_TOO_MANY = 3 };

// *bad_at (may be null): the batch position of the first index >= n.  `out` is written only on MT_DIRTY_OK.
inline MerkleDirtyStatus merkle_dirty(size_t height, const uint64_t* indices, size_t count, MerkleDirty* out, size_t* bad_at) {
    if (!merkle_height_ok(height)) return MT_DIRTY_BAD_HEIGHT;
    if (count > 0xFFFFFFFFu) return MT_DIRTY_TOO_MANY;  // `src` is 32 bits wide
    const size_t levels = height - 1;
    const uint64_t n = (uint64_t)1 << levels;
    for (size_t i = 0; i < count; i++)
        if (indices[i] >= n) {
            if (bad_at) *bad_at = i;
            return MT_DIRTY_BAD_INDEX;
        }
    std::vector<std::pair<uint32_t, uint32_t>> order(count);  // (index, position): the pair order puts a leaf's last writer last
    for (size_t i = 0; i < count; i++) order[i] = {(uint32_t)indices[i], (uint32_t)i};
    std::sort(order.begin(), order.end());
    MerkleDirty d;
    for (size_t i = 0; i < count; i++)
        if (i + 1 == count || order[i + 1].first != order[i].first) d.leaves.push_back({order[i].first, order[i].second});
    d.parents.resize(levels);
    std::vector<uint32_t> cur(d.leaves.size());
    for (size_t i = 0; i < cur.size(); i++) cur[i] = d.leaves[i].index;
    for (size_t l = 0; l < levels; l++) {
        std::vector<uint32_t>& up = d.parents[l];
        for (uint32_t c : cur)
            if (up.empty() || up.back() != (c >> 1)) up.push_back(c >> 1);  // ascending children give ascending parents
        cur = up;
    }
    *out = std::move(d);
    return MT_DIRTY_OK;
}

}  // namespace swm

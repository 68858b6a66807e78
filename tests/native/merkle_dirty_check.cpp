// Stand-alone check of simpleworks_amd/csrc/host/merkle_dirty.h (built with -fsanitize=address,undefined by
// tests/test_merkle_dirty_host.py): the last-writer leaf jobs and the per-level parent lists of a batch of updates against a
// brute-force model — every ancestor marked in a bitmap per level, the last writer of a leaf found by a linear scan — for heights
// 2 .. 8, batch sizes 0 .. 2 n, the index patterns of the GPU tests and seeded random batches with duplicates; then the refusals.
// Prints "ok <cases>".
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "host/merkle_dirty.h"

using namespace swm;

static size_t cases = 0;

static bool fail(const char* what, size_t height, size_t k) {
    printf("FAIL %s (height %zu, batch of %zu)\n", what, height, k);
    return false;
}

static bool check(size_t height, const std::vector<uint64_t>& idx) {
    cases++;
    const size_t levels = height - 1, n = (size_t)1 << levels, k = idx.size();
    MerkleDirty d;
    size_t bad = 12345;
    if (merkle_dirty(height, idx.data(), k, &d, &bad) != MT_DIRTY_OK) return fail("refused", height, k);
    if (bad != 12345) return fail("bad_at written", height, k);
    // level 0: the last writer of every touched leaf, ascending
    size_t at = 0;
    for (size_t leaf = 0; leaf < n; leaf++) {
        long last = -1;
        for (size_t i = 0; i < k; i++)
            if (idx[i] == leaf) last = (long)i;
        if (last < 0) continue;
        if (at >= d.leaves.size() || d.leaves[at].index != leaf || d.leaves[at].src != (uint32_t)last) return fail("leaf job", height, k);
        at++;
    }
    if (at != d.leaves.size()) return fail("leaf job count", height, k);
    // every level: the marked ancestors, ascending, each once
    if (d.parents.size() != levels) return fail("level count", height, k);
    std::vector<char> mark(n, 0);
    for (uint64_t i : idx) mark[i] = 1;
    size_t below = d.leaves.size();
    for (size_t l = 0; l < levels; l++) {
        const size_t cnt = n >> (l + 1);
        std::vector<char> up(cnt, 0);
        for (size_t c = 0; c < 2 * cnt; c++)
            if (mark[c]) up[c >> 1] = 1;
        size_t pos = 0;
        for (size_t p = 0; p < cnt; p++) {
            if (!up[p]) continue;
            if (pos >= d.parents[l].size() || d.parents[l][pos] != p) return fail("parent list", height, k);
            pos++;
        }
        if (pos != d.parents[l].size()) return fail("parent count", height, k);
        if (pos > below) return fail("the dirty count grew", height, k);
        if (k && pos == 0) return fail("an empty level", height, k);
        below = pos;
        mark = up;
    }
    if (k && d.parents[levels - 1].size() != 1) return fail("root", height, k);
    if (merkle_level_offset(levels, 0) != 0 || merkle_level_offset(levels, levels) != 2 * n - 2) return fail("level offsets", height, k);
    return true;
}

static uint64_t rnd(uint64_t* s) {  // xorshift64
    *s ^= *s << 13;
    *s ^= *s >> 7;
    *s ^= *s << 17;
    return *s;
}

int main() {
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    for (size_t height = 2; height <= 8; height++) {
        const size_t n = (size_t)1 << (height - 1);
        for (size_t k = 0; k <= 2 * n; k++) {
            std::vector<uint64_t> v(k);
            // both children of one parent (and beyond: consecutive leaves from an odd start, wrapped)
            for (size_t i = 0; i < k; i++) v[i] = (n - 2 + i) % n;
            if (!check(height, v)) return 1;
            // all in one 8-leaf subtree (the last one)
            for (size_t i = 0; i < k; i++) v[i] = n - 1 - (i * 3) % (n < 8 ? n : 8);
            if (!check(height, v)) return 1;
            // as far apart as possible: bit-reversed counter, descending order
            for (size_t i = 0; i < k; i++) {
                size_t r = 0;
                for (size_t b = 0; b + 1 < height; b++) r |= (((k - 1 - i) >> b) & 1) << (height - 2 - b);
                v[i] = r;
            }
            if (!check(height, v)) return 1;
            // every leaf, descending, wrapped
            for (size_t i = 0; i < k; i++) v[i] = (n - 1 - i % n);
            if (!check(height, v)) return 1;
            // random with duplicates: drawn from the whole tree, and from a handful of leaves
            for (int rep = 0; rep < 4; rep++) {
                for (size_t i = 0; i < k; i++) v[i] = rnd(&seed) % (rep < 2 ? n : (n < 5 ? n : 5));
                if (!check(height, v)) return 1;
            }
        }
    }
    // refusals: `out` stays as it was
    MerkleDirty d;
    d.leaves.push_back({7, 7});
    const uint64_t one[3] = {0, 4, 1};
    size_t bad = 99;
    if (merkle_dirty(1, one, 1, &d, &bad) != MT_DIRTY_BAD_HEIGHT || merkle_dirty(0, one, 0, &d, &bad) != MT_DIRTY_BAD_HEIGHT ||
        merkle_dirty(32, one, 1, &d, &bad) != MT_DIRTY_BAD_HEIGHT || bad != 99) {
        printf("FAIL height bounds\n");
        return 1;
    }
    if (merkle_dirty(3, one, 3, &d, &bad) != MT_DIRTY_BAD_INDEX || bad != 1 || merkle_dirty(3, one, 3, &d, nullptr) != MT_DIRTY_BAD_INDEX) {
        printf("FAIL index >= n\n");
        return 1;
    }
    const uint64_t big[1] = {(uint64_t)1 << 30};
    if (merkle_dirty(31, big, 1, &d, &bad) != MT_DIRTY_BAD_INDEX || bad != 0 || merkle_dirty(4, one, 3, &d, &bad) != MT_DIRTY_OK) {
        printf("FAIL index at the height limit\n");
        return 1;
    }
    if (d.leaves.size() != 3 || d.leaves[2].index != 4 || d.leaves[2].src != 1) {
        printf("FAIL result after refusals\n");
        return 1;
    }
    const uint64_t top[2] = {((uint64_t)1 << 30) - 1, 0};  // the widest tree: indices and offsets stay in range
    if (merkle_dirty(31, top, 2, &d, &bad) != MT_DIRTY_OK || d.parents.size() != 30 || d.parents[0].size() != 2 ||
        d.parents[0][1] != ((uint32_t)1 << 29) - 1 || d.parents[29].size() != 1 ||
        merkle_level_offset(30, 30) != ((size_t)2 << 30) - 2) {
        printf("FAIL height 31\n");
        return 1;
    }
    cases += 8;
    printf("ok %zu\n", cases);
    return 0;
}

// witness_chunks.h — how a batch of witnesses is cut into chunks that fit the device stage, for every circuit unit
// (csrc/*_witness.hip through csrc/witness_host.h).  Plain C++, no GPU headers, no library state: tests/native/witness_chunks_check.cpp
// runs it on the CPU.
#pragma once
#include <stddef.h>

#include <vector>

namespace swm {

// The host forms hold at most this many bytes of witnesses on the device at a time; a larger batch goes in chunks.  The cap a
// driver uses is swm_ctx::witness_stage_bytes, which starts as this.
static constexpr size_t WITNESS_STAGE_BYTES = (size_t)1 << 30;

// Chunks go through the device IN ORDER: where items depend on each other (a block of transfers), item i + 1 is witnessed against
// the state item i left.
struct WitnessChunk {
    size_t base = 0, count = 0;  // items [base, base + count)
};

// How many items of `item_bytes` witness bytes each fit `cap_bytes`: at least one (a single item is never refused for its size).
// 0: item_bytes = 0.
inline size_t witness_chunk_items(size_t item_bytes, size_t cap_bytes) {
    if (item_bytes == 0) return 0;
    const size_t per = cap_bytes / item_bytes;
    return per ? per : 1;
}

// The chunks of `count` items at `per` items per chunk, as a range: consecutive, in order, every chunk but the last full.
// count = 0, or per = 0, gives no chunk.
struct WitnessChunks {
    size_t per, count;
    WitnessChunks(size_t per_, size_t count_) : per(per_), count(per_ ? count_ : 0) {}
    struct Iter {
        size_t per, count, base;
        WitnessChunk operator*() const {
            WitnessChunk c;
            c.base = base;
            c.count = count - base < per ? count - base : per;
            return c;
        }
        Iter& operator++() {
            base += (**this).count;
            return *this;
        }
        bool operator!=(const Iter& o) const { return base != o.base; }
    };
    Iter begin() const { return {per, count, 0}; }
    Iter end() const { return {per, count, count}; }
};

// The same as a list.  false: item_bytes = 0.
inline bool witness_chunk_plan(size_t item_bytes, size_t count, size_t cap_bytes, std::vector<WitnessChunk>* out) {
    out->clear();
    const size_t per = witness_chunk_items(item_bytes, cap_bytes);
    if (per == 0) return false;
    for (const WitnessChunk c : WitnessChunks(per, count)) out->push_back(c);
    return true;
}

}  // namespace swm

// ledger_bytes.cuh — how a ledger kernel reads the little-endian bytes of a message or a leaf, whatever the account tree hashes
// with: nothing here but ff.cuh.
#pragma once
#include <stdint.h>

#include "ff.cuh"

namespace swm {

__device__ __forceinline__ uint64_t le_load_u64(const uint8_t* b) {  // 8 little-endian bytes: an amount, a balance
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) v |= (uint64_t)b[k] << (8 * k);
    return v;
}

__device__ __forceinline__ bool le_below_r(const uint8_t* b) {  // 32 little-endian bytes below r: a key's coordinate
    Fr x, r;
#pragma unroll
    for (int w = 0; w < 8; w++) {
        x.v[w] = (uint32_t)b[4 * w] | (uint32_t)b[4 * w + 1] << 8 | (uint32_t)b[4 * w + 2] << 16 | (uint32_t)b[4 * w + 3] << 24;
        r.v[w] = FrParams::P[w];
    }
    return fp_cmp_std(x, r) < 0;
}

}  // namespace swm

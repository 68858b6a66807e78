// pedersen.cuh — the device side of ONE Pedersen hash, as pedersen.hip and merkle_tree.hip share it: the window loop of a lane,
// the shuffle tree that joins the lanes of a hash, and the digest.  See pedersen.hip for the method.
#pragma once
#include "ed.cuh"
#include "ff.cuh"
#include "frinv.cuh"

namespace swm {

// The partial sum of lane `lane` of `lanes`: windows lane, lane + lanes, ... of a `len`-byte input whose byte i is byte_at(i).
// Windows past the input are zero bits; a window reads at most two bytes (window_size <= 8).
template <class ByteAt>
__device__ __forceinline__ EdExt ped_partial(const EdRow* __restrict__ table, unsigned num_windows, unsigned ws, ByteAt byte_at, size_t len,
                                             unsigned lanes, unsigned lane) {
    EdExt acc = ed_identity();
    const size_t nbits = len * 8;
    const unsigned used = (unsigned)min((size_t)num_windows, (nbits + ws - 1) / ws);
    const unsigned mask = (1u << ws) - 1u;
#pragma unroll 1
    for (unsigned w = lane; w < used; w += lanes) {
        const size_t bit = (size_t)w * ws, byte = bit >> 3;
        unsigned v = byte_at(byte);
        if (byte + 1 < len) v |= (unsigned)byte_at(byte + 1) << 8;
        v = (v >> (bit & 7)) & mask;
        if (v) ed_madd(acc, table[((size_t)w << ws) + v]);
    }
    return acc;
}

// The sum over the `lanes` (a power of two <= 64, aligned in the wave) lanes of a hash; every lane of the wave takes part.
__device__ __forceinline__ EdExt ped_join(EdExt acc, unsigned lanes, const Fr& k2d) {
#pragma unroll 1
    for (unsigned s = lanes >> 1; s; s >>= 1) {
        EdExt other = ed_shfl_xor(acc, (int)s);
        acc = ed_add(acc, other, k2d);
    }
    return acc;
}

struct MtMsg64 {  // 64 message bytes in registers; a byte is picked by selects, never by a dynamic register index
    uint32_t w[16];
    __device__ __forceinline__ unsigned operator()(size_t i) const {
        const unsigned k = (unsigned)(i >> 2);
        uint32_t v = w[0];
#pragma unroll
        for (unsigned j = 1; j < 16; j++) v = k == j ? w[j] : v;
        return (v >> (8 * (i & 3))) & 0xFFu;
    }
};

// TECompressor: the affine x coordinate, canonical.  Z != 0: the law is complete.
__device__ __forceinline__ Fr ped_digest(const EdExt& acc) { return fp_to_std(fp_mul(acc.x, fr_inv_single(acc.z))); }

}  // namespace swm

// poseidon.h — the resident form of a Poseidon parameter set and how a kernel reads it and its inputs (poseidon.hip builds the
// table and hashes; poseidon_witness.hip records the circuit's witness from the same table).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ff.cuh"
#include "fr29.cuh"

struct swm_poseidon {
    unsigned full_rounds = 0, partial_rounds = 0, alpha = 0;
    void* d_table = nullptr;  // PS_ROW words per row: 2^522 | mds[0][0] .. mds[2][2] | ark[0][0] .. ark[F+P-1][2], every entry x 2^261
    size_t rows = 0;
};

namespace swm {

static constexpr unsigned PS_ROW = 12;      // words per table row: 9 limbs, padded to 48 bytes for 16-byte LDS reads
static constexpr unsigned PS_MDS = 1;       // first matrix row of the table (row 0 is 2^522)
static constexpr unsigned PS_ARK = 10;      // first round key
static constexpr unsigned PS_LANES = 64;    // one wave per workgroup
static constexpr size_t PS_MAX_IN = 4096, PS_MAX_OUT = 16, PS_MAX_BYTES = 65536, PS_MAX_ROUNDS = 255;

__device__ __forceinline__ Fr29 ps_row(const uint32_t* tab, unsigned row) {
    const uint4* p = reinterpret_cast<const uint4*>(tab + PS_ROW * row);
    const uint4 a = p[0], b = p[1];
    Fr29 r;
    r.l[0] = a.x, r.l[1] = a.y, r.l[2] = a.z, r.l[3] = a.w;
    r.l[4] = b.x, r.l[5] = b.y, r.l[6] = b.z, r.l[7] = b.w;
    r.l[8] = tab[PS_ROW * row + 8];
    return r;
}

// element e of item `item`: BYTES: the e-th 31-byte chunk of (length || input); else 32 bytes of the element array, with the
// canonical test (bad |= value >= r)
template <bool BYTES>
__device__ __forceinline__ Fr ps_fetch(const uint8_t* __restrict__ in, size_t item, size_t n_in, size_t e, bool& bad) {
    Fr x;
    if (BYTES) {
        const uint8_t* msg = in + item * n_in;  // n_in: the input length in bytes
        const size_t total = 8 + n_in;
#pragma unroll
        for (int w = 0; w < 8; w++) {
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (4 * w + j == 31) continue;
                const size_t pos = 31 * e + 4 * w + j;
                uint32_t byte = 0;
                if (pos < 8) byte = (uint32_t)((uint64_t)n_in >> (8 * pos)) & 0xFFu;
                else if (pos < total) byte = msg[pos - 8];
                v |= byte << (8 * j);
            }
            x.v[w] = v;
        }
    } else {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(in) + 8 * (item * n_in + e);
#pragma unroll
        for (int w = 0; w < 8; w++) x.v[w] = p[w];
        Fr r;
#pragma unroll
        for (int w = 0; w < 8; w++) r.v[w] = FrParams::P[w];
        bad |= fp_cmp_std(x, r) >= 0;
    }
    return x;
}

static bool ps_load_std(const uint8_t* b, Fr* out) {  // 32 little-endian bytes -> words; false when >= r
    Fr s, r;
    for (int i = 0; i < 8; i++) {
        s.v[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
        r.v[i] = FrParams::P[i];
    }
    *out = s;
    return fp_cmp_std(s, r) < 0;
}

}  // namespace swm

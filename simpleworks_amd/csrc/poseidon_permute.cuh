// poseidon_permute.cuh — one Poseidon permutation on one lane: shared by the sponge (poseidon.hip) and the Poseidon Merkle tree
// (poseidon_tree.h).  The arithmetic, the table layout and the bounds are those at the head of poseidon.hip.
#pragma once
#include "fr29.cuh"
#include "poseidon.h"

namespace swm {

// One permutation of the three lazy state entries (bounds: the head of poseidon.hip).
__device__ __forceinline__ void ps_permute(const uint32_t* tab, unsigned half_full, unsigned partial, unsigned alpha, int alpha_top,
                                           Fr29& s0, Fr29& s1, Fr29& s2) {
    const unsigned rounds = 2 * half_full + partial;
#pragma unroll 1
    for (unsigned i = 0; i < rounds; i++) {
        const bool full = i < half_full || i >= half_full + partial;
        const unsigned k = PS_ARK + 3 * i;
        // < 9r, limbs < 5 x 2^29; what the S-box takes is normalised because it is a second operand there
        const Fr29 t0 = fr29_normalize(fr29_add(s0, ps_row(tab, k)));
        Fr29 t1 = fr29_add(s1, ps_row(tab, k + 1)), t2 = fr29_add(s2, ps_row(tab, k + 2));
        if (full) {
            t1 = fr29_normalize(t1);
            t2 = fr29_normalize(t2);
        }
        Fr29 a0 = t0, a1 = t1, a2 = t2;  // x^alpha, left to right over the bits below the top one
#pragma unroll 1
        for (int b = alpha_top - 1; b >= 0; b--) {
            a0 = fr29_mul_fenced(a0, a0);
            if (full) {
                a1 = fr29_mul_fenced(a1, a1);
                a2 = fr29_mul_fenced(a2, a2);
            }
            if ((alpha >> b) & 1u) {
                a0 = fr29_mul_fenced(a0, t0);
                if (full) {
                    a1 = fr29_mul_fenced(a1, t1);
                    a2 = fr29_mul_fenced(a2, t2);
                }
            }
        }
        // new[a] = sum_b mds[a][b] u[b]: three products < 2r added limb-wise (< 6r, limbs < 3 x 2^29); in a partial round a1 and
        // a2 are the lazy t1 and t2, legal first operands
        s0 = fr29_add(fr29_add(fr29_mul_fenced(a0, ps_row(tab, PS_MDS + 0)), fr29_mul_fenced(a1, ps_row(tab, PS_MDS + 1))),
                      fr29_mul_fenced(a2, ps_row(tab, PS_MDS + 2)));
        s1 = fr29_add(fr29_add(fr29_mul_fenced(a0, ps_row(tab, PS_MDS + 3)), fr29_mul_fenced(a1, ps_row(tab, PS_MDS + 4))),
                      fr29_mul_fenced(a2, ps_row(tab, PS_MDS + 5)));
        s2 = fr29_add(fr29_add(fr29_mul_fenced(a0, ps_row(tab, PS_MDS + 6)), fr29_mul_fenced(a1, ps_row(tab, PS_MDS + 7))),
                      fr29_mul_fenced(a2, ps_row(tab, PS_MDS + 8)));
    }
}

}  // namespace swm

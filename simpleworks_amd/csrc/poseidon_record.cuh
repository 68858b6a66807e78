// poseidon_record.cuh — the recording permutation: ps_permute (poseidon_permute.cuh) with a store after every square and every
// product of an S-box.  Shared by the witness of the hash circuit (poseidon_witness.hip) and of the membership circuit over a
// Poseidon tree (poseidon_tree_witness.hip).  What is recorded and its bounds: the head of poseidon_witness.hip.
#pragma once
#include "ff.cuh"
#include "fr29.cuh"
#include "poseidon.h"

namespace swm {

struct PwArgs {
    unsigned rows, half_full, partial, alpha, chain, n_out;
    size_t n_in, n_elems, count, num_witness, sponge_at;
    Fr29 to_std;  // 2^256 mod r, standard form: (v 2^261) x this = v 2^256, the prover's Montgomery form
};

// v 2^261 (normalised, < 2r) -> the 8 words of v 2^256 mod r at dst; `keep` is 0 for an item that is reported bad
__device__ __forceinline__ void pw_put(Fr* dst, const Fr29& v, const Fr29& to_std, bool act, uint32_t keep) {
    const Fr y = fr29_pack(fr29_canonical(fr29_mul_fenced(v, to_std), true));
    if (act) {
        uint4* p = reinterpret_cast<uint4*>(dst);
        p[0] = make_uint4(y.v[0] & keep, y.v[1] & keep, y.v[2] & keep, y.v[3] & keep);
        p[1] = make_uint4(y.v[4] & keep, y.v[5] & keep, y.v[6] & keep, y.v[7] & keep);
    }
}

// ps_permute, recording: the chain of S-box k of a round starts at wp + k * chain; wp moves past the round.
__device__ __forceinline__ void pw_permute(const uint32_t* tab, const PwArgs& A, int alpha_top, Fr29& s0, Fr29& s1, Fr29& s2, Fr*& wp,
                                           bool act, uint32_t keep) {
    const unsigned rounds = 2 * A.half_full + A.partial, m = A.chain;
#pragma unroll 1
    for (unsigned i = 0; i < rounds; i++) {
        const bool full = i < A.half_full || i >= A.half_full + A.partial;
        const unsigned k = PS_ARK + 3 * i;
        const Fr29 t0 = fr29_normalize(fr29_add(s0, ps_row(tab, k)));
        Fr29 t1 = fr29_add(s1, ps_row(tab, k + 1)), t2 = fr29_add(s2, ps_row(tab, k + 2));
        if (full) {
            t1 = fr29_normalize(t1);
            t2 = fr29_normalize(t2);
        }
        Fr29 a0 = t0, a1 = t1, a2 = t2;
        unsigned c = 0;  // position in the chain
#pragma unroll 1
        for (int b = alpha_top - 1; b >= 0; b--) {
            a0 = fr29_mul_fenced(a0, a0);
            pw_put(wp + c, a0, A.to_std, act, keep);
            if (full) {
                a1 = fr29_mul_fenced(a1, a1);
                pw_put(wp + m + c, a1, A.to_std, act, keep);
                a2 = fr29_mul_fenced(a2, a2);
                pw_put(wp + 2 * m + c, a2, A.to_std, act, keep);
            }
            c++;
            if ((A.alpha >> b) & 1u) {
                a0 = fr29_mul_fenced(a0, t0);
                pw_put(wp + c, a0, A.to_std, act, keep);
                if (full) {
                    a1 = fr29_mul_fenced(a1, t1);
                    pw_put(wp + m + c, a1, A.to_std, act, keep);
                    a2 = fr29_mul_fenced(a2, t2);
                    pw_put(wp + 2 * m + c, a2, A.to_std, act, keep);
                }
                c++;
            }
        }
        wp += full ? 3 * m : m;
        s0 = fr29_add(fr29_add(fr29_mul_fenced(a0, ps_row(tab, PS_MDS + 0)), fr29_mul_fenced(a1, ps_row(tab, PS_MDS + 1))),
                      fr29_mul_fenced(a2, ps_row(tab, PS_MDS + 2)));
        s1 = fr29_add(fr29_add(fr29_mul_fenced(a0, ps_row(tab, PS_MDS + 3)), fr29_mul_fenced(a1, ps_row(tab, PS_MDS + 4))),
                      fr29_mul_fenced(a2, ps_row(tab, PS_MDS + 5)));
        s2 = fr29_add(fr29_add(fr29_mul_fenced(a0, ps_row(tab, PS_MDS + 6)), fr29_mul_fenced(a1, ps_row(tab, PS_MDS + 7))),
                      fr29_mul_fenced(a2, ps_row(tab, PS_MDS + 8)));
    }
}

static void pw_std_limbs(const Fr& words, Fr29* out) {  // 8 words of a value < 2^256 -> 9 limbs of 29 bits
    for (int i = 0; i < 9; i++) {
        const int bit = 29 * i, wd = bit >> 5, off = bit & 31;
        uint64_t v = words.v[wd];
        if (wd + 1 < 8) v |= (uint64_t)words.v[wd + 1] << 32;
        out->l[i] = (uint32_t)(v >> off) & (i < 8 ? M29 : 0xFFFFFFFFu);
    }
}

}  // namespace swm

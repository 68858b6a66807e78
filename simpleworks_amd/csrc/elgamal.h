// elgamal.h — the resident forms of ElGamal parameters and of one recipient's key (elgamal.hip builds them; elgamal_witness.hip
// reads them).
#pragma once
#include <stdint.h>

struct swm_elgamal {
    void* d_table = nullptr;  // 32 x 256 rows (swm::EdRow): row (w, v) = v 2^(8 w) G
};
struct swm_elgamal_key {
    void* d_table = nullptr;  // the same of one public key
    uint8_t xy[64] = {0};     // the key as it was handed in: the instance of swm_elgamal_prove_to
};

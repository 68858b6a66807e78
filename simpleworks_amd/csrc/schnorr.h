// schnorr.h — the resident form of a Schnorr parameter set (schnorr.hip builds it; schnorr_witness.hip reads it).
#pragma once
#include <stdint.h>

struct swm_schnorr {
    void* d_table = nullptr;  // 32 x 256 rows (swm::EdRow): row (w, v) = v 2^(8 w) G
    uint32_t salt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool has_salt = false;
};

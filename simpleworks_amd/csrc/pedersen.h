// pedersen.h — the resident form of a Pedersen parameter set (pedersen.hip builds it; merkle_witness.hip reads it).
#pragma once

struct swm_pedersen {
    void* d_table = nullptr;  // num_windows x 2^window_size rows (swm::EdRow)
    unsigned num_windows = 0, window_size = 0;
};

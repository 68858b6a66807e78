// elgamal_shape_check.cpp — csrc/host/elgamal_shape.h under -fsanitize=address,undefined (tests/test_elgamal_circuit_host.py): the
// offset arithmetic of the ElGamal encryption circuit that csrc/elgamal_witness.hip writes witnesses by.  Stand-alone: no GPU, no
// library.  The circuit has one shape, so the numbers to hold the header to come from the caller: the twelve values of
// workloads.elgamal_circuit_layout() on the command line, in the order
//   key msg rnd fix dbl sel add sum out num_instance num_witness num_constraints
// Checks that the header states the same ones, that the witness groups tile the vector without gap or overlap, and that the rows
// are the witnesses' rows plus the ones the header names.  Prints "ok <num_instance> <num_witness> <num_constraints>".
#include <stdio.h>
#include <stdlib.h>

#include "host/elgamal_shape.h"

using namespace swm;

static void fail(const char* what, size_t got, size_t want) {
    fprintf(stderr, "elgamal_shape_check: %s: the header says %zu, expected %zu\n", what, got, want);
    exit(1);
}

int main(int argc, char** argv) {
    static const char* const names[] = {"key", "msg", "rnd", "fix", "dbl", "sel", "add", "sum", "out", "num_instance", "num_witness",
                                        "num_constraints"};
    const size_t n = sizeof(names) / sizeof(names[0]);
    if (argc != (int)n + 1) {
        fprintf(stderr, "usage: elgamal_shape_check key msg rnd fix dbl sel add sum out num_instance num_witness num_constraints\n");
        return 2;
    }
    const ElGamalShape s = elgamal_shape();
    const size_t got[] = {s.key_at, s.msg_at, s.rnd_at, s.fix_at, s.dbl_at, s.sel_at, s.add_at, s.sum_at, s.num_constraints - EW_OUT_ROWS,
                          s.num_instance, s.num_witness, s.num_constraints};
    for (size_t i = 0; i < n; i++) {
        char* end = nullptr;
        const unsigned long long want = strtoull(argv[i + 1], &end, 10);
        if (!end || *end || end == argv[i + 1]) {
            fprintf(stderr, "elgamal_shape_check: %s: not a number: %s\n", names[i], argv[i + 1]);
            return 2;
        }
        if (got[i] != (size_t)want) fail(names[i], got[i], (size_t)want);
    }
    // the groups tile the witness vector in order
    const size_t sizes[] = {EW_KEY_WITNESSES, EW_MSG_WITNESSES, EW_SCALAR_BITS, (EW_SCALAR_BITS - 1) * EW_FIX_STEP,
                            (EW_SCALAR_BITS - 1) * EW_DBL_STEP, EW_SCALAR_BITS * EW_SEL_STEP, (EW_SCALAR_BITS - 1) * EW_ADD_STEP, EW_ADD_STEP};
    size_t at = 0;
    for (size_t i = 0; i < 8; i++) {
        if (got[i] != at) fail(names[i], got[i], at);
        at += sizes[i];
    }
    if (at != s.num_witness) fail("num_witness", s.num_witness, at);
    // two squares and the on-curve row per point; a row per bit and per witness from fix on; the four comparisons
    const size_t rows = 3 + 3 + EW_SCALAR_BITS + (s.num_witness - s.fix_at) + EW_OUT_ROWS;
    if (rows != s.num_constraints) fail("num_constraints", s.num_constraints, rows);
    if (s.num_witness >= ((size_t)1 << 32)) fail("offsets leave 32 bits", s.num_witness, 0);
    printf("ok %zu %zu %zu\n", s.num_instance, s.num_witness, s.num_constraints);
    return 0;
}

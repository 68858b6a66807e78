// program_shape_check.cpp — csrc/host/program_shape.h under -fsanitize=address,undefined (tests/test_program_circuit_host.py builds
// and runs it): the validator and plan compiler that stand between a caller's bytes and the addresses the kernels of
// program_witness.hip compute.  Host only, no GPU.
//   argv[1]: a text file, one tape per line: "<hex tape> <num_instance> <num_witness> <num_constraints>".
// 1. Every tape is accepted with those counts and a plan that holds check_plan's invariants.
// 2. 10 000 seeded mutations of them (bytes overwritten, words swapped, tapes cut or extended): each is either refused, or accepted
//    with a plan that holds the same invariants.
// Prints "ok <tapes> <accepted mutations> <refused mutations>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "host/program_shape.h"

using namespace swm;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, what); \
            return false;                                                        \
        }                                                                        \
    } while (0)

// What the kernels rely on without checking.
static bool check_plan(const ProgramShape& s, const char* what) {
    CHECK(s.num_witness <= PG_MAX_WITNESS && s.instructions <= PG_MAX_INSTRUCTIONS);
    CHECK(s.exec.size() == s.instructions && s.witness_at.size() == s.instructions && s.row_at.size() == s.instructions);
    // the descriptors cover [0, num_witness) exactly once, in order
    size_t at = 0;
    for (const PgDesc& d : s.desc) {
        CHECK(d.at == at && d.count >= 1);
        CHECK(d.kind <= PG_DESC_FIELD);
        if (d.kind == PG_DESC_FIELD) CHECK(d.count == 1 && (size_t)d.slot + 1 < s.slots);
        else CHECK(d.count <= 128 && d.slot < s.slots);
        at += d.count;
    }
    CHECK(at == s.num_witness);
    // the per-block index: block k starts inside desc[block_first[k]]
    const size_t blocks = (s.num_witness + PG_BLOCK_WITNESSES - 1) / PG_BLOCK_WITNESSES;
    CHECK(s.block_first.size() == blocks + 1 && s.block_first[blocks] == s.desc.size());
    for (size_t k = 0; k < blocks; k++) {
        CHECK(s.block_first[k] < s.desc.size());
        const PgDesc& d = s.desc[s.block_first[k]];
        CHECK(d.at <= k * PG_BLOCK_WITNESSES && k * PG_BLOCK_WITNESSES < (size_t)d.at + d.count);
        CHECK(s.block_first[k] <= s.block_first[k + 1]);
        CHECK(s.block_first[k + 1] - s.block_first[k] <= PG_BLOCK_WITNESSES);  // what the expand kernel stages per block fits its LDS
    }
    // the instructions: slots in range and defined before they are read, offsets inside the item's bytes
    size_t slots = 0, witnesses = 0, rows = 0, eqs = 0;
    for (size_t k = 0; k < s.exec.size(); k++) {
        const PgExec& e = s.exec[k];
        CHECK(e.op >= 1 && e.op < PG_OPS && e.op != PG_ROTR);
        CHECK(e.width == 1 || e.width == 8 || e.width == 16 || e.width == 32 || e.width == 64 || e.width == 128);
        const PgCounts c = pg_op_counts(e.op, e.width);
        CHECK(e.dst == slots && s.witness_at[k] == witnesses && s.row_at[k] == rows);
        CHECK(e.a < (slots ? slots : 1) && e.b < (slots ? slots : 1) && e.c < (slots ? slots : 1));
        const size_t bytes = e.width == 1 ? 1 : e.width / 8;
        if (e.op == PG_INPUT_PUBLIC || e.op == PG_INPUT_PRIVATE) CHECK(e.imm_lo + bytes <= s.input_bytes);
        if (e.op == PG_OUTPUT) CHECK(e.imm_lo + bytes <= s.output_bytes);
        if (e.op == PG_SHL || e.op == PG_SHR) CHECK(e.imm_lo <= e.width);
        if (e.op == PG_ROTL) CHECK(e.imm_lo < e.width);
        if (e.op == PG_MUL || e.op == PG_DIV) CHECK(e.width <= 64);
        if (e.op == PG_EQ) {
            CHECK(eqs < s.eq_slots.size() && s.eq_slots[eqs] == e.dst);
            eqs++;
        }
        slots += c.slots;
        witnesses += c.witnesses;
        rows += c.rows;
    }
    CHECK(slots == s.slots && witnesses == s.num_witness && rows == s.num_constraints && eqs == s.eq_slots.size());
    CHECK(s.public_bytes <= s.input_bytes);
    size_t ni = 1;
    for (uint8_t t : s.public_types) ni += pg_width(t);
    for (uint8_t t : s.output_types) ni += pg_width(t);
    CHECK(ni == s.num_instance);
    return true;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::vector<std::vector<uint8_t>> tapes;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string hex;
        size_t ni, nw, nc;
        if (!(ls >> hex >> ni >> nw >> nc)) continue;
        std::vector<uint8_t> tape(hex.size() / 2);
        for (size_t i = 0; i < tape.size(); i++) tape[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
        ProgramShape s;
        const char* why = "";
        if (!program_shape(tape.data(), tape.size(), &s, &why)) {
            fprintf(stderr, "tape %zu refused: %s\n", tapes.size(), why);
            return 1;
        }
        if (s.num_instance != ni || s.num_witness != nw || s.num_constraints != nc) {
            fprintf(stderr, "tape %zu: counts %zu %zu %zu, expected %zu %zu %zu\n", tapes.size(), s.num_instance, s.num_witness,
                    s.num_constraints, ni, nw, nc);
            return 1;
        }
        if (!check_plan(s, "fixture")) return 1;
        tapes.push_back(tape);
    }
    if (tapes.empty()) return 2;
    // degenerate calls
    {
        ProgramShape s;
        const char* why = "";
        if (program_shape(nullptr, 0, &s, &why) || program_shape(tapes[0].data(), 0, &s, &why) || program_shape(tapes[0].data(), 31, &s, nullptr))
            return 1;
    }
    size_t accepted = 0, refused = 0;
    for (int round = 0; round < 10000; round++) {
        // each mutant lives in an allocation of exactly its size: a read past the end is an ASan report
        std::vector<uint8_t> t = tapes[next() % tapes.size()];
        const unsigned kind = (unsigned)(next() % 8);
        const size_t words = t.size() / PG_WORD;
        if (kind == 0 && t.size() > 1) {
            t.resize(next() % t.size());  // cut
        } else if (kind == 1) {
            t.resize(t.size() + 1 + next() % 64, (uint8_t)next());  // extended
        } else if (kind == 2 && words > 2) {  // two instruction words swapped
            const size_t a = 1 + next() % (words - 1), b = 1 + next() % (words - 1);
            for (size_t j = 0; j < PG_WORD; j++) std::swap(t[PG_WORD * a + j], t[PG_WORD * b + j]);
        } else if (kind == 3) {  // the count field
            t[8 + next() % 4] = (uint8_t)next();
        } else {  // one to three bytes of an instruction's op, type and operand fields, or anywhere
            const unsigned n = 1 + (unsigned)(next() % 3);
            for (unsigned j = 0; j < n && words > 1; j++) {
                const size_t w = 1 + next() % (words - 1);
                const size_t off = kind < 7 ? next() % 8 : next() % PG_WORD;
                const uint64_t v = next();
                t[PG_WORD * w + off] = (uint8_t)(v & 1 ? v >> 8 & 31 : v >> 8);  // small values hit valid codes and registers more often
            }
        }
        std::vector<uint8_t> exact(t.begin(), t.end());
        exact.shrink_to_fit();
        ProgramShape s;
        const char* why = "";
        if (program_shape(exact.data(), exact.size(), &s, &why)) {
            if (!check_plan(s, "mutant")) {
                fprintf(stderr, "round %d\n", round);
                return 1;
            }
            accepted++;
        } else {
            if (!why || !*why) return 1;
            refused++;
        }
    }
    printf("ok %zu %zu %zu\n", tapes.size(), accepted, refused);
    return 0;
}

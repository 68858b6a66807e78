// program_shape.h — integer PROGRAMS (simpleworks_amd/workloads.py, build_program): the validator of a tape, the shape of the
// circuit it denotes and the compiled PLAN the kernels of program_witness.hip read.  Plain C++, no GPU headers, no library state:
// shared by host_abi.inc (swm_program_circuit_shape), by program_witness.hip and by tests/native/program_shape_check.cpp.  This is
// what stands between a caller's bytes and a kernel's addresses: the kernels check no index.
//
// The tape, version "SWMPROG1": a 32-byte header — the magic, the instruction count as a little-endian u32, 20 zero bytes — and
// one 32-byte word per instruction:
//   [0] op   [1] type   [2:4] a   [4:6] b   [6:8] c  (register indices, little-endian)   [8:16] zero   [16:32] immediate, little-endian
// Types BOOL, U8, U16, U32, U64, U128 = 0 .. 5.  A register is defined once: inputs come first, public then private, and every later
// instruction but ASSERT_EQ and OUTPUT defines the next register.  `type` is the type of the operands; GT .. EQ give a BOOL.
//   INPUT_PUBLIC INPUT_PRIVATE   -> T           the next value of the item's input bytes (BOOL: bit 0 of a byte)
//   CONST                        imm -> T       imm < 2^W
//   AND OR XOR NAND NOR          T, T -> T      BitwiseOperationGadget (traits.rs), BOOL included
//   NOT                          T -> T
//   ADD SUB MUL DIV              U, U -> U      ADD, MUL wrapping (uint8.rs:237-271, :332-343); SUB underflow (:277) is status bit 0,
//                                               a zero divisor (:305) status bit 1
//   SHL SHR ROTL ROTR            U, imm -> U    imm < 2^32; shifts of >= W positions give 0 (uint64.rs:195, :247), rotations are mod W
//   GT GTE LT LTE                U, U -> BOOL   ComparisonGadget
//   EQ                           T, T -> BOOL   is_eq
//   SELECT                       BOOL a, T b, T c -> T     a ? b : c (conditionally_select)
//   ASSERT_EQ                    T, T           enforce_equal (examples/test-circuit.rs:22); a failure is status bit 2
//   OUTPUT                       T              publishes the register
// Unused operand fields and immediates are zero.  Refused (out of scope): MUL and DIV on U128 — the 256-bit product does not fit
// the 253-bit field — and everything the codes above do not name: Int8, Address, FieldGadget, the byte conversions.
// Limits: PG_MAX_INSTRUCTIONS = 4096 instructions, register indices in 16 bits, PG_MAX_WITNESS = 2^20 witnesses per item.
// (4096 instructions cannot reach 2^20 witnesses — the widest op, DIV on U64, has 192 — but the bound is what the 32-bit offsets of the
// plan rest on, so it is checked where it is stated and not left to that arithmetic.)
//
// The circuit's layout per op (witnesses, rows; W the width) is the block comment of build_program; pg_op_counts states it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

namespace swm {

static constexpr size_t PG_WORD = 32;
static constexpr size_t PG_MAX_INSTRUCTIONS = 4096;
static constexpr size_t PG_MAX_WITNESS = (size_t)1 << 20;
static constexpr unsigned PG_BLOCK_WITNESSES = 128;  // what one workgroup of the expand kernel writes: 256 lanes x 16 bytes

enum PgType : uint8_t { PG_BOOL = 0, PG_U8, PG_U16, PG_U32, PG_U64, PG_U128, PG_TYPES };
enum PgOp : uint8_t {
    PG_INPUT_PUBLIC = 1, PG_INPUT_PRIVATE, PG_CONST, PG_AND, PG_OR, PG_XOR, PG_NAND, PG_NOR, PG_NOT, PG_ADD, PG_SUB, PG_MUL, PG_DIV, PG_SHL,
    PG_SHR, PG_ROTL, PG_ROTR, PG_GT, PG_GTE, PG_LT, PG_LTE, PG_EQ, PG_SELECT, PG_ASSERT_EQ, PG_OUTPUT, PG_OPS
};
enum : uint8_t { PG_STATUS_UNDERFLOW = 1, PG_STATUS_DIV_ZERO = 2, PG_STATUS_ASSERT = 4 };

inline unsigned pg_width(unsigned type) { return type == PG_BOOL ? 1u : 4u << type; }
inline unsigned pg_bytes(unsigned type) { return type == PG_BOOL ? 1u : (4u << type) / 8u; }

// What the kernels read.  One PgExec per instruction: operands and results are SLOTS of the value trace, never registers.  An
// instruction owns `slots` consecutive slots from dst on: its register first, then its auxiliary values —
//   ADD sum, carry | MUL low, high | DIV q, rem, b - 1 - rem | GT .. LTE answer, the low W bits of the sum | EQ answer, inverse (2:
// the exec kernel leaves |a - b| and its sign there, the inversion kernel replaces them)
// imm: the constant; the byte offset of an INPUT in the item's inputs, of an OUTPUT in its outputs; the positions of a shift, already
// clipped to W; of a rotation, already as a left rotation below W (PG_ROTR never reaches the kernel).
struct PgExec {
    uint32_t op, width, a, b, c, dst;
    uint64_t imm_lo, imm_hi;
};
// A run of `count` consecutive witnesses from `at` on: bits 0 .. count - 1 of slot `slot` (PG_DESC_BITS), their complements
// (PG_DESC_NBITS: the witness behind a NAND, NOR, GTE or LTE register), or one field element in slots slot, slot + 1 (PG_DESC_FIELD).
enum : uint32_t { PG_DESC_BITS = 0, PG_DESC_NBITS = 1, PG_DESC_FIELD = 2 };
struct PgDesc {
    uint32_t at, slot, count, kind;
};

struct ProgramShape {
    size_t num_instance = 0, num_witness = 0, num_constraints = 0;
    size_t instructions = 0, registers = 0, slots = 0;
    size_t input_bytes = 0, public_bytes = 0, output_bytes = 0;  // per item; the public inputs are the first public_bytes
    std::vector<uint32_t> witness_at, row_at;                    // per instruction
    std::vector<uint8_t> public_types, output_types;             // declaration / OUTPUT order: what the instance is built from
    std::vector<PgExec> exec;
    std::vector<PgDesc> desc;
    std::vector<uint32_t> eq_slots;     // the first slot of every EQ instruction: what the inversion kernel walks
    std::vector<uint32_t> block_first;  // block k of PG_BLOCK_WITNESSES witnesses starts in desc[block_first[k]]; one entry past the end
};

struct PgCounts {
    unsigned witnesses, rows, slots;
};
// The per-op formulas.  (INPUT_PUBLIC and OUTPUT add W instance variables.)
inline PgCounts pg_op_counts(unsigned op, unsigned W) {
    switch (op) {
        case PG_INPUT_PUBLIC: return {0, 0, 1};
        case PG_INPUT_PRIVATE: return {W, W, 1};
        case PG_CONST: case PG_NOT: case PG_SHL: case PG_SHR: case PG_ROTL: case PG_ROTR: return {0, 0, 1};
        case PG_AND: case PG_OR: case PG_XOR: case PG_NAND: case PG_NOR: case PG_SELECT: return {W, W, 1};
        case PG_ADD: return {W + 1, W + 2, 2};
        case PG_SUB: return {W, W + 1, 1};
        case PG_MUL: return {2 * W, 2 * W + 1, 2};
        case PG_DIV: return {3 * W, 3 * W + 2, 3};
        case PG_GT: case PG_GTE: case PG_LT: case PG_LTE: return {W + 1, W + 2, 2};
        case PG_EQ: return {2, 2, 3};
        case PG_ASSERT_EQ: case PG_OUTPUT: return {0, W, 0};
    }
    return {0, 0, 0};
}

inline uint32_t pg_u16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint64_t pg_u64(const uint8_t* p) {
    uint64_t v = 0;
    for (int k = 0; k < 8; k++) v |= (uint64_t)p[k] << (8 * k);
    return v;
}

// Validates `len` bytes of tape and compiles them.  false (and *why, a static string): anything the header comment does not allow.
// Nothing is read past tape + len, and nothing is computed from a field before it has been checked.
inline bool program_shape(const uint8_t* tape, size_t len, ProgramShape* out, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    *why = "no tape header";
    if (!tape || len < PG_WORD || memcmp(tape, "SWMPROG1", 8) != 0) return false;
    for (size_t k = 12; k < PG_WORD; k++)
        if (tape[k]) return false;
    const size_t n = (size_t)tape[8] | (size_t)tape[9] << 8 | (size_t)tape[10] << 16 | (size_t)tape[11] << 24;
    *why = "the instruction count (at most 4096) does not match the length";
    if (n > PG_MAX_INSTRUCTIONS || len != PG_WORD * (1 + n)) return false;

    ProgramShape s;
    s.instructions = n;
    s.num_instance = 1;
    std::vector<uint8_t> reg_type;
    std::vector<uint32_t> reg_slot;
    unsigned phase = 0;
    for (size_t k = 0; k < n; k++) {
        const uint8_t* w = tape + PG_WORD * (1 + k);
        const unsigned op = w[0], type = w[1];
        const uint32_t r[3] = {pg_u16(w + 2), pg_u16(w + 4), pg_u16(w + 6)};
        const uint64_t imm_lo = pg_u64(w + 16), imm_hi = pg_u64(w + 24);
        *why = "an unknown op or type, or a reserved byte that is set";
        if (op < 1 || op >= PG_OPS || type >= PG_TYPES || pg_u64(w + 8)) return false;
        const unsigned W = pg_width(type);
        // operand types per op: how many registers it reads and of which type (t: the instruction's type, b: BOOL)
        unsigned reads = 0;
        uint8_t want[3] = {(uint8_t)type, (uint8_t)type, (uint8_t)type};
        bool has_imm = false, defines = true;
        switch (op) {
            case PG_INPUT_PUBLIC: case PG_INPUT_PRIVATE: {
                const unsigned now = op == PG_INPUT_PUBLIC ? 1 : 2;
                *why = "inputs come first, public then private";
                if (now < phase) return false;
                phase = now;
                break;
            }
            case PG_CONST:
                has_imm = true;
                *why = "a constant wider than its type";
                if (W < 64 ? (imm_hi || imm_lo >> W) : W == 64 ? imm_hi != 0 : false) return false;
                break;
            case PG_NOT: reads = 1; break;
            case PG_AND: case PG_OR: case PG_XOR: case PG_NAND: case PG_NOR: case PG_EQ: reads = 2; break;
            case PG_ADD: case PG_SUB: case PG_MUL: case PG_DIV: case PG_GT: case PG_GTE: case PG_LT: case PG_LTE:
                reads = 2;
                *why = "arithmetic or a comparison on BOOL";
                if (type == PG_BOOL) return false;
                *why = "MUL and DIV on U128 are out of scope";
                if (type == PG_U128 && (op == PG_MUL || op == PG_DIV)) return false;
                break;
            case PG_SHL: case PG_SHR: case PG_ROTL: case PG_ROTR:
                reads = 1;
                has_imm = true;
                *why = "a shift on BOOL, or by 2^32 positions or more";
                if (type == PG_BOOL || imm_hi || imm_lo >> 32) return false;
                break;
            case PG_SELECT:
                reads = 3;
                want[0] = PG_BOOL;
                break;
            case PG_ASSERT_EQ: reads = 2; defines = false; break;
            case PG_OUTPUT: reads = 1; defines = false; break;
        }
        if (op > PG_INPUT_PRIVATE) phase = 3;
        *why = "an immediate where the op takes none";
        if (!has_imm && (imm_lo || imm_hi)) return false;
        *why = "an operand that is no earlier register of the right type, or an unused operand field that is set";
        for (unsigned j = 0; j < 3; j++) {
            if (j < reads ? (r[j] >= reg_type.size() || reg_type[r[j]] != want[j]) : r[j] != 0) return false;
        }
        const PgCounts cnt = pg_op_counts(op, W);

        PgExec e = {};
        e.op = op;
        e.width = W;
        e.a = reads > 0 ? reg_slot[r[0]] : 0;
        e.b = reads > 1 ? reg_slot[r[1]] : 0;
        e.c = reads > 2 ? reg_slot[r[2]] : 0;
        e.dst = (uint32_t)s.slots;
        e.imm_lo = imm_lo;
        e.imm_hi = imm_hi;
        if (op == PG_INPUT_PUBLIC || op == PG_INPUT_PRIVATE) {
            e.imm_lo = s.input_bytes;
            s.input_bytes += pg_bytes(type);
            if (op == PG_INPUT_PUBLIC) {
                s.public_bytes += pg_bytes(type);
                s.public_types.push_back((uint8_t)type);
                s.num_instance += W;
            }
        } else if (op == PG_OUTPUT) {
            e.imm_lo = s.output_bytes;
            s.output_bytes += pg_bytes(type);
            s.output_types.push_back((uint8_t)type);
            s.num_instance += W;
        } else if (op == PG_SHL || op == PG_SHR) {
            e.imm_lo = imm_lo < W ? imm_lo : W;
        } else if (op == PG_ROTL) {
            e.imm_lo = imm_lo % W;
        } else if (op == PG_ROTR) {
            e.op = PG_ROTL;
            e.imm_lo = (W - imm_lo % W) % W;
        }
        s.exec.push_back(e);

        // the witnesses of this instruction, in the order build_program allocates them
        s.witness_at.push_back((uint32_t)s.num_witness);
        s.row_at.push_back((uint32_t)s.num_constraints);
        const uint32_t at = (uint32_t)s.num_witness, d = e.dst;
        switch (op) {
            case PG_INPUT_PRIVATE: case PG_AND: case PG_OR: case PG_XOR: case PG_SUB: case PG_SELECT:
                s.desc.push_back({at, d, W, PG_DESC_BITS});
                break;
            case PG_NAND: case PG_NOR: s.desc.push_back({at, d, W, PG_DESC_NBITS}); break;
            case PG_ADD:
                s.desc.push_back({at, d, W, PG_DESC_BITS});
                s.desc.push_back({at + W, d + 1, 1, PG_DESC_BITS});
                break;
            case PG_MUL:
                s.desc.push_back({at, d, W, PG_DESC_BITS});
                s.desc.push_back({at + W, d + 1, W, PG_DESC_BITS});
                break;
            case PG_DIV:
                for (uint32_t j = 0; j < 3; j++) s.desc.push_back({at + j * W, d + j, W, PG_DESC_BITS});
                break;
            case PG_GT: case PG_GTE: case PG_LT: case PG_LTE:
                s.desc.push_back({at, d + 1, W, PG_DESC_BITS});
                s.desc.push_back({at + W, d, 1, (op == PG_GT || op == PG_LT) ? PG_DESC_BITS : PG_DESC_NBITS});
                break;
            case PG_EQ:
                s.eq_slots.push_back(d);
                s.desc.push_back({at, d + 1, 1, PG_DESC_FIELD});
                s.desc.push_back({at + 1, d, 1, PG_DESC_BITS});
                break;
            default: break;
        }
        s.num_witness += cnt.witnesses;
        s.num_constraints += cnt.rows;
        s.slots += cnt.slots;
        *why = "more than 2^20 witnesses per item";
        if (s.num_witness > PG_MAX_WITNESS) return false;
        if (defines) {
            reg_type.push_back(op >= PG_GT && op <= PG_EQ ? (uint8_t)PG_BOOL : (uint8_t)type);
            reg_slot.push_back(e.dst);
        }
    }
    s.registers = reg_type.size();
    // the per-block index of the expand kernel
    size_t dsc = 0;
    for (size_t at = 0; at < s.num_witness; at += PG_BLOCK_WITNESSES) {
        while (s.desc[dsc].at + s.desc[dsc].count <= at) dsc++;
        s.block_first.push_back((uint32_t)dsc);
    }
    s.block_first.push_back((uint32_t)s.desc.size());
    *why = "";
    *out = std::move(s);
    return true;
}

}  // namespace swm

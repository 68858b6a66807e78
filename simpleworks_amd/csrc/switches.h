// switches.h — the ONE place libswmarlin.so reads its environment ("geometry knobs nobody tests are a way to get
// wrong commitments from a typo").
//
// Every variable the library reads is one row of SWITCHES below: its name, its kind (with range and default), its class and when
// it is read.  The rest of csrc/ reads through sw() / sw_path() with the row's enum, so a switch that is not declared does not
// compile; tests/test_switch_audit.py parses the rows and holds its class sets, tests/test_gpu_switches.py and the source to them.
// An integer that does not parse, or lies outside its row's range, is REFUSED — one line on stderr and the default is used — it is
// never clamped into a geometry nobody asked for.  switch_fingerprint() is what the ranks of a sharded proof compare.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <mutex>

namespace swm {

// ---- parsing primitives (used by the table's accessors below and by nothing else in csrc/)
// NAME as an integer in [lo, hi]; unset or empty: def.
inline long env_switch(const char* name, long def, long lo, long hi) {
    const char* e = getenv(name);
    if (!e || !*e) return def;
    char* end = nullptr;
    errno = 0;
    const long v = strtol(e, &end, 0);
    if (errno != 0 || end == e || *end != '\0' || v < lo || v > hi) {
        fprintf(stderr, "[swm] %s=%s refused (an integer in [%ld, %ld] is expected): using the default %ld\n", name, e, lo, hi, def);
        return def;
    }
    return v;
}
// set to anything but "" / "0"
inline bool env_flag(const char* name) {
    const char* e = getenv(name);
    return e && *e && !(e[0] == '0' && e[1] == '\0');
}
// a path; nullptr when unset or empty
inline const char* env_path(const char* name) {
    const char* e = getenv(name);
    return e && *e ? e : nullptr;
}

// ---- the table
enum SwKind {
    K_INT,   // integer in [lo, hi], default def
    K_OPT,   // the same, but def lies OUTSIDE [lo, hi] and means "not set": the call site then takes a value of its own
    K_FLAG,  // 1 when set to anything but "" / "0", else 0
    K_FILE,  // a path, read with sw_path()
};
enum SwClass {
    C_PATH,        // selects between maintained paths of the product; exercised for golden proof bytes by tests/test_gpu_switches.py
    C_SHARDING,    // how one proof is split over ranks; exercised by the sharded-prover tests
    C_DIAGNOSTIC,  // cannot change a result
    C_HOOK,        // measurement hook (wrong proofs by construction): only under -DSWM_MEASURE_HOOKS, in the second library that
                   // tools/ubench/shard_emulate.py builds — no switch of the shipped library can make a proof wrong with status 0
};
enum SwWhen {
    W_ONCE,  // parsed at first use and cached for the process
    W_LIVE,  // read at every use (tests flip these inside one process)
};
enum Switch {
    SW_MSM_TABLE_C, SW_MSM_TE, SW_MSM_NO_TABLE, SW_MSM_QUAD, SW_MSM_LOW, SW_MSM_TWIN, SW_MSM_BATCH_BELOW,
    SW_PROVE_ONE_STREAM_LOG, SW_MASK_PIECES, SW_NTT_LAZY, SW_NTT_PASS_TABLES, SW_RALPHA_TRANSFORMS, SW_SAMPLE_TIGHT,
    SW_SHARD_FORCE, SW_SHARD_RANGE, SW_SHARD_BUCKETS, SW_SHARD_BLOCK_LOG, SW_SHARD_R1_OFF, SW_SHARD_R2_OFF,
    SW_TRACE, SW_PROOF_MARKS, SW_POOL_WORKERS, SW_POOL_SPIN_US, SW_LOCAL_WORLD_SIZE, SW_RCCL_PATH,
#ifdef SWM_MEASURE_HOOKS
    SW_SHARD_EMULATE,
#endif  // SWM_MEASURE_HOOKS
    SW_COUNT
};
struct SwitchDecl {
    Switch id; const char* name; SwKind kind; long def, lo, hi; SwClass cls; SwWhen when;
};
constexpr SwitchDecl SWITCHES[] = {
    // MSM (msm.hip and its units: msm_sort.hip, msm_table.hip, msm_stages.hip)
    {SW_MSM_TABLE_C, "SWM_MSM_TABLE_C", K_OPT, 0, 8, 22, C_PATH, W_ONCE},       // one table width for every base set; 0: the width rule decides
    {SW_MSM_TE, "SWM_MSM_TE", K_INT, 1, 0, 1, C_PATH, W_ONCE},                  // 0: XYZZ tables everywhere (the form of sets outside the subgroup)
    {SW_MSM_NO_TABLE, "SWM_MSM_NO_TABLE", K_FLAG, 0, 0, 1, C_PATH, W_ONCE},     // the per-window schedule for every set (what table-less sets run)
    {SW_MSM_QUAD, "SWM_MSM_QUAD", K_INT, 1, 0, 1, C_PATH, W_ONCE},              // 0: small MSMs with one lane per chain / per segment
    {SW_MSM_LOW, "SWM_MSM_LOW", K_INT, 2, 0, 2, C_PATH, W_ONCE},                // the low-LDS bucket stage: 0 nowhere, 1 everywhere, 2 in joint stages
    {SW_MSM_TWIN, "SWM_MSM_TWIN", K_INT, 1, 0, 1, C_PATH, W_ONCE},              // 0: the shifted commitment of a pair sorts for itself
    // points below which a job's bucket stage joins its round's joint launch; -1 (outside the range): not set, the table form's own bound
    {SW_MSM_BATCH_BELOW, "SWM_MSM_BATCH_BELOW", K_OPT, -1, 0, 1L << 31, C_PATH, W_ONCE},
    // prover (marlin_prove.hip, ntt.hip, devops.cuh)
    {SW_PROVE_ONE_STREAM_LOG, "SWM_PROVE_ONE_STREAM_LOG", K_INT, 19, 0, 47, C_PATH, W_ONCE},  // proofs below 2^this constraints: one stream per lane
    {SW_MASK_PIECES, "SWM_MASK_PIECES", K_INT, 3, 1, 3, C_PATH, W_ONCE},        // caller-owned generator: the mask commitment in this many pieces
    {SW_NTT_LAZY, "SWM_NTT_LAZY", K_INT, 1, 0, 1, C_PATH, W_ONCE},              // 0: the 8 x 32-bit transform instead of the 9 x 29-bit lazy one
    {SW_NTT_PASS_TABLES, "SWM_NTT_PASS_TABLES", K_INT, 1, 0, 1, C_PATH, W_ONCE},  // 0: twiddles from the two-level tables
    {SW_RALPHA_TRANSFORMS, "SWM_RALPHA_TRANSFORMS", K_FLAG, 0, 0, 1, C_PATH, W_LIVE},  // r(alpha, X) by two transforms (the closed form's 2^-231 case)
    {SW_SAMPLE_TIGHT, "SWM_SAMPLE_TIGHT", K_FLAG, 0, 0, 1, C_PATH, W_LIVE},     // the bulk sampler draws no spare candidates: its retry branch runs
    // one proof over several ranks (marlin_commit.hip, marlin_prove.hip, capi.hip)
    {SW_SHARD_FORCE, "SWM_SHARD_FORCE", K_FLAG, 0, 0, 1, C_SHARDING, W_LIVE},   // test hook: the exchange path with a world of one
    {SW_SHARD_RANGE, "SWM_SHARD_RANGE", K_FLAG, 0, 0, 1, C_SHARDING, W_LIVE},   // commitments split by point range
    {SW_SHARD_BUCKETS, "SWM_SHARD_BUCKETS", K_FLAG, 0, 0, 1, C_SHARDING, W_LIVE},  // ... by bucket range
    {SW_SHARD_BLOCK_LOG, "SWM_SHARD_BLOCK_LOG", K_INT, 12, 0, 20, C_SHARDING, W_LIVE},  // log2 of the block of the block-cyclic split
    {SW_SHARD_R1_OFF, "SWM_SHARD_R1_OFF", K_FLAG, 0, 0, 1, C_SHARDING, W_LIVE},  // round 1's transforms whole on every rank
    {SW_SHARD_R2_OFF, "SWM_SHARD_R2_OFF", K_FLAG, 0, 0, 1, C_SHARDING, W_LIVE},  // rounds 2 and 3 likewise
    // diagnostics
    {SW_TRACE, "SWM_TRACE", K_INT, 0, 0, 2, C_DIAGNOSTIC, W_ONCE},              // 1: phases (synchronising), MSM shapes, allocations; 2: host timestamps only
    {SW_PROOF_MARKS, "SWM_PROOF_MARKS", K_FLAG, 0, 0, 1, C_DIAGNOSTIC, W_ONCE},  // a marker kernel at the start of each proof, for kernel traces
    {SW_POOL_WORKERS, "SWM_POOL_WORKERS", K_OPT, -1, 0, 64, C_DIAGNOSTIC, W_LIVE},  // the host fold's worker threads; -1: the process's share of the cores
    {SW_POOL_SPIN_US, "SWM_POOL_SPIN_US", K_INT, 1500, 0, 100000, C_DIAGNOSTIC, W_ONCE},  // how long they poll for a fold (0: they sleep)
    {SW_LOCAL_WORLD_SIZE, "LOCAL_WORLD_SIZE", K_INT, 1, 1, 4096, C_DIAGNOSTIC, W_LIVE},  // torchrun's: ranks that share this host's cores
    {SW_RCCL_PATH, "SWM_RCCL_PATH", K_FILE, 0, 0, 0, C_DIAGNOSTIC, W_LIVE},     // that librccl or nothing (its one reader runs once per process)
#ifdef SWM_MEASURE_HOOKS
    {SW_SHARD_EMULATE, "SWM_SHARD_EMULATE", K_FLAG, 0, 0, 1, C_HOOK, W_ONCE},   // device exchanges answered with the rank's own data
#endif  // SWM_MEASURE_HOOKS
};
constexpr bool switches_ok() {
    if (sizeof(SWITCHES) / sizeof(SWITCHES[0]) != SW_COUNT) return false;
    for (int s = 0; s < SW_COUNT; s++) {
        const SwitchDecl& d = SWITCHES[s];
        const bool def_in_range = d.lo <= d.def && d.def <= d.hi;
        if (d.id != s || (d.kind == K_INT && !def_in_range) || (d.kind == K_OPT && def_in_range)) return false;
    }
    return true;
}
static_assert(switches_ok(), "SWITCHES: one row per enumerator, in its order; K_INT defaults inside their range, K_OPT defaults outside");

// ---- the accessors
inline long sw_parse(const SwitchDecl& d) { return d.kind == K_FLAG ? (long)env_flag(d.name) : env_switch(d.name, d.def, d.lo, d.hi); }
// the effective value of an integer or flag row
inline long sw(Switch s) {
    const SwitchDecl& d = SWITCHES[s];
    if (d.when == W_LIVE) return sw_parse(d);
    static std::once_flag once[SW_COUNT];
    static long cached[SW_COUNT];
    std::call_once(once[s], [&] { cached[s] = sw_parse(d); });
    return cached[s];
}
inline const char* sw_path(Switch s) { return env_path(SWITCHES[s].name); }

// What two ranks of one proof must agree on: 32-bit FNV-1a over (name, effective value) of every C_PATH and C_SHARDING row, in
// table order — decisions, not text: an unset switch, its default spelled out, another spelling of the same number and a refused
// value all hash alike.  Diagnostics, hooks and paths do not enter.  Needs no GPU.
inline uint32_t switch_fingerprint() {
    uint32_t h = 2166136261u;
    for (int s = 0; s < SW_COUNT; s++) {
        const SwitchDecl& d = SWITCHES[s];
        if (d.cls != C_PATH && d.cls != C_SHARDING) continue;
        for (const char* p = d.name; *p; p++) h = (h ^ (uint8_t)*p) * 16777619u;
        const uint64_t v = (uint64_t)sw((Switch)s);
        for (int i = 0; i < 64; i += 8) h = (h ^ (uint8_t)(v >> i)) * 16777619u;
    }
    return h;
}

}  // namespace swm

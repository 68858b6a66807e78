"""csrc/ reads its environment in ONE place (csrc/switches.h), through ONE table of declared switches, and every switch in it is
either exercised for golden proof bytes by tests/test_gpu_switches.py or is a declared diagnostic that cannot change a result
(VERDICT r05 "next" #5).  CPU only: a source audit, and host programs compiled against the shipped header."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simpleworks_amd", "csrc")

# switches that cannot change what a call returns: traces, kernel-trace delimiters, host-thread counts, which librccl is loaded
DIAGNOSTICS = {"SWM_TRACE", "SWM_PROOF_MARKS", "SWM_POOL_WORKERS", "SWM_POOL_SPIN_US", "SWM_RCCL_PATH", "LOCAL_WORLD_SIZE"}
# exercised by the sharded-prover tests (tests/test_gpu_marlin.py, tests/test_gpu_multi.py, tests/test_dist.py), not by the switch test
SHARDING = {"SWM_SHARD_RANGE", "SWM_SHARD_BUCKETS", "SWM_SHARD_BLOCK_LOG", "SWM_SHARD_R1_OFF", "SWM_SHARD_R2_OFF", "SWM_SHARD_FORCE"}
# compiled only with -DSWM_MEASURE_HOOKS (tools/ubench/shard_emulate.py builds that second library); never in the shipped one
MEASURE_HOOKS = {"SWM_SHARD_EMULATE"}


def _sources():
    for dirpath, _, files in os.walk(CSRC):
        if os.path.basename(dirpath) == "build":
            continue
        for f in files:
            if f.endswith((".hip", ".cuh", ".h", ".inc", ".cpp")):
                yield os.path.join(dirpath, f)


ROW = re.compile(r'\{\s*(SW_[A-Z0-9_]+),\s*"([A-Z0-9_]+)",\s*(K_[A-Z]+),\s*([^,{}]+),\s*([^,{}]+),\s*([^,{}]+),\s*(C_[A-Z]+),\s*(W_[A-Z]+)\s*\}')


def _read_switches():
    """The rows of SWITCHES in csrc/switches.h by name: id, kind, cls, when, and the files that read the row through sw() / sw_path()."""
    rows = {}
    for m in ROW.finditer(open(os.path.join(CSRC, "switches.h")).read()):
        assert m.group(2) not in rows, "%s is declared twice" % m.group(2)
        rows[m.group(2)] = {"id": m.group(1), "kind": m.group(3), "cls": m.group(7), "when": m.group(8), "where": set()}
    for path in _sources():
        if os.path.basename(path) == "switches.h":
            continue
        text = open(path, errors="replace").read()
        for row in rows.values():
            if re.search(r"\bsw(?:_path)?\(\s*(?:swm::)?%s\s*\)" % row["id"], text):
                row["where"].add(os.path.relpath(path, CSRC))
    return rows


def _of_class(rows, cls):
    return {name for name, row in rows.items() if row["cls"] == cls}


def test_getenv_only_in_switches_h():
    """Outside switches.h nothing under csrc/ touches the environment: no getenv / secure_getenv, no walk of `environ`, and no call
    of the parsing primitives — every read goes through the table's accessors."""
    forbidden = (r"\bgetenv\s*\(", r"\bsecure_getenv\b", r"\benviron\b", r"\benv_switch\s*\(", r"\benv_flag\s*\(", r"\benv_path\s*\(")
    offenders = []
    for path in _sources():
        if os.path.basename(path) == "switches.h":
            continue
        text = re.sub(r"//[^\n]*", "", open(path, errors="replace").read())
        offenders += [(os.path.relpath(path, CSRC), pat) for pat in forbidden if re.search(pat, text)]
    assert not offenders, "the environment is read outside csrc/switches.h: %s" % offenders
    n = len(re.findall(r"\bgetenv\s*\(", open(os.path.join(CSRC, "switches.h")).read()))
    assert 1 <= n <= 4, n   # (r05: 95 getenv calls over seven files)


def test_every_switch_is_tested_or_a_declared_diagnostic():
    import test_gpu_switches as T
    tested = set()
    for env in T.SETTINGS:
        tested |= set(env)
    read = _read_switches()
    assert len(read) >= 15, read
    for name, row in sorted(read.items()):
        assert name in tested or name in DIAGNOSTICS or name in SHARDING or name in MEASURE_HOOKS, \
            "%s is declared in csrc/switches.h but neither exercised by tests/test_gpu_switches.py nor a declared diagnostic" % name
        assert row["where"], "%s is declared in csrc/switches.h and read nowhere" % name
    for name in tested:
        assert name in read, "tests/test_gpu_switches.py sets %s, which the library no longer reads" % name
    # the table's classes are this file's sets, and its PATH rows are what tests/test_gpu_switches.py sets
    assert _of_class(read, "C_PATH") == tested
    assert _of_class(read, "C_DIAGNOSTIC") == DIAGNOSTICS
    assert _of_class(read, "C_SHARDING") == SHARDING
    assert _of_class(read, "C_HOOK") == MEASURE_HOOKS
    assert set(read) == tested | DIAGNOSTICS | SHARDING | MEASURE_HOOKS
    # the sharding switches are referenced by the sharded-prover tests
    body = "".join(open(os.path.join(ROOT, "tests", f)).read() for f in ("test_gpu_marlin.py", "test_gpu_multi.py", "test_dist.py"))
    for name in SHARDING:
        assert name in body, "%s: no sharded-prover test sets it" % name


def test_measurement_hook_is_not_in_the_shipped_library():
    """SWM_SHARD_EMULATE answers exchanges with the rank's own data (wrong proofs by construction): its row, its enumerator and its
    reads sit between #ifdef SWM_MEASURE_HOOKS / #endif, the Makefile does not define that macro, and the built library does not
    contain the name."""
    for path in _sources():
        text = open(path, errors="replace").read()
        for m in re.finditer(r'\bSW_SHARD_EMULATE\b|"SWM_SHARD_EMULATE"', text):
            before = text[: m.start()]
            assert before.count("#ifdef SWM_MEASURE_HOOKS") > before.count("#endif  // SWM_MEASURE_HOOKS") or \
                before.rfind("#ifdef SWM_MEASURE_HOOKS") > before.rfind("#endif"), path
    assert "SWM_MEASURE_HOOKS" not in open(os.path.join(CSRC, "Makefile")).read()
    lib = os.path.join(ROOT, "simpleworks_amd", "libswmarlin.so")
    if os.path.exists(lib):
        assert b"SWM_SHARD_EMULATE" not in open(lib, "rb").read()


def test_refused_values_fall_back_to_the_default(tmp_path):
    """env_switch: a value that does not parse or lies outside the declared range is refused, never clamped (compiled on the host
    from the shipped header)."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        import pytest
        pytest.skip("needs g++")
    src = tmp_path / "t.cpp"
    src.write_text('#include "switches.h"\n#include <stdio.h>\nint main() { printf("%ld %ld %d %d\\n", swm::env_switch("SWM_T_A", 7, 0, 9), '
                   'swm::env_switch("SWM_T_B", 3, 1, 3), (int)swm::env_flag("SWM_T_C"), (int)swm::env_flag("SWM_T_D")); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])

    def run(**env):
        e = {k: v for k, v in os.environ.items() if not k.startswith("SWM_T_")}
        e.update(env)
        out = subprocess.run([str(exe)], env=e, capture_output=True, text=True)
        return out.stdout.split(), out.stderr
    assert run()[0] == ["7", "3", "0", "0"]
    assert run(SWM_T_A="5", SWM_T_B="2", SWM_T_C="1", SWM_T_D="0")[0] == ["5", "2", "1", "0"]
    vals, err = run(SWM_T_A="10", SWM_T_B="2x")
    assert vals[:2] == ["7", "3"] and err.count("refused") == 2
    assert run(SWM_T_A="-1", SWM_T_B="")[0][:2] == ["7", "3"]
    assert run(SWM_T_A="0x9")[0][0] == "9"


def _host_program(tmp_path, body):
    """Compiles `body` (the statements of main) against the shipped switches.h; returns run(**env) -> (stdout words, stderr) under
    an environment without any of the library's variables but those given."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        import pytest
        pytest.skip("needs g++")
    src = tmp_path / "t.cpp"
    src.write_text('#include "switches.h"\n#include <stdio.h>\nusing namespace swm;\nint main() {\n%s\nreturn 0; }\n' % body)
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-I", CSRC, str(src), "-o", str(exe)])

    def run(**env):
        e = {k: v for k, v in os.environ.items() if not k.startswith("SWM_") and k != "LOCAL_WORLD_SIZE"}
        e.update(env)
        out = subprocess.run([str(exe)], env=e, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        return out.stdout.split(), out.stderr
    return run


def test_table_sanity(tmp_path):
    """The compiled table: unique names, integer defaults inside their range; a default outside the range is the declared "not
    set" of a K_OPT row, SWM_MSM_BATCH_BELOW among them.  And it is the table this file's row parser sees."""
    run = _host_program(tmp_path, 'for (const SwitchDecl& d : SWITCHES) printf("%s %d %ld %ld %ld %d %d\\n", d.name, (int)d.kind, d.def, d.lo, '
                                  'd.hi, (int)d.cls, (int)d.when);\nprintf("%d %d %d %d\\n", (int)K_INT, (int)K_OPT, (int)K_FLAG, (int)K_FILE);')
    words = run()[0]
    k_int, k_opt, k_flag, k_file = (int(x) for x in words[-4:])
    rows = [words[i:i + 7] for i in range(0, len(words) - 4, 7)]
    names = [r[0] for r in rows]
    assert len(set(names)) == len(names), names
    parsed = _read_switches()
    assert set(names) == {n for n, row in parsed.items() if row["cls"] != "C_HOOK"}   # (hooks: not in a build without the macro)
    kind_names = {k_int: "K_INT", k_opt: "K_OPT", k_flag: "K_FLAG", k_file: "K_FILE"}
    unset_outside_range = set()
    for name, kind, dflt, lo, hi, _, _ in rows:
        kind, dflt, lo, hi = int(kind), int(dflt), int(lo), int(hi)
        assert kind_names[kind] == parsed[name]["kind"], name
        if kind == k_int:
            assert lo <= dflt <= hi, name
        elif kind == k_opt:
            assert lo <= hi and not lo <= dflt <= hi, name
            unset_outside_range.add(name)
    assert "SWM_MSM_BATCH_BELOW" in unset_outside_range
    assert unset_outside_range == {"SWM_MSM_BATCH_BELOW", "SWM_MSM_TABLE_C", "SWM_POOL_WORKERS"}


def test_fingerprint_compares_decisions_not_text(tmp_path):
    """What the ranks of a sharded proof compare (shard_agree): equal for every environment in which the process takes the same
    decisions — a default spelled out, another spelling of a number, a refused value, a diagnostic — and different for every
    PATH or SHARDING switch that leaves its default."""
    run = _host_program(tmp_path, 'printf("%u\\n", switch_fingerprint());')
    empty = run()[0]
    for same in ({"SWM_MSM_QUAD": "1"}, {"SWM_SHARD_BLOCK_LOG": "12"}, {"SWM_SHARD_BLOCK_LOG": "0xc"}, {"SWM_MSM_LOW": "7"},
                 {"SWM_TRACE": "1"}, {"SWM_POOL_WORKERS": "3"}):
        assert run(**same)[0] == empty, same
    assert "refused" in run(SWM_MSM_LOW="7")[1]
    others = [run(**env)[0][0] for env in ({"SWM_MSM_QUAD": "0"}, {"SWM_SHARD_BLOCK_LOG": "10"}, {"SWM_NTT_LAZY": "0"},
                                           {"SWM_MASK_PIECES": "1"}, {"SWM_SHARD_RANGE": "1"})]
    assert len(set(others + empty)) == 6, (empty, others)


def test_once_rows_are_cached_and_live_rows_are_not(tmp_path):
    rows = _read_switches()
    assert rows["SWM_MSM_QUAD"]["when"] == "W_ONCE" and rows["SWM_SHARD_BLOCK_LOG"]["when"] == "W_LIVE"
    run = _host_program(tmp_path, 'long a = sw(SW_MSM_QUAD), b = sw(SW_SHARD_BLOCK_LOG);\nsetenv("SWM_MSM_QUAD", "1", 1);\n'
                                  'setenv("SWM_SHARD_BLOCK_LOG", "7", 1);\nprintf("%ld %ld %ld %ld\\n", a, sw(SW_MSM_QUAD), b, sw(SW_SHARD_BLOCK_LOG));')
    assert run(SWM_MSM_QUAD="0", SWM_SHARD_BLOCK_LOG="3")[0] == ["0", "0", "3", "7"]
    # the switches that the sharded-prover tests flip inside one process are LIVE; SWM_TRACE is one level, parsed once
    for name in SHARDING | {"SWM_RALPHA_TRANSFORMS", "SWM_SAMPLE_TIGHT"}:
        assert rows[name]["when"] == "W_LIVE", name
    assert (rows["SWM_TRACE"]["kind"], rows["SWM_TRACE"]["when"]) == ("K_INT", "W_ONCE")

"""Load and write times of one proving key at 2^lg constraints in the three forms of its bytes: the compressed checked reader
(swm_pk_deserialize), the uncompressed checked one (SWM_KEY_UNCOMPRESSED), the unchecked one (| SWM_KEY_UNCHECKED) and the two
writers, in alternating order, `rounds` times each; medians and spread (min .. max) per leg, next to one index() of the same key.
Only the library call is timed: the bytes sit in a ctypes buffer before the clock starts.  A last, profiled unchecked load lists
the kernels that take its device time, and what is left of the wall time for the host (parsing the matrices, the transposes).
usage: pk_load_time.py [lg=16] [rounds=5]"""
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simpleworks_amd import marlin as M, serialization as S, workloads as W  # noqa: E402

lg = int(sys.argv[1]) if len(sys.argv) > 1 else 16
rounds = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
n = 1 << lg
ctx = M.default_context()
lib = ctx.lib
cs, public = W.synthetic_r1cs(n, 3 + lg, 5)
srs = M.generate_universal_srs(n, n, n, M.generate_rand())
t = time.perf_counter()
pk, vk = M.generate_proving_and_verifying_keys(srs, cs)
ctx.synchronize()
t_index = time.perf_counter() - t
srs.free()


def write(flags):
    """(seconds, ctypes buffer) of one swm_pk_serialize_ex with a buffer of the right size"""
    size = ctypes.c_size_t(0)
    assert lib.swm_pk_serialize_ex(ctx.h, pk.h, flags, None, 0, ctypes.byref(size)) == 0
    buf = (ctypes.c_uint8 * size.value)()
    t0 = time.perf_counter()
    rc = lib.swm_pk_serialize_ex(ctx.h, pk.h, flags, buf, size.value, ctypes.byref(size))
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    return dt, buf


def load(buf, flags):
    h = ctypes.c_void_p()
    t0 = time.perf_counter()
    rc = lib.swm_pk_deserialize_ex(ctx.h, buf, len(buf), flags, ctypes.byref(h)) if flags else \
        lib.swm_pk_deserialize(ctx.h, buf, len(buf), ctypes.byref(h))
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    return dt, M.ProvingKey(ctx, h)


_, comp = write(0)
_, unc = write(S.KEY_UNCOMPRESSED)
legs = {"load compressed checked": [], "load uncompressed checked": [], "load unchecked": [], "write compressed": [], "write uncompressed": []}
last = None
for r in range(rounds):
    order = [("load compressed checked", comp, 0), ("load uncompressed checked", unc, S.KEY_UNCOMPRESSED),
             ("load unchecked", unc, S.KEY_UNCOMPRESSED | S.KEY_UNCHECKED)]
    for name, buf, flags in (order if r % 2 == 0 else order[::-1]):
        dt, key = load(buf, flags)
        legs[name].append(dt)
        if last is not None:
            last.free()
        last = key
    for name, flags in ((("write compressed", 0), ("write uncompressed", S.KEY_UNCOMPRESSED)) if r % 2 == 0 else
                        (("write uncompressed", S.KEY_UNCOMPRESSED), ("write compressed", 0))):
        legs[name].append(write(flags)[0])
# the last key loaded proves like the original
seed = bytes(range(32))
assert M.generate_proof(cs, last, M.rng_from_seed(seed)).data == M.generate_proof(cs, pk, M.rng_from_seed(seed)).data
last.free()

print("2^%d constraints, %d rounds; key bytes: compressed %.1f MB, uncompressed %.1f MB; index() %.3f s (one run, SRS resident)"
      % (lg, rounds, len(comp) / 1e6, len(unc) / 1e6, t_index))
for name, ts in legs.items():
    print("  %-26s median %8.1f ms   min %8.1f   max %8.1f" % (name, statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3))

ctx.profile_enable(True)
ctx.profile_reset()
dt, key = load(unc, S.KEY_UNCOMPRESSED | S.KEY_UNCHECKED)
kernels = ctx.profile()
ctx.profile_enable(False)
key.free()
dev = sum(k["total_ms"] for k in kernels.values())
print("  profiled unchecked load: wall %.1f ms, kernels %.1f ms (%.0f %%); the rest is host work and copies"
      % (dt * 1e3, dev, 100 * dev / (dt * 1e3)))
for k in sorted(kernels.values(), key=lambda k: -k["total_ms"])[:8]:
    print("    %-28s %4d calls %9.2f ms" % (k["name"], k["calls"], k["total_ms"]))
pk.free()

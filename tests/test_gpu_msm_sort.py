"""The arrays the MSM's sort stage leaves on the device — everything between the scalars and the first addition: digits, histogram,
placement, bucket and segment descriptors, the ordering by length, the list of oversized buckets — held to the digit model of
tests/msm_sort_model.py count by count, through swm_selftest_msm_sort, which runs the host functions msm_enqueue runs and stops
after msm_seg_order.  In-process, default switches, no oracle: nothing here adds points.

The final point of a whole MSM cannot show these: a segment missing from order[] leaves the partial sum an earlier job of the same
shape left (often the right point), a wrong length order costs only time, len_hist / nseg_live / big_list have no reader that turns
a small error into a wrong group element on the vectors the other tests run.  The checker (msm_sort_model.check) is shown to reject
each such corruption by tests/test_msm_sort_model_host.py.

Jobs (msm_sort_model.JOBS; the shape the entry returns must be the predicted one, msm_sort_model.predicted_shape, and read the
regime msm_sort_model.REGIME names — a tuning change fails here by name):
  * per-window schedule on a 300-point set: n = 1, 2, 300 (msm_hist, msm_scan_*, msm_seg_desc, msm_scatter);
  * flat, low-latency, quad bucket stage: 513 points on a set of their own (c = 11);
  * flat, low-latency, one lane, on [tau^i]G of 2^18 + 1 points (c = 19) with the identity holes of test_gpu_msm_te29.py:
    n = 2^15 + 3 (SEG 16, big_nseg 4) at offset 0 and at an offset, n = 65537 (big_nseg 6), n = 190000 (SEG 32);
  * flat, throughput: n = 2^18 + 1 (SEG 128, big_nseg 16, G = 256);
  * twin lead: n = 2^15 + 3 with a follower at another offset, on a set without identity bases.
Vectors per job: uniform; scalars_for of test_gpu_msm_te29.py (jobs of at least 458 points); the occupancy ladder, whose buckets
sit ON every entry count the stage branches on; all zeros; all equal; all r - 1.  Every (job, vector) runs the entry twice in a
row and checks both downloads: the second run meets the first one's scratch.

Known and NOT covered here:
  * the two-level per-window sort (SWM_MSM_NO_TABLE=1, n >= 262144): it needs a child process; test_gpu_msm_schedules.py runs it
    through whole MSMs;
  * as there: the 4096-bin / 8 K-tile form of msm_flat_partition (more than 57 M digits), the `ns >= 2^24` clause of flat_seg_write."""
import numpy as np
import pytest

import msm_sort_model as M
from oracle_lib import Oracle, golden, h2i
from test_gpu_msm_te29 import HOLES, scalars_for

KINDS = ("uniform", "te29", "ladder", "zeros", "equal", "r_minus_1")
TE29_MIN = 458      # scalars_for places that many special scalars


@pytest.fixture(scope="module")
def env():
    import simpleworks_amd as swm
    orc = Oracle()
    tau = h2i(golden("msm.json")["tau"])
    G = orc.points_to_mont([tuple(h2i(v) for v in golden("g1.json")["generator"])])
    bases = orc.srs_bases(M.N_BIG, tau, G)
    bases[list(HOLES)] = 0
    bases[M.N_BIG - 2] = 0
    assert max(HOLES) < M.TWIN_LO and M.TWIN_LO + 2 * M.N_MID < M.N_BIG - 2
    ctx = swm.Context(0)
    first = {"big": 0, "quad": 0, "small": 0, "twin": M.TWIN_LO}
    sets = {k: ctx.srs_upload(np.ascontiguousarray(bases[first[k]:first[k] + M.SET_SIZE[k]])) for k in first}
    holes = {k: ~bases[first[k]:first[k] + M.SET_SIZE[k]].any(axis=1) for k in first}
    yield ctx, sets, holes
    for s in sets.values():
        s.free()
    ctx.close()


def vector(kind, name, shape, skip):
    from pyref.prng import fr_array
    job = M.JOBS[name]
    n, seed = job["n"], 3100 + sorted(M.JOBS).index(name)
    if kind == "uniform":
        return fr_array(n, seed)
    if kind == "te29":
        return scalars_for(n, seed)
    if kind == "ladder":
        return M.ladder(shape, n, seed, job["rungs"], skip=skip)[0]
    if kind == "zeros":
        return np.zeros((n, 4), dtype=np.uint64)
    if kind == "equal":
        return np.ascontiguousarray(np.tile(fr_array(1, seed), (n, 1)))
    return np.ascontiguousarray(np.tile(M.limbs([M.R - 1]), (n, 1)))


CASES = [(name, kind) for name in M.JOBS for kind in KINDS if kind != "te29" or M.JOBS[name]["n"] >= TE29_MIN]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", CASES, ids=["%s-%s" % c for c in CASES])
def test_sort_stage_against_the_model(env, name, kind):
    ctx, sets, holes = env
    job = M.JOBS[name]
    n, offset, bh = job["n"], job["offset"], sets[job["set"]]
    follow = (bh, job["follow_offset"]) if "follow_offset" in job else None
    shape, _ = ctx.selftest_msm_sort(bh, np.zeros((n, 4), dtype=np.uint64), offset=offset, follow=follow, shape_only=True)
    print("shape %s: %r" % (name, shape))
    assert shape == M.job_shape(name), "the library shapes this job otherwise than msm_sort_model.predicted_shape"
    assert {k: shape[k] for k in M.REGIME[name]} == M.REGIME[name]
    skip = holes[job["set"]][offset:offset + n]
    sc = vector(kind, name, shape, skip)
    model = M.Model(sc, shape, offset=offset, skip=skip, follow=(shape["tstride"], job["follow_offset"]) if follow else None)
    if kind == "zeros":
        assert model.entries == 0
    if kind in ("equal", "r_minus_1"):   # one bucket per window digit, each holding every point with a base
        assert set(np.unique(model.count)) <= {0} | {int((~skip).sum()) * k for k in range(1, shape["nwin"] + 1)}
    for run in (1, 2):
        got_shape, arrays = ctx.selftest_msm_sort(bh, sc, offset=offset, follow=follow)
        assert got_shape == shape
        assert arrays["bad_scalar"] == 0
        assert arrays["zero_points"] == int((skip | ~sc.any(axis=1)).sum())
        try:
            M.check(shape, arrays, model)
        except M.SortMismatch as e:
            raise AssertionError("%s / %s, run %d: %s" % (name, kind, run, e)) from None
        if kind == "zeros":
            assert arrays["nseg_live"] == 0 and arrays["big_count"] == 0 and arrays["entries"] == 0


@pytest.mark.gpu
def test_montgomery_scalars_and_deferred_shape(env):
    """the same job from Montgomery-form scalars, and shaped as a deferred job (the sort stage does not depend on it)"""
    ctx, sets, holes = env
    name = "lat_2p15_offset"
    job = M.JOBS[name]
    shape = M.job_shape(name)
    skip = holes["big"][job["offset"]:job["offset"] + job["n"]]
    sc = vector("ladder", name, shape, skip)
    model = M.Model(sc, shape, offset=job["offset"], skip=skip)
    mont = Oracle().fr_to_mont(np.ascontiguousarray(sc))
    for kwargs, vec in (({"montgomery": True}, mont), ({"defer_tail": True}, sc)):
        got_shape, arrays = ctx.selftest_msm_sort(sets["big"], vec, offset=job["offset"], **kwargs)
        assert got_shape == shape
        M.check(shape, arrays, model)


@pytest.mark.gpu
def test_bad_arguments(env):
    import simpleworks_amd as swm
    ctx, sets, _ = env
    for kwargs in ({"offset": M.N_SMALL}, {"follow": (sets["quad"], M.N_QUAD)}):
        with pytest.raises(swm.SwmError) as e:
            ctx.selftest_msm_sort(sets["small"], np.zeros((2, 4), dtype=np.uint64), **kwargs)
        assert e.value.code == -1

"""Whole MSMs whose bucket stage adds in the 29-bit domain (csrc/fq29.cuh te29_slot_add; msm_points.cuh FormTE29, msm_stages.h MsmShape::raw) against the
CPU oracle, on subgroup bases [tau^i]G with the scalar vectors of tests/test_gpu_msm_te29.py (0, 1, r - 1, extreme digits of every
table width, scalars repeated 1, 2, 128 and 300 times, identity bases under some of them) plus one scalar repeated 4173 times: with
the 128-entry segments of a large job that is a bucket of 33 segments, more than BIG_NSEG = 16, which msm_big_bucket_sum folds
ahead of the stage (in the small jobs, 16-entry segments, the 300 repeats already are 19).

Shapes, each the smallest that takes its path (the table's width follows the size of the base SET: 2^18 + 1 bases give c = 19,
2^18 buckets, too many for the quad stage whatever the job's size):
  * two jobs of 2^18 + 1 points back to back, bucket stages not deferred: msm_accumulate_te stores raw partial sums; the first
    job's stage is launched thin by the second's enqueue, the last one's wide by the flush — msm_bucket_reduce<256, FormTE29>;
  * three deferred jobs of 2^15 + 3 points on the same set: msm_accumulate_te_quad stores raw partial sums, one joint
    msm_bucket_reduce_low on 29-bit slots, its weighted sums in HBM at the raw stride;
  * 513 points on a set of their own (c = 11): a quad bucket stage, partial sums still 28-bit slots through the epilogue.
Each test also holds its jobs to the stage kernel named above, through the context's per-kernel job counts.

The occupancy ladders of tests/msm_sort_model.py — vectors whose buckets hold EXACTLY 1, 2, SEG - 1 .. 2 SEG + 1 entries, big_nseg
and big_nseg + 1 segments, FLAT_WIDE_NS and one more, G - 1 .. 2 G + 1 segments for the lane group G of msm_big_bucket_sum, one
bucket of negative digits only — run through whole MSMs in the four table regimes (quad; low-latency one lane, deferred and not;
throughput).  tests/test_gpu_msm_sort.py holds the sort's arrays on these vectors to the model; here the three places that must
agree on `ns > big_nseg` (the list, the fold of msm_big_bucket_sum, the walk of msm_bucket_reduce / _low / the quad form over a
listed bucket's first partial sum only) and the fold's strided loop around ns = G have to add up to the oracle's point.

There is no run-time switch back to 28-bit slots for one-lane jobs and so no child-process leg: that stage is no longer in the
library."""
import numpy as np
import pytest

import msm_sort_model as M
from oracle_lib import Oracle, golden, h2i, ints_to_limbs
from test_gpu_msm_te29 import HOLES, affine, scalars_for

N_BIG = (1 << 18) + 1
N_MID = (1 << 15) + 3
BIG_REPEATS = 4173


def scalars_with_big_bucket(n, seed):
    sc = scalars_for(n, seed)
    if n >= 2 * BIG_REPEATS:
        rep = int(np.random.default_rng(seed + 1).integers(1, 1 << 62)) | (1 << 251)
        sc[n - 7 - BIG_REPEATS:n - 7] = ints_to_limbs([rep], 4)
    return sc


@pytest.fixture(scope="module")
def env():
    import simpleworks_amd as swm
    orc = Oracle()
    tau = h2i(golden("msm.json")["tau"])
    G = orc.points_to_mont([tuple(h2i(v) for v in golden("g1.json")["generator"])])
    bases = orc.srs_bases(N_BIG, tau, G)
    bases[list(HOLES)] = 0
    bases[N_BIG - 2] = 0
    ctx = swm.Context(0)
    bh = ctx.srs_upload(bases)
    yield orc, ctx, bases, bh
    bh.free()
    ctx.close()


def tails_run(ctx, before):
    """jobs per bucket-stage kernel since `before`"""
    now = ctx.selftest_msm_tail_counts()
    return {k: now[k] - before[k] for k in now}


def oracle_point(orc, b, sc):
    return orc.jac_to_affine_int(orc.msm(np.ascontiguousarray(b), sc, threads=orc.lib.oracle_max_threads()))


def test_the_big_bucket_is_big():
    """No device: the repeated scalar fills more than BIG_NSEG segments of the large job's segment length"""
    sc = scalars_with_big_bucket(N_BIG, 5)
    rows, counts = np.unique(sc, axis=0, return_counts=True)
    assert counts.max() == BIG_REPEATS > 16 * 128
    assert np.array_equal(scalars_with_big_bucket(513, 5), scalars_for(513, 5))


@pytest.mark.gpu
def test_two_large_jobs_thin_then_wide(env):
    orc, ctx, bases, bh = env
    vecs = [scalars_with_big_bucket(N_BIG, 2951), scalars_with_big_bucket(N_BIG, 2952)]
    before = ctx.selftest_msm_tail_counts()
    jacs, _ = ctx.selftest_msm_jobs([bh], vecs, [(0, 0, 0, N_BIG, None), (0, 0, 1, N_BIG, None)], defer_tail="off")
    assert tails_run(ctx, before) == {"quad": 0, "low": 0, "te29": 2, "xyzz": 0}
    for j, sc in zip(jacs, vecs):
        assert affine(orc, ctx, j) == oracle_point(orc, bases, sc)


@pytest.mark.gpu
def test_three_deferred_jobs_share_the_low_lds_stage(env):
    orc, ctx, bases, bh = env
    offs = (0, 1000, N_BIG - N_MID)
    vecs = [scalars_with_big_bucket(N_MID, 2960 + i) for i in range(3)]
    before = ctx.selftest_msm_tail_counts()
    jacs, _ = ctx.selftest_msm_jobs([bh], vecs, [(0, off, i, N_MID, None) for i, off in enumerate(offs)], defer_tail="on")
    assert tails_run(ctx, before) == {"quad": 0, "low": 3, "te29": 0, "xyzz": 0}
    for j, off, sc in zip(jacs, offs, vecs):
        assert affine(orc, ctx, j) == oracle_point(orc, bases[off:off + N_MID], sc), off


@pytest.mark.gpu
def test_quad_tail_keeps_28_bit_slots(env):
    orc, ctx, bases, _ = env
    b = np.ascontiguousarray(bases[:513])
    sc = scalars_with_big_bucket(513, 2970)
    small = ctx.srs_upload(b)
    before = ctx.selftest_msm_tail_counts()
    try:
        got = affine(orc, ctx, ctx.msm_g1(small, sc))
    finally:
        small.free()
    assert tails_run(ctx, before) == {"quad": 1, "low": 0, "te29": 0, "xyzz": 0}
    assert got == oracle_point(orc, b, sc)


# regime -> (job of msm_sort_model.JOBS whose ladder it runs, defer_tail, the bucket-stage kernel it must take)
LADDERS = {"quad": ("quad_513", None, "quad"), "low_latency_deferred": ("lat_2p15_offset", "on", "low"),
           "low_latency": ("lat_2p15", "off", "te29"), "throughput": ("throughput", "off", "te29")}


@pytest.mark.gpu
@pytest.mark.parametrize("regime", list(LADDERS))
def test_ladder_msm_equals_the_oracle(env, regime):
    orc, ctx, bases, bh = env
    name, defer, kernel = LADDERS[regime]
    job = M.JOBS[name]
    n, off = job["n"], job["offset"]
    b = np.ascontiguousarray(bases[off:off + n])
    shape = M.job_shape(name)
    sc, rung = M.ladder(shape, n, 2980 + len(name), job["rungs"], skip=~b.any(axis=1))
    model = M.Model(sc, shape, offset=off, skip=~b.any(axis=1))
    targets = M.rung_targets(shape)
    assert {k: int(model.count[v]) for k, v in rung.items()} == {k: targets[k] for k in job["rungs"]}
    assert {rung["ns=big+1,first+1"]} <= model.big and rung["ns=big"] not in model.big
    before = ctx.selftest_msm_tail_counts()
    if defer is None:
        small = ctx.srs_upload(b)
        try:
            got = affine(orc, ctx, ctx.msm_g1(small, sc))
        finally:
            small.free()
    else:
        jacs, _ = ctx.selftest_msm_jobs([bh], [sc], [(0, off, 0, n, None)], defer_tail=defer)
        got = affine(orc, ctx, jacs[0])
    want = {"quad": 0, "low": 0, "te29": 0, "xyzz": 0}
    want[kernel] = 1
    assert tails_run(ctx, before) == want
    assert got == oracle_point(orc, b, sc), regime

"""The planned sparse mat-vec (csrc/spmv.hip: rows up to 64 entries one lane each, longer rows cut into chunks of 2048 that one
workgroup each reduces, then one workgroup per long row adds its chunk sums) — the schedule the prover and is_satisfied run for
A, B, C and the transposes — directly, through swm_selftest_spmv_plan, which uploads the matrix the way a key's matrix is and
runs with the plan recorded there.  Row lengths sit on both thresholds and their multiples, long rows first, last, adjacent
and alone, and one row has more chunks than the last kernel has lanes.  Bit-exact against the C oracle (64-bit limbs) and
against the unplanned schedules behind swm_spmv_fr; the plan's chunk and long-row counts are the ones 64 and 2048 give."""
import numpy as np
import pytest

from oracle_lib import Oracle, R
from pyref.prng import fr_array

pytestmark = pytest.mark.gpu

DIRECT_MAX, CHUNK, LANES = 64, 2048, 256
COLS = 1500


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def ctx():
    import simpleworks_amd as swm
    c = swm.Context(0)
    yield c
    c.close()


def _short(rng, rows):
    return np.minimum(rng.poisson(2, rows), DIRECT_MAX).astype(np.int64)


def _thresholds(rng):
    cnt = _short(rng, 400)
    cnt[0] = 4097                                      # a long row first
    cnt[50:54] = [0, 1, DIRECT_MAX, DIRECT_MAX + 1]
    cnt[100:102] = [CHUNK - 1, CHUNK]                  # two long rows side by side
    cnt[200] = 2 * CHUNK
    cnt[399] = CHUNK + 1                               # a long row last
    return cnt


def _only_long(rng):
    return np.array([DIRECT_MAX + 1, CHUNK, CHUNK + 1, 100, 2 * CHUNK + 1], dtype=np.int64)


def _more_chunks_than_lanes(rng):
    cnt = _short(rng, 60)
    cnt[31] = LANES * CHUNK + 1                        # 257 chunks: the second trip of the strided loop over chunk sums
    cnt[32] = DIRECT_MAX + 1
    return cnt


def _no_long(rng):
    cnt = _short(rng, 300)
    cnt[[0, 7, 299]] = DIRECT_MAX
    cnt[[3, 8]] = [0, 1]
    return cnt


SHAPES = {"thresholds": _thresholds, "only_long": _only_long, "more_chunks_than_lanes": _more_chunks_than_lanes,
          "no_long": _no_long}


def _matrix(orc, name):
    seed = sorted(SHAPES).index(name)
    rng = np.random.default_rng(100 + seed)
    cnt = SHAPES[name](rng)
    rowptr = np.zeros(cnt.size + 1, dtype=np.uint32)
    rowptr[1:] = np.cumsum(cnt)
    nnz = int(rowptr[-1])
    col = rng.integers(0, COLS, nnz, dtype=np.uint32)
    one, minus_one, zero = orc.fr_mont_from_ints([1, R - 1, 0])
    val = orc.fr_to_mont(fr_array(nnz, 200 + seed))
    val[::3] = one                                     # the coefficient-one shortcut
    val[1::7] = minus_one
    z = orc.fr_to_mont(fr_array(COLS, 300 + seed))
    z[::11] = zero
    z[5::13] = minus_one
    return cnt, rowptr, col, val, z


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_planned_spmv_against_the_oracle_and_the_unplanned_schedules(ctx, orc, name):
    cnt, rowptr, col, val, z = _matrix(orc, name)
    want = orc.spmv(rowptr, col, val, z, threads=8)
    got, n_chunks, n_lrows = ctx.selftest_spmv_plan(rowptr, col, val, z)
    long_rows = cnt[cnt > DIRECT_MAX]
    assert n_lrows == long_rows.size
    assert n_chunks == int(((long_rows + CHUNK - 1) // CHUNK).sum())
    if name == "no_long":
        assert n_chunks == 0 and n_lrows == 0
    else:
        assert n_lrows >= 2
    assert np.array_equal(got, want)
    assert np.array_equal(got, ctx.spmv_fr(rowptr, col, val, z))
    # the same call again: the pool hands the result block back, every row must be written anew
    assert np.array_equal(ctx.selftest_spmv_plan(rowptr, col, val, z)[0], want)


def test_planned_spmv_refuses_malformed_input(ctx, orc):
    import simpleworks_amd as swm
    _, rowptr, col, val, z = _matrix(orc, "no_long")
    bad_col = col.copy()
    bad_col[-1] = COLS
    bad_ptr = rowptr.copy()
    bad_ptr[5] = bad_ptr[4] - 1                        # row 0 holds 64 entries, so this is not below zero
    for args in ((rowptr, bad_col, val, z), (bad_ptr, col, val, z), (rowptr + np.uint32(1), col, val, z)):
        with pytest.raises(swm.SwmError) as e:
            ctx.selftest_spmv_plan(*args)
        assert e.value.code == -1

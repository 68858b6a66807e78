"""No device: the sort-stage model of tests/msm_sort_model.py, its checker and its occupancy ladders.

  * the model's entry words, buckets, counts and segment lengths against plain integers, scalar by scalar;
  * the checker: arrays built by the model are accepted; corrupted one way at a time, each is rejected with a message that names
    the broken promise — what shows that tests/test_gpu_msm_sort.py can fail;
  * the ladders: for every job of the case table the count of every rung bucket is EXACTLY its target under the model, the rungs
    hold a bucket on both sides of every predicate the stage branches on (but for the ones the table lists as one-sided because
    the job is too small), and a rung that does not fit is refused by name."""
import numpy as np
import pytest

import msm_sort_model as M


def small_job(follow=None, seed=11):
    """the 513-point quad job with its ladder (SEG = 32, big_nseg = 4), optionally as a lead"""
    shape = M.job_shape("quad_513")
    if follow:
        shape["lead"] = 1
    sc, rung = M.ladder(shape, M.N_QUAD, seed, M.JOBS["quad_513"]["rungs"])
    return shape, sc, rung, M.Model(sc, shape, offset=0, follow=follow)


def test_model_against_plain_integers():
    """every entry of a flat and of a per-window job, rebuilt digit by digit on Python integers"""
    from pyref.prng import fr_array
    special = M.limbs([0, 1, M.R - 1, M.R - 2, 1 << 9, (1 << 9) + 1, (1 << 252) + 12345])
    for name, n, offset in (("quad_513", M.N_QUAD, 0), ("per_window_n300", M.N_SMALL, 0)):
        shape = M.job_shape(name)
        sc = fr_array(n, 77)
        sc[:len(special)] = special
        skip = np.zeros(n, dtype=bool)
        skip[[2, 9]] = True
        m = M.Model(sc, shape, offset=offset, skip=skip)
        want = {}
        for i in range(n):
            s = sum(int(sc[i, k]) << (64 * k) for k in range(4))
            carry, bit, tot, boff = 0, 0, 0, 0
            for w, c in enumerate(shape["c"]):
                d = ((s >> bit) & ((1 << c) - 1)) + carry
                carry = 1 if d > (1 << (c - 1)) else 0
                d -= carry << c
                tot += d << bit
                bit += c
                if d and not skip[i]:
                    row = w * shape["tstride"] + offset + i if shape["flat"] else i
                    b = (0 if shape["flat"] else boff) + abs(d) - 1
                    want.setdefault(b, []).append(row | ((1 << 31) if d < 0 else 0))
                boff += 1 << (c - 1)
            assert tot == s and carry == 0
        assert m.entries == sum(len(v) for v in want.values())
        assert {b: int(c) for b, c in enumerate(m.count) if c} == {b: len(v) for b, v in want.items()}
        for b in want:
            assert sorted(int(x) for x in m.word[m.bucket == b]) == sorted(want[b])
        assert m.nseg_live == sum(-(-len(v) // shape["SEG"]) for v in want.values())


def test_segment_lengths():
    for count in (1, 2, 31, 32, 33, 64, 65, 97, 128, 129, 2049):
        for seg in (16, 32, 128):
            ns = -(-count // seg)
            for inter in (False, True):
                ln = M.segment_lengths(count, seg, inter)
                assert len(ln) == ns and sum(ln) == count and max(ln) <= seg and max(ln) - min(ln) <= 1
            if ns > 1:   # round-robin: segment k takes the entries k, k + ns, ...
                assert M.segment_lengths(count, seg, True) == [len(range(k, count, ns)) for k in range(ns)]


def test_checker_accepts_what_the_model_builds():
    shape, sc, rung, m = small_job()
    M.check(shape, m.arrays(), m)
    M.check(shape, m.arrays(gap=0), m)
    shape, sc, rung, m = small_job(follow=(700, 150))
    M.check(shape, m.arrays(), m)
    for name in ("per_window_n1", "per_window_n300"):
        shape = M.job_shape(name)
        sc, _ = M.ladder(shape, M.JOBS[name]["n"], 5, M.JOBS[name]["rungs"])
        m = M.Model(sc, shape)
        M.check(shape, m.arrays(), m)
    zeros = np.zeros((M.N_QUAD, 4), dtype=np.uint64)
    shape = M.job_shape("quad_513")
    m = M.Model(zeros, shape)
    assert m.entries == 0 and m.nseg_live == 0 and not m.big
    M.check(shape, m.arrays(), m)


def swap_across_buckets(a, m, rung):
    i, j = int(a["bucket_off"][rung["SEG"]]), int(a["bucket_off"][rung["SEG+1"]])
    a["sorted"][[i, j]] = a["sorted"][[j, i]]


def duplicate_over_neighbour(a, m, rung):
    i = int(a["bucket_off"][rung["SEG+1"]])
    a["sorted"][i + 1] = a["sorted"][i]


def order_drops_one_repeats_another(a, m, rung):
    a["order"][5] = a["order"][6]


def order_by_length_broken(a, m, rung):
    k = m.nseg_live - 1
    assert (a["seg_len"][a["order"][0]] & 0xFF) > (a["seg_len"][a["order"][k]] & 0xFF)
    a["order"][[0, k]] = a["order"][[k, 0]]


def length_bumped(a, m, rung):
    a["seg_len"][a["seg_off"][rung["SEG-1"]]] += 1


def tail_left_nonzero(a, m, rung):
    used = np.zeros(a["seg_bound"], dtype=bool)
    for b in np.nonzero(m.count)[0]:
        used[a["seg_off"][b]:a["seg_off"][b] + m.ns[b]] = True
    a["seg_len"][np.nonzero(~used)[0][0]] = M.UNWRITTEN


def big_list_lists_exactly_big_nseg(a, m, rung):
    assert m.ns[rung["ns=big"]] == m.big_nseg
    a["big_list"][a["big_count"]] = rung["ns=big"]
    a["big_count"] += 1


def big_list_misses_big_nseg_plus_one(a, m, rung):
    b = rung["ns=big+1,first+1"]
    assert m.ns[b] == m.big_nseg + 1
    keep = [x for x in a["big_list"][:a["big_count"]] if x != b]
    assert len(keep) == a["big_count"] - 1
    a["big_list"][:len(keep)] = keep
    a["big_count"] -= 1


def len_hist_off_by_one(a, m, rung):
    a["len_hist"][m.seg - 2] += 1


def sorted2_word_unmapped(a, m, rung):
    i = int(a["bucket_off"][rung["2SEG+1"]]) + 3
    a["sorted2"][i] = a["sorted"][i]


def unwritten_word_in_a_range(a, m, rung):
    a["sorted"][int(a["bucket_off"][rung["2"]]) + 1] = M.UNWRITTEN


def hist_off_by_one(a, m, rung):
    a["hist"][rung["1"]] += 1


def entries_word_off(a, m, rung):
    a["entries"] -= 1


CORRUPTIONS = (
    (swap_across_buckets, "multiset"), (duplicate_over_neighbour, "multiset"), (order_drops_one_repeats_another, "order"),
    (order_by_length_broken, "order"), (length_bumped, "cover"), (tail_left_nonzero, "tail"),
    (big_list_lists_exactly_big_nseg, "big_list"), (big_list_misses_big_nseg_plus_one, "big_list"), (len_hist_off_by_one, "len_hist"),
    (sorted2_word_unmapped, "sorted2"), (unwritten_word_in_a_range, "unwritten"), (hist_off_by_one, "hist"), (entries_word_off, "entries"),
)


@pytest.fixture(scope="module")
def lead_job():
    return small_job(follow=(700, 150))


@pytest.mark.parametrize("corrupt,tag", CORRUPTIONS, ids=[c[0].__name__ for c in CORRUPTIONS])
def test_checker_rejects(lead_job, corrupt, tag):
    shape, sc, rung, m = lead_job
    a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in m.arrays().items()}
    corrupt(a, m, rung)
    with pytest.raises(M.SortMismatch) as e:
        M.check(shape, a, m)
    assert str(e.value).startswith(tag + ":"), str(e.value)


@pytest.mark.parametrize("name", list(M.JOBS))
def test_ladder_counts_are_exact(name):
    job = M.JOBS[name]
    shape = M.job_shape(name)
    assert {k: shape[k] for k in M.REGIME[name]} == M.REGIME[name]
    n = job["n"]
    skip = np.zeros(n, dtype=bool)
    skip[[i for i in (0, 5, 100) if i < n - 1]] = n > 2
    sc, rung = M.ladder(shape, n, 40 + len(name), job["rungs"], skip=skip)
    assert sc.shape == (n, 4) and set(rung) == set(job["rungs"]) and len(set(rung.values())) == len(rung)
    m = M.Model(sc, shape, offset=job["offset"], skip=skip)
    targets = M.rung_targets(shape)
    assert {k: int(m.count[b]) for k, b in rung.items()} == {k: targets[k] for k in job["rungs"]}
    if "negative" in rung:
        words = m.word[m.bucket == rung["negative"]]
        assert len(words) == 3 and (words >> 31).all()
    counts = [targets[k] for k in job["rungs"]]
    one_sided = tuple(p for p, f in M.predicates(shape).items() if len({bool(f(c)) for c in counts}) < 2)
    assert one_sided == tuple(job["one_sided"])
    # the named segment counts are what their names say
    ns = lambda k: -(-targets[k] // shape["SEG"])
    G = 1 << shape["log_g"]
    assert [ns(k) for k in ("ns=big", "ns=big,first+1", "ns=big+1", "ns=big+1,first+1")] == [shape["big_nseg"]] * 2 + [shape["big_nseg"] + 1] * 2
    assert [ns(k) for k in ("ns=wide", "ns=wide+1", "ns=G-1", "ns=G", "ns=G+1", "ns=2G+1")] == [16, 17, G - 1, G, G + 1, 2 * G + 1]


def test_a_rung_that_does_not_fit_is_refused_by_name():
    shape = M.job_shape("per_window_n300")
    with pytest.raises(ValueError, match="ns=big"):
        M.ladder(shape, M.N_SMALL, 3, ("1", "ns=big"))
    dropped = {name: [k for k in M.RUNGS if k not in job["rungs"]] for name, job in M.JOBS.items()}
    assert dropped["throughput"] == dropped["lat_2p15"] == dropped["twin_lead"] == []
    assert dropped["quad_513"] == ["2SEG", "ns=big,first+1", "ns=big+1", "ns=wide", "ns=wide+1", "ns=G-1", "ns=G", "ns=G+1", "ns=2G+1"]
    for name, job in M.JOBS.items():   # nothing is dropped that would have fitted beside the rungs kept
        targets = M.rung_targets(M.job_shape(name))
        room = job["n"] - sum(targets[k] for k in job["rungs"])
        assert all(targets[k] > room for k in dropped[name]), name

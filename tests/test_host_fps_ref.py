"""Host: the three statements of tests/fps_ref.py against the C oracle and against one another on every case of tests/fps_cases.py, and
the cases against the properties they are named for.  What this file establishes for tests/test_gpu_fps_edges.py:
  * fps_f32 is the oracle's FPS, and its picks are farthest points in float64 (check_farthest_f64, which does reject a pick at 0.99);
  * the slab algorithm as designed (slab_model) returns the plain picks on every slab-size case;
  * on the elongated families the skip leaves most slabs alone, and bounds narrowed by 8 bins, or taken from the next slab, change the
    picks on named cases of every slab instantiation: a kernel with such a bound cannot pass the GPU file;
  * the plain kernel's arg-max hierarchy (plain_model) returns the plain picks on every other case; >= in a thread's walk or an
    unfiltered lowest index in a wave change the picks of the tie cases at every instantiation that can show it; an empty slot holding 0
    instead of -1 changes nothing anywhere (like the two-bin widening of the slab bounds, a margin that no input can see);
  * every tie case has its equal candidates where its name says, by the kernels' ownership rules restated here.
"""
import functools

import numpy as np
import pytest

import fps_cases as cases
import fps_ref as ref
import keypoint_sampling_ref

SLAB_RUNS = [r for r in cases.RUNS if cases.is_slab(r[2])]
ELONGATED_SLAB_RUNS = [r for r in SLAB_RUNS if len(r[1]) == 1 and r[1][0] in cases.ELONGATED]
TIE_RUNS = [r for r in cases.RUNS if r[1][0].startswith("tie_")]


@functools.lru_cache(maxsize=None)
def want(rid):
    _, families, n, k = cases.RUNS[cases.RUN_IDS.index(rid)]
    out = ref.fps_f32(cases.build(families, n), k)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model(family, n, k, narrow):
    return ref.slab_model(cases.cloud(family, n), k, narrow)


def test_the_runs_cover_the_dispatcher():
    sizes = {n for _, _, n, _ in cases.RUNS}
    assert sizes >= set(cases.SIZES) and max(sizes) == 65536
    for f in cases.ELONGATED + cases.SLAB_TIES:
        assert {n for _, fam, n, _ in cases.RUNS if fam == (f,)} >= set(cases.SLAB_SIZES), f
    for f in cases.ELONGATED + cases.PLAIN_TIES[1:]:
        assert {n for _, fam, n, _ in cases.RUNS if fam == (f,)} >= set(cases.PLAIN_ONE_PER_KERNEL), f
    assert {n for _, fam, n, _ in cases.RUNS if fam == ("tie_slots",)} == set(cases.PLAIN_ONE_PER_KERNEL[1:])
    assert {cases.slab_slots(n) for n in cases.SLAB_SIZES} == {16, 32, 64}
    assert [cases.slab_slots(n) for n in (1025, 4096, 4097, 8192, 8193, 16384)] == [16, 16, 32, 32, 64, 64]
    assert {(n, k) for _, fam, n, k in cases.RUNS if fam == ("doubled",) and k == n} == {(1024, 1024), (1025, 1025), (1300, 1300)}
    assert all(k <= 256 or k == n for _, _, n, k in cases.RUNS)
    assert any(len(fam) == 3 and "all_equal" in fam and len(set(fam)) == 3 for _, fam, _, _ in cases.RUNS)


@pytest.mark.parametrize("run", cases.RUNS, ids=cases.RUN_IDS)
def test_fps_f32_is_the_oracle_and_picks_farthest_points(oracle, run):
    rid, families, n, k = run
    xyz = cases.build(families, n)
    got = want(rid)
    assert got.dtype == np.int32 and got.shape == (len(families), k)
    np.testing.assert_array_equal(got, oracle.fps(xyz, k))
    for b in range(len(families)):
        ref.check_farthest_f64(xyz[b], got[b])


def test_fps_chain_is_fps_f32():
    p = cases.cloud("lattice", 1023)
    assert keypoint_sampling_ref.fps_chain(p, 40) == ref.fps_f32(p, 40).tolist()
    assert ref.fps_f32(p[None], 40).shape == (1, 40) and ref.fps_f32(p[:1], 1).tolist() == [0]


def test_check_farthest_rejects_a_pick_at_099():
    # by hand: from the origin, (1, 0, 0) is 1 away and (0, sqrt(0.99), 0) is 0.99 away
    p = np.array([[0, 0, 0], [1, 0, 0], [0, np.sqrt(0.99), 0], [0.5, 0, 0]], np.float32)
    ref.check_farthest_f64(p, [0, 1, 2])
    with pytest.raises(AssertionError, match="pick 1"):
        ref.check_farthest_f64(p, [0, 2, 1])
    with pytest.raises(AssertionError, match="first pick"):
        ref.check_farthest_f64(p, [1, 0, 2])
    # on a cloud: each pick of a good chain in turn replaced by the point nearest to 0.99 of the maximum, where the cloud has one
    for family, n in (("cube", 1023), ("road", 4097), ("line", 1025)):
        xyz = cases.cloud(family, n)
        good = ref.fps_f32(xyz, 48)
        p64 = xyz.astype(np.float64)
        td = np.full(n, ref.START)
        rejected = 0
        for s in range(1, 48):
            td = np.minimum(td, ((p64 - p64[good[s - 1]]) ** 2).sum(1))
            swap = int(np.argmin(np.abs(td - 0.99 * td.max())))
            if not 0.98 * td.max() < td[swap] < 0.995 * td.max():
                continue
            bad = good.copy()
            bad[s] = swap
            with pytest.raises(AssertionError, match=f"pick {s} "):
                ref.check_farthest_f64(xyz, bad[:s + 1])
            rejected += 1
        assert rejected >= 10, (family, n, rejected)


@pytest.mark.parametrize("run", SLAB_RUNS, ids=[r[0] for r in SLAB_RUNS])
def test_slab_model_is_plain_fps(run):
    rid, families, n, k = run
    for b, f in enumerate(families):
        picks, touched = model(f, n, k, 0)
        np.testing.assert_array_equal(picks, want(rid)[b])
        assert 0.0 <= touched <= 1.0


@pytest.mark.parametrize("run", ELONGATED_SLAB_RUNS, ids=[r[0] for r in ELONGATED_SLAB_RUNS])
def test_the_skip_decides_on_the_elongated_families(run):
    """Measured: line 0.23 / 0.10 / 0.10 / 0.07 / 0.07 / 0.06, road 0.26 / 0.14 / 0.14 / 0.11 / 0.11 / 0.10, comb 0.23 / 0.10 / 0.10 /
    0.07 / 0.07 / 0.06, clusters 0.296 / 0.20 / 0.20 / 0.18 / 0.18 / 0.17 at n = 1 025 / 4 096 / 4 097 / 8 192 / 8 193 / 16 384 (a cube:
    0.61 to 0.66)."""
    _, (family,), n, k = run
    touched = model(family, n, k, 0)[1]
    print(f"{run[0]}: touched {touched:.3f}")
    assert touched < 0.3


@pytest.mark.parametrize("slots", [16, 32, 64])
def test_narrowed_bounds_change_the_picks(slots):
    """Every bound pulled in by 8 bins changes the picks on these cases, so a kernel with such a bound fails their GPU test."""
    changed = []
    for rid, (family,), n, k in ELONGATED_SLAB_RUNS:
        if cases.slab_slots(n) == slots and not np.array_equal(model(family, n, k, 8)[0], want(rid)[0]):
            changed.append(rid)
    print(slots, changed)
    assert {rid.split("-")[0] for rid in changed} >= {"line", "comb", "clusters"}, changed


@pytest.mark.parametrize("slots", [16, 32, 64])
def test_the_next_slabs_bounds_change_the_picks(slots):
    """Slab j skipping by slab j + 1's bounds changes the picks of every elongated case within the first three."""
    for rid, (family,), n, k in ELONGATED_SLAB_RUNS:
        if cases.slab_slots(n) == slots:
            picks = ref.slab_model(cases.cloud(family, n), 8, shift=1)[0]
            assert not np.array_equal(picks[:3], want(rid)[0][:3]), rid


PLAIN_RUNS = [r for r in cases.RUNS if not cases.is_slab(r[2])]


@pytest.mark.parametrize("run", PLAIN_RUNS, ids=[r[0] for r in PLAIN_RUNS])
def test_plain_model_is_plain_fps(run):
    """The thread / wave / workgroup arg-max as fps_kernel states it is the first maximum; and an empty slot holding 0 instead of -1
    changes nothing on any case (it ties only when every point is at 0, and then every point has a lower index): the -1 is a margin."""
    rid, families, n, k = run
    k = min(k, 64)
    for b, f in enumerate(families):
        np.testing.assert_array_equal(ref.plain_model(cases.cloud(f, n), k), want(rid)[b][:k])
        np.testing.assert_array_equal(ref.plain_model(cases.cloud(f, n), k, empty=0.0), want(rid)[b][:k])


@pytest.mark.parametrize("n", cases.PLAIN_ONE_PER_KERNEL)
def test_a_wrong_plain_arg_max_changes_the_picks_of_the_tie_cases(n):
    """>= in the thread's walk: the last of a thread's equal slots wins, seen by tie_slots (one slot per thread at 1 024: nothing to see).
    The wave's lowest index taken over all its threads, not those holding the maximum: seen by every case, tie_lanes at pick 1."""
    if n > cases.PLAIN_THREADS:
        xyz, idx = cases.cloud("tie_slots", n), cases.tie_indices("tie_slots", n)
        assert ref.plain_model(xyz, 2, strict=False)[1] == idx[-1] != ref.fps_f32(xyz, 2)[1] == idx[0]
    for family in ("tie_lanes", "tie_waves"):
        xyz = cases.cloud(family, n)
        assert ref.plain_model(xyz, 2, filtered=False)[1] != ref.fps_f32(xyz, 2)[1], family


def _maxima_per_step(xyz, picks):
    """float32 running distances along `picks`: -> the set of points holding the maximum at each step 1 .. len(picks) - 1"""
    out = []
    td = np.full(len(xyz), ref.F(ref.START), ref.F)
    for s in range(1, len(picks)):
        d = xyz - xyz[picks[s - 1]]
        td = np.minimum(td, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        out.append(set(np.flatnonzero(td == td.max()).tolist()))
    return out


@pytest.mark.parametrize("run", TIE_RUNS, ids=[r[0] for r in TIE_RUNS])
def test_tie_cases_tie_where_they_say(run):
    rid, (family,), n, k = run
    xyz = cases.cloud(family, n)
    cand = cases.tie_indices(family, n)
    c = len(cand)
    assert c >= 2 and cand == sorted(set(cand)) and 0 < cand[0] and cand[-1] < n and k > c
    picks = want(rid)[0]
    assert picks[1:c + 1].tolist() == cand  # lowest index first
    maxima = _maxima_per_step(xyz, picks)
    for s in range(1, c):  # steps 1 .. c - 1 are exact ties between all candidates still unpicked
        assert maxima[s - 1] == set(cand[s - 1:]), (s, maxima[s - 1])
    cand = np.array(cand)
    thread, slot = cand % cases.PLAIN_THREADS, cand // cases.PLAIN_THREADS
    lane, wave = thread % 64, thread // 64
    if family == "tie_slots":  # (a) register slots of one thread
        assert len(set(thread)) == 1 and len(set(slot)) == c and slot.max() == (n - 1 - cand[0]) // cases.PLAIN_THREADS
    elif family == "tie_lanes":  # (b) lanes of one wave, the same slot
        assert len(set(wave)) == 1 and len(set(slot)) == 1 and len(set(lane)) == c
    elif family == "tie_waves":  # (c) waves, the same lane and slot
        assert len(set(lane)) == 1 and len(set(slot)) == 1 and len(set(wave)) == c
    else:
        bins, _, _ = ref.slab_bins(xyz)
        order, slab_of_pos, _, _ = ref.slab_layout(xyz)
        pos = np.empty(n, np.int64)
        pos[order] = np.arange(n)
        if family == "tie_slabs":  # several slabs, and the winner (lowest index) in the last of them
            slabs = slab_of_pos[pos[cand]]
            assert len(set(slabs)) >= 3 and slabs[0] == slabs.max() == (n - 1) // ref.SLAB_THREADS and slabs.min() == 0
        else:  # one bin, larger than a slab: wherever the scatter puts the candidates inside it, the lowest original index must win
            assert len(set(bins[cand])) == 1
            run_pos = pos[bins == bins[cand[0]]]
            assert len(run_pos) > ref.SLAB_THREADS and slab_of_pos[run_pos.min()] < slab_of_pos[run_pos.max()]

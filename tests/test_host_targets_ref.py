"""Host: tests/targets_ref.py against hand-worked tables and against the project's fp32 route on the CPU (oracle.box_iou_rotated -- the
plain-C restatement of the IoU core -- + ops.Matcher + box_encode.encode, all pure torch), and every case of tests/targets_cases.py
against the property it is named for.  What this file establishes for tests/test_gpu_targets_edges.py:
  * the float64 reference and the fp32 route give the same labels and matches on every case;
  * every margin of every case -- best IoU to a band edge, best to second-best ground truth, a ground truth's maximum to the next
    anchor -- is exactly 0 by construction (the band cases, the twin ground truths of first_max) or at least 1e-5, the margin the NMS
    fixtures demand (tests/test_gpu_iou_nms.py), AND at least ten times the largest difference between the fp32 and the float64 IoU
    of the case; the GPU test therefore leaves out no anchor;
  * the named ties are exact in both arithmetics, the duplicate anchors attain the maximum, the crowd's matches start at 128, ...;
  * each single-line mutation of the reference (targets_ref's keyword switches) changes the result of a named case: a kernel with the
    same mistake fails that case's GPU test.  Which case notices which:
      `<=` at lo                          band-at_lo            `<=` at hi                 band-at_hi
      `>=` in the arg-max                 first_max, first_max-reversed
      ties dropped from the rule          low_quality-dup_anchors
      the zero row left out of the rule   low_quality-far_gt
      staging cut at 128                  crowd-129, crowd-200, crowd-257, crowd-mixed (crowd-128: no change)
      the direction loop's second trip    direction n = 262 145 and 300 000 (262 144: no change)
      remainder with the dividend's sign  encode-yaw
"""
import numpy as np
import pytest
import torch

import direction_cases
import direction_ref
import targets_cases as cases
import targets_ref as ref

MARGIN = 1e-5


def want(name, low_quality=None):
    return cases.reference(name, cases.case(name)["low_quality"] if low_quality is None else low_quality)


def fp32_route(oracle, c, low_quality):
    """core/proposal_targets.py's forward_torch on the CPU, the IoU from the oracle -> labels, matches (n_cls, A), the IoU matrices"""
    from vision3d_amd.ops import Matcher
    n_cls, A = c["anchors"].shape[:2]
    labels, matches, ious = np.zeros((n_cls, A), np.int64), np.zeros((n_cls, A), np.int64), []
    for k in range(n_cls):
        idx = np.flatnonzero(c["gt_class"] == k)
        iou = oracle.box_iou_rotated(c["gt"][idx][:, ref.BEV], c["anchors"][k][:, ref.BEV]).reshape(len(idx), A)
        ious.append(iou)
        m, lab = Matcher([float(t) for t in c["thresh"][k]], [0, -1, +1], low_quality)(torch.from_numpy(iou))
        labels[k] = lab.numpy()
        matches[k] = idx[m.numpy()] if len(idx) else 0
    return labels, matches, ious


# ------------------------------------------------------------------------------------------------------------------ hand tables
def test_match_on_a_table_worked_by_hand():
    #             a0    a1    a2    a3
    iou = [[0.70, 0.30, 0.50, 0.00],   # ground truth 0: maximum 0.70 at a0
           [0.20, 0.30, 0.50, 0.00]]   # ground truth 1: maximum 0.50 at a2
    # best        0.70  0.30  0.50  0.00;  first arg-max 0, 0 (tie), 0 (tie), 0 (tie);  bands [0.3, 0.6): +1, -1, -1, 0
    labels, matches = ref.match(iou, 0.3, 0.6, False)
    assert labels.tolist() == [1, -1, -1, 0] and matches.tolist() == [0, 0, 0, 0]
    labels, matches = ref.match(iou, 0.3, 0.6, True)  # a0 attains row 0's maximum, a2 row 1's
    assert labels.tolist() == [1, -1, 1, 0] and matches.tolist() == [0, 0, 0, 0]
    labels, _ = ref.match([[0.0, 0.0, 0.0], [0.1, 0.4, 0.1]], 0.3, 0.6, True)  # a row of zeros: every anchor attains it
    assert labels.tolist() == [1, 1, 1]
    labels, matches = ref.match(np.zeros((0, 3)), 0.3, 0.6, True)
    assert labels.tolist() == [0, 0, 0] and matches.tolist() == [0, 0, 0]
    # the mutations, on the same table
    assert ref.match(iou, 0.3, 0.6, False, lo_closed=False)[0].tolist() == [1, 0, -1, 0]
    assert ref.match(iou, 0.3, 0.5, False, hi_closed=False)[0].tolist() == [1, -1, -1, 0]
    assert ref.match(iou, 0.3, 0.5, False)[0].tolist() == [1, -1, 1, 0]
    assert ref.match(iou, 0.3, 0.6, False, strict=False)[1].tolist() == [0, 1, 1, 1]
    assert ref.match([[0.2, 0.2]], 0.3, 0.6, True, ties=False)[0].tolist() == [1, 0]
    assert ref.match([[0.0, 0.0, 0.0], [0.1, 0.4, 0.1]], 0.3, 0.6, True, zero_row=False)[0].tolist() == [0, 1, 0]


def test_iou_of_the_containment_and_of_a_turn_read_as_degrees(oracle):
    a = np.array([[0, 0, 0, 2, 2, 1.5, 0]], np.float32)
    g = np.array([[0.5, 0.5, 0, 4, 4, 1.5, 0]], np.float32)
    assert ref.bev_iou(g, a)[0, 0] == 0.25 == oracle.box_iou_rotated(g[:, ref.BEV], a[:, ref.BEV])[0, 0]
    # a unit square turned by "45" about its centre against itself: the octagon, 2 (sqrt 2 - 1) of the square; IoU = that / (2 - that)
    sq = np.array([[3, -2, 0, 1, 1, 1, 0]], np.float32)
    turned = sq.copy()
    turned[0, 6] = 45.0
    octagon = 2 * (np.sqrt(2) - 1)
    assert abs(ref.bev_iou(turned, sq)[0, 0] - octagon / (2 - octagon)) < 1e-12
    turned[0, 6] = np.float32(np.pi / 4)  # radians read as degrees: 0.785 degrees, hardly a turn
    assert ref.bev_iou(turned, sq)[0, 0] > 0.97


def test_encode_worked_by_hand():
    anchor = np.array([[1.0, 2.0, -1.0, 3.0, 4.0, 2.0, 0.5]], np.float32)       # diag = 5
    box = np.array([[2.0, 0.0, 0.0, 6.0, 1.0, 2.0, -0.25]], np.float32)         # yaw difference -0.75 -> pi - 0.75
    got = ref.encode(box, anchor)[0]
    want = [0.2, -0.4, 0.5, np.log(2.0), np.log(0.25), 0.0, ref.PI32 - 0.75]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
    assert ref.encode(box, anchor, wrap_sign="dividend")[0, 6] == -0.75
    for d, r in ((0.0, 0.0), (ref.PI32, 0.0), (-ref.PI32, 0.0), (2 * ref.PI32, 0.0), (-1e-7, ref.PI32 - float(np.float32(1e-7)))):
        box[0, 6], anchor[0, 6] = d, 0.0
        assert abs(ref.encode(box, anchor)[0, 6] - r) < 1e-15, d


# ------------------------------------------------------------------------------------------- the reference is the project's route
@pytest.mark.parametrize("run", cases.RUNS, ids=cases.RUN_IDS)
def test_reference_agrees_with_the_fp32_route_and_has_its_margins(oracle, run):
    from vision3d_amd.core.box_encode import encode
    name, low_quality = run
    c, w = cases.case(name), want(*run)
    labels, matches, ious = fp32_route(oracle, c, low_quality)
    np.testing.assert_array_equal(labels, w["labels"])
    np.testing.assert_array_equal(matches, w["matches"])
    err = max([float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(ious, w["iou"]) if b.size] + [0.0])
    print(f"{cases.RUN_IDS[cases.RUNS.index(run)]}: fp32 IoU within {err:.2e}; band {w['band']:.2e} gt_gap {w['gt_gap']:.2e} "
          f"row_gap {w['row_gap']:.2e}; {int(w['M_reg'].sum())} positives, {int((~w['M_cls']).sum())} ignored")
    # fp32 against float64: 3e-7 at most where the boxes are turned by a few "degrees"; 1.1e-5 on ONE pair of crowd-mixed, a sliver (IoU
    # 0.0017) between edges 0.2 degrees from parallel -- the algorithm's own conditioning, the reference's core gives the same bits
    floor = max(MARGIN, 10 * err)
    exact_band = name.startswith("band-")
    exact_gap = name.startswith("first_max")
    assert w["band"] >= floor or (exact_band and w["band"] <= 2.0 ** -25)  # at the edge, or one float32 step (2^-25) under it
    assert w["gt_gap"] >= floor or (exact_gap and w["gt_gap"] == 0.0)
    assert w["row_gap"] >= floor
    pos = w["M_reg"]
    torch_reg = encode(torch.from_numpy(c["gt"][w["matches"][pos]]), torch.from_numpy(c["anchors"][pos])).numpy() if pos.any() else np.zeros((0, 7))
    np.testing.assert_allclose(torch_reg, w["G_reg"][pos], rtol=1e-5, atol=1e-6)
    assert not w["G_reg"][~pos].any()
    if "cfg" in c:  # the direction bit of every ground truth that a positive reads is clear
        used = np.unique(w["matches"][pos])
        assert (direction_ref.bin_edge_distance(c["gt"][used, 6].astype(np.float64)) >= direction_cases.BIN_MARGIN).all()


# ------------------------------------------------------------------------------------------------------ every case is what it says
def test_the_runs_cover_the_issue():
    assert [cases.case(n)["anchors"].shape[1] for n in cases.GRID] == [1, 63, 64, 65, 255, 256, 257, 513]
    assert all(cases.case(n)["low_quality"] for n in cases.GRID + cases.LOW_QUALITY + ["crowd-mixed", "encode-size", "stale-high", "stale-low"])
    assert {n for n, lq in cases.RUNS if not lq} >= set(cases.LOW_QUALITY)
    assert [len(cases.case(f"crowd-{n}")["gt"]) for n in cases.CROWD_SIZES] == [128, 129, 200, 257]
    assert all(cases.case(n)["anchors"].shape[1] == 70 and "cfg" in cases.case(n) for n in cases.CROWD)


@pytest.mark.parametrize("name", cases.GRID)
def test_grid_cases(name):
    c, w = cases.case(name), want(name)
    A = c["anchors"].shape[1]
    assert len(c["gt"]) == 3 and (c["gt_class"] == 0).all() and w["M_reg"].sum() >= 1
    assert (w["iou"][0].max(1) > 0).all(), "every ground truth overlaps an anchor"
    if A >= 257:  # ground truth 0's two best anchors: 255 and 256, in different workgroups; the rule marks exactly the better one
        two = np.argsort(w["iou"][0][0])[-2:]
        assert sorted(two.tolist()) == [255, 256] and two[0] // ref.BLOCK != two[1] // ref.BLOCK
        assert w["M_reg"][0, two[1]]
    if A > 1:
        top = int(np.argmax(w["iou"][0][2]))  # ground truth 2 is positive by the low-quality rule alone
        assert w["iou"][0][2, top] < c["thresh"][0, 0] and w["M_reg"][0, top] and not want(name, False)["M_reg"][0, top]


@pytest.mark.parametrize("which", list(cases.BAND))
def test_band_cases_sit_on_the_edge_in_both_arithmetics(oracle, which):
    c, w = cases.case(f"band-{which}"), want(f"band-{which}")
    thresh, label = cases.BAND[which]
    n = len(cases.BAND_SHIFTS)
    q32 = oracle.box_iou_rotated(c["gt"][:, ref.BEV], c["anchors"][0][:, ref.BEV])
    assert (np.diag(q32) == np.float32(0.25)).all() and (np.diag(w["iou"][0]) == 0.25).all()
    assert not (q32 - np.diag(np.diag(q32))).any() and not (w["iou"][0] - np.diag(np.diag(w["iou"][0]))).any()
    assert w["labels"].tolist() == [[label] * n]
    assert np.float32(0.25) in c["thresh"][0] or np.nextafter(np.float32(0.25), np.float32(1)) in c["thresh"][0]
    assert w["matches"].tolist() == [list(range(n))]


def test_first_max_cases_tie_exactly(oracle):
    a, b = cases.case("first_max"), cases.case("first_max-reversed")
    wa, wb = want("first_max"), want("first_max-reversed")
    assert a["gt_class"].tolist() == [0, 1, 0]
    np.testing.assert_array_equal(a["gt"][[2, 1, 0]], b["gt"])  # the twins swapped
    np.testing.assert_array_equal(a["gt"][0, ref.BEV], a["gt"][2, ref.BEV])
    assert a["gt"][0, 2] != a["gt"][2, 2] and a["gt"][0, 5] != a["gt"][2, 5]
    for c, w in ((a, wa), (b, wb)):
        np.testing.assert_array_equal(w["iou"][0][0], w["iou"][0][1])
        q32 = oracle.box_iou_rotated(c["gt"][[0, 2]][:, ref.BEV], c["anchors"][0][:, ref.BEV])
        np.testing.assert_array_equal(q32[0], q32[1])
        assert w["M_reg"][0].sum() >= 1 and w["M_reg"][1].sum() >= 1
        assert (w["matches"][0] == 0).all(), "the lower input index, never 2"
        assert (w["matches"][1] == 1).all()
    # the match index stays with the input position: what is matched swaps with the twins, and shows in the z and h targets alone
    pos = wa["M_reg"][0]
    np.testing.assert_array_equal(pos, wb["M_reg"][0])
    np.testing.assert_array_equal(wa["G_reg"][0][pos][:, [0, 1, 3, 4, 6]], wb["G_reg"][0][pos][:, [0, 1, 3, 4, 6]])
    assert (wa["G_reg"][0][pos][:, [2, 5]] != wb["G_reg"][0][pos][:, [2, 5]]).all()


@pytest.mark.parametrize("n_cls", [3, 16])
def test_interleaved_cases(n_cls):
    c, w = cases.case(f"interleaved-c{n_cls}"), want(f"interleaved-c{n_cls}")
    cls = c["gt_class"]
    assert c["anchors"].shape[0] == n_cls and set(cls.tolist()) == (set(range(n_cls)) - {1}) | {-1, n_cls}
    assert (np.diff(cls) < 0).any() and (np.diff(cls) > 0).any(), "the input is not sorted by class"
    assert not w["labels"][1].any() and not w["matches"][1].any(), "the empty class: label 0, match 0"
    outsiders = set(np.flatnonzero((cls < 0) | (cls >= n_cls)).tolist())
    assert len(outsiders) == 4 and not outsiders & set(w["matches"].reshape(-1).tolist())
    for k in range(n_cls):
        if k != 1:
            idx = np.flatnonzero(cls == k)
            assert len(idx) == 2 and idx[1] >= 2, "the second ground truth's input index is not its position in the class"
            assert set(w["matches"][k][w["M_reg"][k]].tolist()) == set(idx.tolist()), k


def test_low_quality_cases(oracle):
    lo = cases.CAR_THRESH[0]
    for which in ("clear", "dup_anchors", "far_gt"):
        c, on, off = cases.case(f"low_quality-{which}"), want(f"low_quality-{which}", True), want(f"low_quality-{which}", False)
        iou = on["iou"][0]
        top = int(np.argmax(iou[1]))
        assert top == 3 and MARGIN < iou[1, 3] < lo - MARGIN and iou[0].max() > cases.CAR_THRESH[1]
        assert on["M_reg"][0, 3] and on["matches"][0, 3] == 1 and not off["M_reg"][0, 3] and off["M_reg"].sum() == 1
        if which == "clear":
            assert on["M_reg"].sum() == 2
        if which == "dup_anchors":
            q32 = oracle.box_iou_rotated(c["gt"][:, ref.BEV], c["anchors"][0][:, ref.BEV])
            assert c["anchors"][0][3].tobytes() == c["anchors"][0][300].tobytes() and 3 // ref.BLOCK != 300 // ref.BLOCK
            assert iou[1, 3] == iou[1, 300] == iou[1].max() and q32[1, 3] == q32[1, 300] == q32[1].max()
            assert np.flatnonzero(on["M_reg"][0]).tolist() == sorted([3, 300, int(np.argmax(iou[0]))])
        if which == "far_gt":
            assert not iou[2].any() and on["M_reg"].all() and on["G_cls"].all()
            d = np.linalg.norm(c["anchors"][0][:, :2].astype(np.float64) - c["gt"][2, :2], axis=1)
            assert d.min() > 50 > 10 * np.hypot(*cases.CAR[:2]), "far beyond the sum of the circumradii, in any arithmetic"
            assert set(on["matches"][0].tolist()) == {0, 1}, "an anchor that overlaps nothing takes the first ground truth"
    on, off = want("low_quality-below_lo", True), want("low_quality-below_lo", False)
    assert (on["iou"][0].max(1) < lo - MARGIN).all() and not off["M_reg"].any() and on["M_reg"].sum() == 2


@pytest.mark.parametrize("n", cases.CROWD_SIZES)
def test_crowd_cases_decide_on_the_last_ground_truth(n):
    c, w = cases.case(f"crowd-{n}"), want(f"crowd-{n}")
    assert len(c["gt"]) == n and (c["gt_class"] == 0).all() and not c["low_quality"]
    assert w["M_reg"].sum() >= 4 and (~w["M_cls"]).sum() >= 1
    assert (w["matches"][w["M_reg"]] == n - 1).all() and (n - 1 >= 128) == (n > 128)
    assert not w["iou"][0][:-1].any(), "no other ground truth reaches the grid"
    cut = ref.assign(c["gt"], c["gt_class"], c["anchors"], c["thresh"], False, stage_limit=128)
    assert (not cut["M_reg"].any()) == (n > 128), "a staging cut at 128 loses every positive"


def test_crowd_mixed_case():
    c, w = cases.case("crowd-mixed"), want("crowd-mixed")
    cls = c["gt_class"]
    assert np.bincount(cls).tolist() == [130, 30, 40] and (np.diff(cls) != 0).sum() > 20
    assert all((q.max(1) > MARGIN).all() for q in w["iou"]), "every ground truth overlaps an anchor: no maximum is 0"
    ordinal = np.cumsum(cls == 0) - 1
    hit = ordinal[w["matches"][0][w["M_reg"][0]]]
    assert (hit < 128).any() and (hit >= 128).any(), "positives matched on both sides of the staging limit"
    assert w["M_reg"].sum() > want("crowd-mixed", False)["M_reg"].sum() > 0, "some positives by the low-quality rule alone"
    late = np.flatnonzero(cls == 0)[128:]
    by_rule = w["M_reg"][0] & ~want("crowd-mixed", False)["M_reg"][0]
    assert np.isin(w["iou"][0][128:].argmax(1), np.flatnonzero(by_rule)).any(), "one of them for a ground truth past the limit"
    assert len(late) == 2


def test_encode_cases():
    c, w = cases.case("encode-yaw"), want("encode-yaw")
    n = len(cases.YAW_DIFFS)
    assert w["M_reg"].all() and w["matches"].tolist() == [list(range(len(c["gt"])))]
    d = c["gt"][:, 6] - c["anchors"][0][:, 6]
    np.testing.assert_array_equal(d[:n], np.asarray(cases.YAW_DIFFS, np.float32))
    assert d[n] == np.float32(ref.PI32) or abs(float(d[n]) - ref.PI32) < 5e-7  # (base + pi) - base, both float32
    got = w["G_reg"][0][:, 6]
    assert (got >= 0).all() and (got <= ref.PI32).all()
    assert got[0] == 0 and got[2] == 0 and got[3] == 0 and got[4] == 0 and got[5] == 0 and abs(got[1] - ref.PI32) < 2e-7
    assert abs(got[6] - (3.5 - ref.PI32)) < 1e-6 and abs(got[7] - (2 * ref.PI32 - 3.5)) < 1e-6
    assert not w["G_reg"][0][:, :6].any(), "the boxes sit on their anchors"
    c, w = cases.case("encode-size"), want("encode-size")
    assert w["M_reg"].all() and not want("encode-size", False)["M_reg"].any(), "positive by the low-quality rule alone"
    ratio = c["gt"][:, 3:6].astype(np.float64) / c["anchors"][0][:, 3:6]
    np.testing.assert_allclose(ratio, cases.SIZE_RATIOS, rtol=1e-6)
    np.testing.assert_allclose(w["G_reg"][0][:, 3:6], np.log(cases.SIZE_RATIOS), atol=1e-6)
    assert ratio.min() < 0.126 and ratio.max() > 7.9


def test_stale_and_empty_cases():
    hi, lo = cases.case("stale-high"), cases.case("stale-low")
    assert hi["gt"].shape == lo["gt"].shape and hi["anchors"].tobytes() == lo["anchors"].tobytes()
    wh, wl = want("stale-high"), want("stale-low")
    assert (wh["iou"][0].max(1) > wl["iou"][0].max(1) + 0.3).all(), "maxima left from the first frame are above everything in the second"
    assert wl["M_reg"].sum() == 2 and not want("stale-low", False)["M_reg"].any()
    e, w = cases.case("empty"), want("empty")
    assert e["gt"].shape == (0, 7) and not w["labels"].any() and not w["matches"].any() and not w["G_reg"].any() and w["M_cls"].all()


@pytest.mark.parametrize("n", cases.DIRECTION_SIZES)
def test_direction_cases(n):
    c = cases.direction_case(n)
    blocks = min(ref.DIRECTION_MAX_BLOCKS, -(-n // ref.BLOCK))
    assert (n > blocks * ref.BLOCK) == (n > 262144), "the second trip of the loop"
    assert c["matches"][-1] in cases.BAD_MATCHES and c["m_reg"][-1]
    w = ref.direction(c["gt"], c["matches"], c["m_reg"])
    assert w.dtype == np.int8 and w[-1] == 0
    bad = (c["matches"] < 0) | (c["matches"] >= cases.DIRECTION_N_GT)
    assert not w[bad].any() and not w[~c["m_reg"]].any()
    if n > 1:
        assert w[-2] == 1 and set(w.tolist()) == {0, 1} and set(c["matches"][bad].tolist()) <= set(cases.BAD_MATCHES)
    if n >= 255:
        assert set(c["matches"][bad].tolist()) == set(cases.BAD_MATCHES) and (bad & c["m_reg"]).any() and (~c["m_reg"]).any()
    np.testing.assert_array_equal(ref.direction_strided(c["gt"], c["matches"], c["m_reg"]), w)
    # the float32 statement of the bit (core/proposal_targets.py direction_bit) agrees: the yaws are clear of the bin edges
    from vision3d_amd.core.proposal_targets import direction_bit
    bits32 = direction_bit(torch.from_numpy(c["gt"][:, 6].copy()), direction_ref.OFFSET).numpy()
    np.testing.assert_array_equal(bits32, direction_ref.bit(c["gt"][:, 6].astype(np.float64)).astype(bool))


# ------------------------------------------------------------------------------------------------------------------- mutations
def _mutated(name, **mutation):
    c = cases.case(name)
    return ref.assign(c["gt"], c["gt_class"], c["anchors"], c["thresh"], c["low_quality"], **mutation)


def _differs(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in ("G_cls", "M_cls", "M_reg", "matches", "G_reg"))


@pytest.mark.parametrize("mutation, noticed_by, blind", [
    (dict(lo_closed=False), ["band-at_lo"], ["band-at_hi", "band-above_lo"]),
    (dict(hi_closed=False), ["band-at_hi"], ["band-at_lo", "band-above_hi"]),
    (dict(strict=False), ["first_max", "first_max-reversed"], []),  # (any anchor that overlaps nothing ties at 0: every case sees it)
    (dict(ties=False), ["low_quality-dup_anchors"], ["low_quality-clear"]),
    (dict(zero_row=False), ["low_quality-far_gt"], ["low_quality-clear", "low_quality-dup_anchors"]),
    (dict(stage_limit=128), ["crowd-129", "crowd-200", "crowd-257", "crowd-mixed"], ["crowd-128"]),
    (dict(wrap_sign="dividend"), ["encode-yaw"], ["band-at_hi"]),
], ids=["lo<=", "hi<=", "argmax>=", "no_ties", "no_zero_row", "stage128", "fmod"])
def test_each_mutation_of_the_reference_is_noticed(mutation, noticed_by, blind):
    for name in noticed_by:
        assert _differs(_mutated(name, **mutation), want(name)), name
    for name in blind:  # and the mutation is what the case sees, not the harness
        assert not _differs(_mutated(name, **mutation), want(name)), name


def test_a_direction_loop_without_its_second_trip_is_noticed():
    for n in cases.DIRECTION_SIZES:
        c = cases.direction_case(n)
        full = ref.direction_strided(c["gt"], c["matches"], c["m_reg"])
        once = ref.direction_strided(c["gt"], c["matches"], c["m_reg"], trips=1)
        assert np.array_equal(full, once) == (n <= 262144), n

"""CPU only: the float64 statement of the proposal stage (tests/proposal_ref.py) agrees with the statements the project already
has, and every case of tests/test_gpu_proposal_edges.py is well-posed ON THE REFERENCE ALONE -- scores separated by 64 ulps or
bit-equal, every NMS decision at least 1e-5 away from its threshold, the survivor share, and the property each hand-built case
is named for.  The GPU tests assert nothing about their inputs that is not asserted here first."""
import numpy as np
import pytest
import torch

import proposal_cases as C
import proposal_ref as R


# csrc/proposal.hip, prop_run: how a group's n anchors are cut into level-1 slices (restated here, not imported, on purpose)
def level1_slicing(n, topk):
    chunks = 40
    while chunks > 1 and (chunks * topk > 4 * 1024 or n // chunks < 4 * topk):
        chunks -= 1
    chunk_len = ((n + chunks - 1) // chunks + 63) & ~63
    return chunks, chunk_len, [max(0, min(n, (c + 1) * chunk_len) - min(n, c * chunk_len)) for c in range(chunks)]


def test_slicing_of_the_table():
    """The slicing column of the table: which branch of the level-1 split each row is there for."""
    want = {
        (1, 2, 5, 10): (1, 64, [10]),
        (2, 7, 9, 10): (3, 64, [64, 62, 0]),
        (1, 9, 29, 16): (4, 128, [128, 128, 5, 0]),
        (2, 5, 13, 1): (32, 64, [64, 64, 2] + [0] * 29),
        (2, 24, 24, 64): (4, 320, [320, 320, 320, 192]),
        (2, 24, 24, 65): (4, 320, [320, 320, 320, 192]),
        (2, 40, 40, 256): (3, 1088, [1088, 1088, 1024]),
        (2, 40, 40, 257): (3, 1088, [1088, 1088, 1024]),
        (2, 60, 60, 300): (6, 1216, [1216] * 5 + [1120]),
        (1, 64, 64, 1024): (1, 4096, [4096]),
        (1, 181, 181, 1024): (4, 8192, [8192, 8192, 8192, 8185]),
        (2, 288, 288, 100): (40, 4160, [4160] * 39 + [3648]),
    }
    assert list(want) == C.SELECT_ROWS
    for (n_yaw, H, W, topk), (chunks, chunk_len, lens) in want.items():
        assert level1_slicing(n_yaw * H * W, topk) == (chunks, chunk_len, lens), (n_yaw, H, W, topk)
    over_4096 = [r for r in C.SELECT_ROWS if level1_slicing(r[0] * r[1] * r[2], r[3])[1] > 4096]
    assert over_4096 == C.SELECT_ROWS[10:], "rows 11 and 12 (and only they) take the 8-elements-per-thread instantiation"
    assert level1_slicing(181 * 181, 1024)[0] * 1024 == 4096, "a merge of exactly 4 x 1024 rows"
    # the acceptance edge: 40 full slices of exactly 8192; one more W column passes the 8192 a workgroup holds
    n_yaw, H, W = C.EDGE_SHAPE
    assert n_yaw * H * W == 327680 and level1_slicing(n_yaw * H * W, C.EDGE_TOPK)[1:] == (8192, [8192] * 40)
    assert level1_slicing(n_yaw * H * (W + 1), C.EDGE_TOPK)[1] > 8192


def test_native_supported_agrees_with_the_acceptance_edge():
    from vision3d_amd.core.config import second_car_cfg
    from vision3d_amd.detector.proposal import ProposalLayer
    cfg = second_car_cfg()
    assert cfg.PROPOSAL.TOPK == C.EDGE_TOPK
    head = ProposalLayer(cfg)
    n_yaw, H, W = C.EDGE_SHAPE
    assert head.native_supported(1, n_yaw * H * W) and not head.native_supported(1, n_yaw * H * (W + 1))


def test_select_topk_equals_torch_topk_without_ties():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 3, 5000)) - 3.0).astype(np.float32)
    sig = torch.from_numpy(x).sigmoid()
    top = sig.topk(41, -1)[0]
    assert bool((top[..., :-1] > top[..., 1:]).all()), "tie-free in the top-k"
    want_s, want_i = sig.topk(40, -1)
    idx, sc = R.select_topk(x, 40)
    np.testing.assert_array_equal(idx, want_i.numpy())
    np.testing.assert_allclose(sc, want_s.numpy(), rtol=1e-6, atol=0)


def test_select_topk_orders_ties_by_index():
    x = np.array([[1.0, 30.0, 1.0, 20.0, -110.0, 0.0, -0.0, 1.0, -120.0]], np.float32)
    idx, sc = R.select_topk(x, 9)
    np.testing.assert_array_equal(idx[0], [1, 3, 0, 2, 7, 5, 6, 4, 8])
    assert sc[0, 0] == sc[0, 1] == 1.0 and sc[0, 5] == sc[0, 6] == 0.5 and sc[0, 7] == sc[0, 8] == 0.0


def test_minus_100_is_a_denormal_under_the_float64_formula():
    """Why the zero pair of the special values is -110 / -120: float32(1 / (1 + exp(100.0))) is a non-zero denormal (float32
    arithmetic gives 0.0: expf(100) overflows), closer than 64 ulps to the 0.0 of -110 -- not a separated input."""
    assert 0.0 < R.score(np.float32(-100.0)) < 1e-43
    assert R.score(np.float32(-110.0)) == 0.0 and R.score(np.float32(-120.0)) == 0.0
    assert R.score(np.float32(20.0)) == 1.0 and R.score(np.float32(30.0)) == 1.0
    with pytest.raises(AssertionError):
        R.assert_separated(np.array([-100.0, -110.0], np.float32))


def test_decode_equals_the_package_decode():
    from vision3d_amd.core.box_encode import decode
    rng = np.random.default_rng(6)
    anchors = R.kitti_anchors(rng, 1, 2, 5, 7).reshape(-1, 7)
    deltas = (rng.standard_normal(anchors.shape) * 0.3).astype(np.float32)
    want = decode(torch.from_numpy(deltas).double(), torch.from_numpy(anchors).double()).numpy()
    np.testing.assert_allclose(R.decode(deltas, anchors), want, rtol=1e-14, atol=0)


def test_stage_equals_the_cpu_oracle_without_ties(oracle):
    from oracle import second_cpu
    B, n_cls, n_yaw, H, W, topk = 2, 3, 2, 12, 14, 24
    rng = np.random.default_rng(7)
    n_a = n_cls * n_yaw
    cls = (rng.standard_normal((B, n_a, H, W)) - 1.0).astype(np.float32)
    reg = (rng.standard_normal((B, n_a * 7, H, W)) * 0.3).astype(np.float32)
    anchors = R.kitti_anchors(rng, n_cls, n_yaw, H, W)
    top = torch.from_numpy(cls).sigmoid().reshape(B, n_cls, -1).topk(topk + 1, -1)[0]
    assert bool((top[..., :-1] > top[..., 1:]).all()), "tie-free in the top-k"
    thresh = [0.55, 0.7, 0.8]
    maps = np.concatenate([cls, reg], 1)
    got = R.stage(maps, anchors, B, n_cls, n_yaw, H, W, topk, thresh, 0.01)
    assert R.batched_margin(got["bev"], got["all_scores"], got["groups"], 0.01) > C.MARGIN
    boxes, bi, ci, scores = second_cpu.proposals(cls, reg, anchors, n_cls, n_yaw, 7, topk, thresh)
    assert 0 < len(scores) < got["n_nms"] < B * n_cls * topk, "the NMS and the cut both drop and both keep"
    np.testing.assert_array_equal(got["batch"], bi)
    np.testing.assert_array_equal(got["cls"], ci)
    np.testing.assert_allclose(got["scores"], scores, rtol=1e-6, atol=0)
    np.testing.assert_allclose(got["boxes"], boxes, rtol=1e-5, atol=1e-6)
    # the anchor indices: every output box is the decode of the candidate `cand` names
    idx, _, cand_boxes = R.candidates(maps, anchors, B, n_cls, n_yaw, H, W, topk)
    want_idx = torch.from_numpy(cls).sigmoid().reshape(B, n_cls, -1).topk(topk, -1)[1].numpy()
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(got["boxes"], cand_boxes.reshape(-1, 7)[got["cand"]])


def test_batched_margin_shares_the_oracles_group_offset(oracle):
    """Two identical boxes: IoU 1 in one group (margin 1 - thr), IoU 0 once the offset has moved them apart (margin thr)."""
    b = np.array([[3.0, 4.0, 2.0, 4.0, 0.3]] * 2, np.float32)
    s = np.array([0.9, 0.8], np.float32)
    assert R.batched_margin(b, s, np.array([0, 0]), 0.25) == pytest.approx(0.75)
    assert R.batched_margin(b, s, np.array([0, 1]), 0.25) == pytest.approx(0.25)
    np.testing.assert_array_equal(oracle.batched_nms_rotated(b, s, np.array([0, 1]), 0.25), [0, 1])
    np.testing.assert_array_equal(oracle.batched_nms_rotated(b, s, np.array([0, 0]), 0.25), [0])


# ------------------------------------------------------------------------------------------ the GPU tables are well-posed
@pytest.mark.parametrize("case", C.SELECT_CASES, ids=C.case_id)
def test_select_cases_are_separated(case):
    c = C.select_case(*case)
    R.assert_separated(c["logits"])
    row, B, n_cls, fill = case
    n = row[0] * row[1] * row[2]
    if fill == "specials" and n >= len(R.SPECIALS):
        bits = c["logits"].view(np.uint32)
        for g in bits.reshape(-1, n)[:1]:
            assert set(R.SPECIALS.view(np.uint32)) <= set(g), "every special value (both zeros by sign) is in the map"
    if fill == "lattice":
        s = c["scores"]
        assert (s[..., 1:] == s[..., :-1]).any() or row[3] == 1 or n < 100, "the lattice ties inside the top-k"


@pytest.mark.parametrize("case", C.TIE_CASES, ids=C.case_id)
def test_tie_cases_have_their_property(case):
    row, kind = case
    n_yaw, H, W, topk = row
    c = C.tie_case(*case)
    x = c["logits"].reshape(-1)
    R.assert_separated(x)
    s = R.score(x)
    chunks, chunk_len, lens = level1_slicing(x.size, topk)
    if kind == "straddle":
        s_k = c["scores"][0, 0, topk - 1]  # the score in row K
        n_gt, members = int((s > s_k).sum()), np.flatnonzero(s == s_k)
        assert 0 < n_gt < topk and n_gt + members.size > topk, "the tie class straddles row K below strictly better candidates"
        per_slice = np.bincount(members // chunk_len, minlength=chunks)
        assert (per_slice > 0).sum() >= 2, "its members lie in at least two level-1 slices"
        gt_slice = np.bincount(np.flatnonzero(s > s_k) // chunk_len, minlength=chunks)
        full = np.array(lens) >= topk
        assert (gt_slice + per_slice > topk)[full].all(), "more members than free rows in every full slice: lowest index first there too"
        want = np.concatenate([np.flatnonzero(s > s_k)[np.argsort(-s[s > s_k], kind="stable")], members[:topk - n_gt]])
        np.testing.assert_array_equal(c["idx"][0, 0], want)
    else:
        assert np.unique(s).size == 1 and s[0] == {"all_equal": s[0], "all_zero": 0.0, "signed_zero": 0.5}[kind]
        if kind != "all_equal":
            assert np.unique(x.view(np.uint32)).size == 2, "one score from two different keys"
            assert np.unique(x.view(np.uint32)[:topk]).size == min(2, topk), "both keys among the selected"
        np.testing.assert_array_equal(c["idx"][0, 0], np.arange(topk))
    if row == C.SELECT_ROWS[11]:
        assert chunk_len > 1024, "a slice spans several register slices of the level-1 workgroup"


def test_nonfinite_case_has_its_property():
    c = C.nonfinite_case()
    x = c["logits"].reshape(-1)
    bits = x.view(np.uint32)
    assert (bits == 0x7FC00000).sum() == 6 and (bits == 0xFFC00000).sum() == 6 and np.isposinf(x).sum() == 3 and np.isneginf(x).sum() == 3
    R.assert_separated(R.nan_as_neg_inf(x))
    n_yaw, H, W, topk = C.NONFINITE_ROW
    chunks, chunk_len, lens = level1_slicing(x.size, topk)
    last = x[2 * chunk_len:]
    assert lens[2] == last.size == 5 < topk and np.isnan(last).sum() == 2, "a slice that must emit its NaN anchors"
    assert np.isfinite(x[c["idx"][0, 0][3:]]).all() and np.isposinf(x[c["idx"][0, 0][:3]]).all(), "+inf first, no NaN in the result"


@pytest.mark.parametrize("case", C.DECODE_CASES, ids=C.case_id)
def test_decode_cases_are_separated(case):
    R.assert_separated(C.decode_case(*case)["logits"])


@pytest.mark.parametrize("row", C.STAGE_CASES, ids=C.case_id)
def test_stage_cases_are_well_posed(row):
    c = C.stage_case(row)
    ref = c["ref"]
    R.assert_separated(c["logits"], c["thresh"])
    assert len(set(c["thresh"])) == 3
    assert R.batched_margin(ref["bev"], ref["all_scores"], ref["groups"], c["iou"]) > C.STAGE_MARGIN
    N = 3 * row[3]
    assert 0 < len(ref["cand"]) < ref["n_nms"] < N, "the NMS and the cut both drop and both keep"
    assert set(ref["cls"]) == {0, 1, 2}


@pytest.mark.parametrize("case", C.TAIL_CASES, ids=C.case_id)
def test_tail_cases_are_well_posed(case):
    B, n_cls, topk, iou, mode = case
    c = C.tail_case(*case)
    ref, N = c["ref"], B * n_cls * topk
    R.assert_separated(c["conf"], c["thresh"])
    assert R.batched_margin(ref["bev"], ref["all_scores"], ref["groups"], iou) > C.MARGIN
    assert N / 4 <= ref["n_nms"] <= 3 * N / 4, "between a quarter and three quarters survive the NMS"
    np.testing.assert_array_equal(ref["bev"], c["proposals"][:, [0, 1, 3, 4, 6]])  # zero deltas: refined == proposals
    lo, hi = c["block"]
    assert hi - lo >= 3 and (c["proposals"][lo:hi, [0, 1, 3, 4, 5, 6]] == c["proposals"][lo, [0, 1, 3, 4, 5, 6]]).all()
    assert np.isin(np.arange(lo, hi), ref["kept"]).sum() <= 1, "a block of identical boxes keeps one at most"
    if B * n_cls > 1:
        a, b = c["pair"]
        assert b - a == topk and (c["proposals"][a, [0, 1, 3, 4, 5, 6]] == c["proposals"][b, [0, 1, 3, 4, 5, 6]]).all()
        assert a in ref["kept"] and b in ref["kept"], "identical boxes in different groups both survive"
    s = ref["all_scores"]
    assert np.unique(s).size <= len(C.TAIL_CONF_VALUES) < N / 4, "many equal scores: the order is by candidate index"
    kept_s = s[ref["kept"]]
    assert (np.diff(kept_s) <= 0).all() and (np.diff(ref["kept"])[np.diff(kept_s) == 0] > 0).all()
    if mode == "mix":
        at = (kept_s == np.float32(0.5)) & (ref["groups"][ref["kept"]] % n_cls == 0)
        assert c["thresh"][0] == 0.5 and at.any(), "NMS survivors of class 0 sit exactly on its threshold: the strict cut drops them"
        assert 0 < len(ref["cand"]) < ref["n_nms"] and not (ref["scores"][ref["cls"] == 0] == 0.5).any()
    elif mode == "none":
        assert (s == 1.0).any() and len(ref["cand"]) == 0, "not even a score of exactly 1.0 passes a threshold of 1.0"
    else:
        assert (s == 0.0).any() and len(ref["cand"]) == ref["n_nms"], "everything the NMS keeps passes a threshold of -1"


def test_the_mask_home_switches_between_341_and_342():
    """prop_nms_reduce_finalize_kernel keeps the mask in LDS while N * ceil(N / 64) <= 2048"""
    words = lambda n: n * ((n + 63) // 64)
    assert words(341) <= 2048 < words(342)
    assert {63, 64, 65, 341, 342, 1024} <= {s[2] for s in C.TAIL_SHAPES if s[:2] == (1, 1)}

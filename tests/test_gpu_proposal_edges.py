"""GPU: csrc/proposal.hip against the float64 statement tests/proposal_ref.py, through the C ABI (no config decides a shape or a
topk), at the smallest shapes at which each branch of the file is taken.  The cases and why each is well-posed -- scores
separated, NMS decisions clear of the threshold -- live in tests/proposal_cases.py and are proved on the CPU by
tests/test_host_proposal_ref.py; the same conditions are asserted here again before a result is compared.

Which case covers what:
  level 1   prop_topk_chunk_kernel<4>: every selection row up to (1, 64, 64); <8>: (1, 181, 181) and (2, 288, 288); an empty
            trailing slice: (2, 7, 9), (1, 9, 29), (2, 5, 13); a slice shorter than K (sentinel rows): (1, 9, 29)
  select    rank sort: topk 1 ... 256; bitonic: topk 257, 300, 1024; the lowest-index-first branch over several register slices:
            the (2, 288, 288) tie cases
  merge     fused merge + decode launch: every B = n_cls = 1 case; separate merge and decode launches: the B = 2, n_cls = 3
            selection and decode cases (exact equality both)
  decode    rank sort: N <= 256; bitonic: (2, 40, 40) with topk 257, the stage cases with 768 / 771 candidates, the tail from 341 on
  NMS tail  mask in LDS: N <= 341; in global memory: N >= 342
Every case runs in fresh allocations, pre-filled with a pattern no result can equal."""
import numpy as np
import pytest
import torch

import proposal_cases as C
import proposal_ref as R
from gpu_util import dev

pytestmark = pytest.mark.gpu

FILL = -7.0  # no box coordinate, score, class or frame of any case
V3D_EUNSUPPORTED = -3  # include/vision3d_hip.h
SCORE_TOL = dict(rtol=1e-5, atol=1e-7)  # the bar of test_gpu_proposal.py against the CPU oracle
BOX_TOL = dict(rtol=1e-5, atol=1e-6)  # ... and against the torch statement


def _lib():
    from vision3d_amd import _lib as L
    return L, L.lib()


def run_topk(maps, anchors, geom):
    """v3d_proposals_topk -> (return code, boxes (B, n_cls, topk, 7), scores (B, n_cls, topk))"""
    L, lib = _lib()
    B, n_cls, n_yaw, H, W, topk = geom
    m, a = dev(maps), dev(anchors)
    boxes = torch.full((B, n_cls, topk, 7), FILL, dtype=torch.float32, device="cuda")
    scores = torch.full((B, n_cls, topk), FILL, dtype=torch.float32, device="cuda")
    ws = L.workspace(lib.v3d_proposals_workspace(B, n_cls, topk), m.device)
    rc = lib.v3d_proposals_topk(L.ptr(m), L.ptr(a), B, n_cls, n_yaw, H, W, topk, L.ptr(boxes), L.ptr(scores), L.ptr(ws), ws.numel(),
                                L.stream_ptr())
    torch.cuda.synchronize()
    return rc, boxes.cpu().numpy(), scores.cpu().numpy()


def _outputs(N):
    return (torch.full((N, 7), FILL, dtype=torch.float32, device="cuda"), torch.full((N,), int(FILL), dtype=torch.int64, device="cuda"),
            torch.full((N,), int(FILL), dtype=torch.int64, device="cuda"), torch.full((N,), FILL, dtype=torch.float32, device="cuda"),
            torch.full((1,), int(FILL), dtype=torch.int32, device="cuda"))


def _trim(boxes, bi, ci, scores, n_out):
    """-> dict of the first n_out rows; the rows behind them still hold the fill pattern"""
    torch.cuda.synchronize()
    n = int(n_out.item())
    assert 0 <= n <= boxes.shape[0]
    assert bool((boxes[n:] == FILL).all()) and bool((scores[n:] == FILL).all()) and bool((bi[n:] == int(FILL)).all()) \
        and bool((ci[n:] == int(FILL)).all()), "rows behind n_out are not written"
    return dict(n=n, boxes=boxes[:n].cpu().numpy(), batch=bi[:n].cpu().numpy(), cls=ci[:n].cpu().numpy(), scores=scores[:n].cpu().numpy())


def run_stage(maps, anchors, geom, thresh, iou):
    """v3d_proposals -> (return code, outputs as they were left)"""
    L, lib = _lib()
    B, n_cls, n_yaw, H, W, topk = geom
    m, a = dev(maps), dev(anchors)
    out = _outputs(B * n_cls * topk)
    ws = L.workspace(lib.v3d_proposals_workspace(B, n_cls, topk), m.device)
    rc = lib.v3d_proposals(L.ptr(m), L.ptr(a), B, n_cls, n_yaw, H, W, topk, L.host_f32(thresh), float(iou), *(L.ptr(t) for t in out),
                           L.ptr(ws), ws.numel(), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def run_refine(c):
    """v3d_refine_nms on a tail case -> (refined (N, 7), trimmed outputs)"""
    L, lib = _lib()
    B, n_cls, topk = c["geom"]
    N = B * n_cls * topk
    d, p, conf = dev(c["deltas"]), dev(c["proposals"]), dev(c["conf"])
    refined = torch.full((N, 7), FILL, dtype=torch.float32, device="cuda")
    out = _outputs(N)
    ws = L.workspace(lib.v3d_refine_nms_workspace(B, n_cls, topk), d.device)
    L.check(lib.v3d_refine_nms(L.ptr(d), L.ptr(p), L.ptr(conf), B, n_cls, topk, L.host_f32(c["thresh"]), float(c["iou"]), L.ptr(refined),
                               *(L.ptr(t) for t in out), L.ptr(ws), ws.numel(), L.stream_ptr()), "refine_nms")
    got = _trim(*out)
    return refined.cpu().numpy(), got


def check_selection(c, runs=2):
    """The full candidate list equals the reference's: the decoded box of an index-anchor case IS the selected anchor, bit for bit."""
    B, n_cls, n_yaw, H, W, topk = c["geom"]
    rc, boxes, scores = run_topk(c["maps"], c["anchors"], c["geom"])
    assert rc == 0
    np.testing.assert_array_equal(boxes[..., 0].astype(np.int64), c["idx"], err_msg="selected anchors, in order")
    want = np.take_along_axis(np.broadcast_to(c["anchors"].reshape(1, n_cls, -1, 7), (B, n_cls, n_yaw * H * W, 7)), c["idx"][..., None], 2)
    np.testing.assert_array_equal(boxes, want)
    np.testing.assert_allclose(scores, c["scores"], **SCORE_TOL)
    for _ in range(runs - 1):
        rc2, boxes2, scores2 = run_topk(c["maps"], c["anchors"], c["geom"])
        assert rc2 == 0 and np.array_equal(boxes, boxes2) and np.array_equal(scores.view(np.uint32), scores2.view(np.uint32)), \
            "two runs are bit-equal"
    return scores


@pytest.mark.parametrize("case", C.SELECT_CASES, ids=C.case_id)
def test_selection(case):
    """Lattice logits (heavy natural ties) and lattice plus the saturating / signed-zero values, on index anchors.  B = n_cls = 1:
    the fused merge + decode launch; B = 2, n_cls = 3: the separate launches."""
    c = C.select_case(*case)
    R.assert_separated(c["logits"])
    check_selection(c)


@pytest.mark.parametrize("case", C.TIE_CASES, ids=C.case_id)
def test_hand_built_ties(case):
    """A tie class straddling row K under strictly better candidates, the whole map equal, every score 0.0, a +0.0 / -0.0
    checkerboard: the lowest anchor indices of the tie class, in index order."""
    c = C.tie_case(*case)
    R.assert_separated(c["logits"])
    scores = check_selection(c)
    if case[1] == "all_zero":
        assert (scores == 0.0).all()
    if case[1] == "signed_zero":
        assert (scores == 0.5).all()


def test_nonfinite_logits():
    """A NaN logit of either sign counts as -inf (the header of proposal.hip); +inf scores 1.0, -inf 0.0.  One run."""
    c = C.nonfinite_case()
    R.assert_separated(R.nan_as_neg_inf(c["logits"]))
    scores = check_selection(c, runs=1)
    assert (scores[0, 0, :3] == 1.0).all() and np.isfinite(scores).all()


@pytest.mark.parametrize("case", C.DECODE_CASES, ids=C.case_id)
def test_decode(case):
    """Random anchors in KITTI ranges, regression channels N(0, 0.3): the decoded candidates against the float64 decode of the
    reference's selection."""
    c = C.decode_case(*case)
    R.assert_separated(c["logits"])
    rc, boxes, scores = run_topk(c["maps"], c["anchors"], c["geom"])
    assert rc == 0
    np.testing.assert_allclose(scores, c["scores"], **SCORE_TOL)
    np.testing.assert_allclose(boxes, c["boxes"], **BOX_TOL)
    rc2, boxes2, scores2 = run_topk(c["maps"], c["anchors"], c["geom"])
    assert rc2 == 0 and np.array_equal(boxes, boxes2) and np.array_equal(scores, scores2), "two runs are bit-equal"


def _assert_tail_equal(got, ref, exact_boxes):
    assert got["n"] == len(ref["cand"])
    np.testing.assert_array_equal(got["batch"], ref["batch"])
    np.testing.assert_array_equal(got["cls"], ref["cls"])
    np.testing.assert_allclose(got["scores"], ref["scores"], **SCORE_TOL)
    if exact_boxes:
        np.testing.assert_array_equal(got["boxes"], ref["boxes"].astype(np.float32))
    else:
        np.testing.assert_allclose(got["boxes"], ref["boxes"], **BOX_TOL)


@pytest.mark.parametrize("case", C.TAIL_CASES, ids=C.case_id)
def test_tail(case):
    """v3d_refine_nms with zero deltas: sort, NMS in every mask home, group offsets and the strict score cut on boxes of our
    choosing.  z of a box is its candidate index, so the output names the surviving candidates."""
    c = C.tail_case(*case)
    ref = c["ref"]
    R.assert_separated(c["conf"], c["thresh"])
    assert R.batched_margin(ref["bev"], ref["all_scores"], ref["groups"], c["iou"]) > C.MARGIN
    refined, got = run_refine(c)
    np.testing.assert_array_equal(refined, c["proposals"])  # zero deltas: bit for bit
    assert got["n"] == len(ref["cand"])
    np.testing.assert_array_equal(got["boxes"][:, 2].astype(np.int64), ref["cand"], err_msg="surviving candidates, in order")
    _assert_tail_equal(got, ref, exact_boxes=True)
    if case[4] == "none":
        assert got["n"] == 0
    refined2, got2 = run_refine(c)
    assert np.array_equal(refined, refined2) and all(np.array_equal(got[k], got2[k]) for k in got), "two runs are bit-equal"


@pytest.mark.parametrize("row", C.STAGE_CASES, ids=C.case_id)
def test_whole_stage(row):
    """v3d_proposals, three classes with distinct thresholds, random anchors and deltas, against `proposal_ref.stage`."""
    c = C.stage_case(row)
    ref = c["ref"]
    R.assert_separated(c["logits"], c["thresh"])
    assert R.batched_margin(ref["bev"], ref["all_scores"], ref["groups"], c["iou"]) > C.STAGE_MARGIN
    rc, out = run_stage(c["maps"], c["anchors"], c["geom"], c["thresh"], c["iou"])
    assert rc == 0
    _assert_tail_equal(_trim(*out), ref, exact_boxes=False)


def _edge_maps(W):
    n_yaw, H, _ = C.EDGE_SHAPE
    n = n_yaw * H * W
    logits = R.lattice_logits(np.random.default_rng(W), (1, 1, n))
    return logits, R.maps_from_logits(logits, 1, 1, n_yaw, H, W), R.index_anchors(1, n_yaw, H, W), (1, 1, n_yaw, H, W, C.EDGE_TOPK)


def test_acceptance_edge_accepts_327680_anchors():
    """40 slices of exactly 8192 anchors: the most a call accepts; ProposalLayer.native_supported says the same."""
    from vision3d_amd.core.config import second_car_cfg
    from vision3d_amd.detector.proposal import ProposalLayer
    logits, maps, anchors, geom = _edge_maps(C.EDGE_SHAPE[2])
    assert logits.shape[-1] == 327680 and ProposalLayer(second_car_cfg()).native_supported(1, logits.shape[-1])
    idx, sc = R.select_topk(logits, C.EDGE_TOPK)
    rc, boxes, scores = run_topk(maps, anchors, geom)
    assert rc == 0
    np.testing.assert_array_equal(boxes[..., 0].astype(np.int64), idx)
    np.testing.assert_allclose(scores, sc, **SCORE_TOL)


def test_acceptance_edge_refuses_one_more_column():
    """One more W column: the slice length passes 8192 -> V3D_EUNSUPPORTED from both entries, no output touched."""
    from vision3d_amd.core.config import second_car_cfg
    from vision3d_amd.detector.proposal import ProposalLayer
    logits, maps, anchors, geom = _edge_maps(C.EDGE_SHAPE[2] + 1)
    assert not ProposalLayer(second_car_cfg()).native_supported(1, logits.shape[-1])
    rc, boxes, scores = run_topk(maps, anchors, geom)
    assert rc == V3D_EUNSUPPORTED and (boxes == FILL).all() and (scores == FILL).all()
    rc, out = run_stage(maps, anchors, geom, [0.3], 0.01)
    assert rc == V3D_EUNSUPPORTED
    for t in out:
        assert bool((t == (FILL if t.is_floating_point() else int(FILL))).all())

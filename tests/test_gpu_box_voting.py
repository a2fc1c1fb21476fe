"""GPU: IoU-weighted box voting (cfg.BOX_VOTING) -- the native op (csrc/box_voting.hip v3d_box_voting), the two fused tails that vote
(csrc/proposal.hip v3d_proposals_vote_flag / v3d_refine_nms_vote) and one captured graph -- against the float64 torch statement
(ops.box_voting_statement), which takes its IoU matrix from ops.box_iou_rotated like the kernel: both make the same membership
decisions, no case needs a margin around the threshold.  tests/test_host_box_voting.py holds the statement against the numpy
restatement on the CPU.

Yardstick (the own_factor rule of tests/gpu_util.py / tests/test_gpu_iou_head.py): the fp32 torch statement run on the same device and
case.  The kernel's error against float64, relative to max(1, |coordinate|), may be at most OWN_FACTOR = 2 times that statement's own,
plus one unit in the last place of the coordinate (2^-23 max(1, |value|); the statement can be exact where the kernel rounds once).
Every figure is printed before it is asserted; tools/mb_box_voting.py writes the largest over the cases into profiles/box_voting.txt.
Exact-bit expectations are asserted as bits."""
import numpy as np
import pytest
import torch

import box_voting_cases as VC
import box_voting_ref as VR
from gpu_util import dev

pytestmark = pytest.mark.gpu

OWN_FACTOR, ULP = 2.0, 2.0 ** -23
STATEMENT_TOL = 1e-5  # native tail against the op-by-op tail: their decodes differ by an ulp of expf (the bar of tests/test_gpu_iou_head.py)


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _np64(t):
    return t.detach().double().cpu().numpy()


def figures(boxes, scores, iou, got):
    """-> (the fp32 torch statement's error against the float64 statement, the error of `got`), relative to max(1, |coordinate|)"""
    from vision3d_amd.ops import box_voting_statement
    from vision3d_amd.ops.box_voting import group_iou
    u = group_iou(boxes)
    ref = _np64(box_voting_statement(boxes, scores, iou, torch.float64, iou=u))
    own = VR.scaled_error(_np64(box_voting_statement(boxes, scores, iou, torch.float32, iou=u)), ref)
    return own, VR.scaled_error(_np64(got), ref), ref


# --------------------------------------------------------------------------------------------------------------------------- op
@pytest.mark.parametrize("name", VC.OP_CASES)
def test_op_against_the_float64_statement(name):
    from vision3d_amd.ops import box_voting_rotated
    c = VC.op_case(name)
    boxes, scores = dev(c["boxes"]), dev(c["scores"])
    got = box_voting_rotated(boxes, scores, c["iou"])
    own, err, ref = figures(boxes, scores, c["iou"], got)
    bar = OWN_FACTOR * own + ULP
    print(f"box-voting-op {name}: kernel {err:.3e}, fp32 statement {own:.3e}, bar {bar:.3e}")
    assert got.shape == boxes.shape and got.dtype == torch.float32
    assert err <= bar
    moved = (_bits(got) != _bits(boxes)).any(-1)
    if name.startswith(("t", "g")) or name in ("far_field", "isolation", "hand", "yaw_far"):
        assert moved.any(), "centres with voters beside themselves move"
    # inert threshold: nobody votes, the input's bits
    np.testing.assert_array_equal(_bits(box_voting_rotated(boxes, scores, 2.0)), _bits(boxes))


def test_op_hand_cases_and_exact_bits():
    from vision3d_amd.ops import box_iou_rotated, box_voting_rotated
    run = lambda name, iou=None: (lambda c: box_voting_rotated(dev(c["boxes"]), dev(c["scores"]), c["iou"] if iou is None else iou))(VC.op_case(name))
    hand = run("hand")
    x = float(hand[0, 0, 0])
    print(f"box-voting-op hand: x = {x!r}, literal {VC.HAND_X!r}")
    assert abs(x - VC.HAND_X) <= OWN_FACTOR * ULP and abs(float(hand[0, 0, 2]) - VC.HAND_Z) <= OWN_FACTOR * ULP
    # single candidate: the input's bits
    np.testing.assert_array_equal(_bits(run("single")), VC.op_case("single")["boxes"].view(np.uint32))
    # non-members (s = 0, the -1 sentinel, a NaN and an inf component, all overlapping the centre): the centre and its voter have the
    # bits of the case without them
    np.testing.assert_array_equal(_bits(run("non_members"))[0, :2], _bits(hand)[0])
    # centres with a NaN x, a NaN yaw, zero area, an inf y come back unchanged; their ordinary neighbours vote for one another
    c = VC.op_case("unchanged_centres")
    got = _bits(run("unchanged_centres"))
    np.testing.assert_array_equal(got[0, :4], c["boxes"].view(np.uint32)[0, :4])
    assert (got[0, 4:] != c["boxes"].view(np.uint32)[0, 4:]).any()
    # yaw: a neighbour at yaw_k + pi - 0.1 pulls by -0.1; +-pi / 2 exactly keeps its sign (round half to even)
    c = VC.op_case("yaw_half_turn")
    b = dev(c["boxes"])[0][:, [0, 1, 3, 4, 6]].contiguous()
    w = 0.4 * float(box_iou_rotated(b[:1], b[1:])[0, 0])
    assert abs(float(run("yaw_half_turn")[0, 0, 6]) - (0.3 - 0.1 * w / (0.8 + w))) <= 1e-6
    for name, sign in (("yaw_plus_half_pi", 1.0), ("yaw_minus_half_pi", -1.0)):
        c = VC.op_case(name)
        b = dev(c["boxes"])[0][:, [0, 1, 3, 4, 6]].contiguous()
        w = 0.4 * float(box_iou_rotated(b[:1], b[1:])[0, 0])
        assert w > 0 and abs(float(run(name)[0, 0, 6]) - sign * float(VC.HALF_PI32) * w / (0.8 + w)) <= 1e-6
    # group isolation: identical boxes, different scores -- a group's rows are those of the group alone, bit for bit
    c = VC.op_case("isolation")
    whole = _bits(run("isolation"))
    for g in range(4):
        alone = box_voting_rotated(dev(c["boxes"][g:g + 1]), dev(c["scores"][g:g + 1]), c["iou"])
        np.testing.assert_array_equal(_bits(alone)[0], whole[g])
    assert (whole[0] != whole[1]).any()


def test_op_threshold_edge_is_inclusive():
    """the rule is >=: at the fp32 value ops.box_iou_rotated returns for the pair the neighbour votes, one ulp above it does not"""
    from vision3d_amd.ops import box_iou_rotated, box_voting_rotated
    c = VC.op_case("hand")
    boxes, scores = dev(c["boxes"]), dev(c["scores"])
    bev = boxes[0][:, [0, 1, 3, 4, 6]].contiguous()
    at = float(box_iou_rotated(bev[:1], bev[1:])[0, 0])
    above = float(np.nextafter(np.float32(at), np.float32(np.inf)))
    voted, not_voted = box_voting_rotated(boxes, scores, at), box_voting_rotated(boxes, scores, above)
    print(f"box-voting-op threshold edge: IoU {at!r}, next {above!r}, x {float(voted[0, 0, 0])!r} / {float(not_voted[0, 0, 0])!r}")
    assert abs(float(voted[0, 0, 0]) - VC.HAND_X) <= 1e-6
    np.testing.assert_array_equal(_bits(not_voted), _bits(boxes))


# ---------------------------------------------------------------------------------------------------------------------- stage 1
def _heads(with_dir, with_iou):
    from vision3d_amd.detector.proposal import ProposalLayer
    return tuple(ProposalLayer(VC.make_cfg(with_dir, with_iou, vote=v)).cuda().eval() for v in (False, True))


def _candidate_rows(cand_boxes, unvoted):
    """row of every un-voted output box among the candidates, by its bits (the tails copy candidates: a survivor IS a candidate row)"""
    eq = (_bits(unvoted)[:, None, :] == _bits(cand_boxes)[None, :, :]).all(-1)
    assert (eq.sum(1) >= 1).all()
    return torch.from_numpy(eq.argmax(1)).to(cand_boxes.device)


def _sorted_rows(r):
    a = np.concatenate((r[0].double().cpu().numpy(), r[3].double().cpu().numpy()[:, None], r[1].cpu().numpy()[:, None], r[2].cpu().numpy()[:, None]), 1)
    return a[np.lexsort((a[:, 1], a[:, 0], -a[:, 7]))]


@pytest.mark.parametrize("with_dir,with_iou", VC.STAGE_VARIANTS)
def test_stage1_votes_and_changes_nothing_else(with_dir, with_iou):
    c = VC.stage_case(with_dir, with_iou)
    B, n_cls, n_yaw, H, W, topk = c["geom"]
    off, on = _heads(with_dir, with_iou)
    maps, anchors = dev(c["maps"]), dev(c["anchors"])
    plain = off.finalize_native(*off.native_proposals(maps, anchors))
    voted = on.finalize_native(*on.native_proposals(maps, anchors))
    # count, indices and scores: the bits of the same call with voting off
    assert len(voted[0]) == len(plain[0]) > 0
    for k in (1, 2, 3):
        np.testing.assert_array_equal(_bits(voted[k]) if k == 3 else voted[k].cpu().numpy(), _bits(plain[k]) if k == 3 else plain[k].cpu().numpy())
    moved = (_bits(voted[0]) != _bits(plain[0])).any(-1)
    assert moved.any(), "no survivor had a voter beside itself: the case checks nothing"
    # the boxes: the vote of the stage's own candidates (v3d_proposals_topk decodes with the same kernel body), by the op's bar
    cand_boxes, cand_scores = off.native_topk(maps, anchors)
    cb, cs = cand_boxes.reshape(B * n_cls, topk, 7), cand_scores.reshape(B * n_cls, topk)
    rows = _candidate_rows(cand_boxes.reshape(-1, 7), plain[0])
    from vision3d_amd.ops import box_voting_rotated
    rows = rows.cpu().numpy()
    np.testing.assert_array_equal(_bits(cs.reshape(-1))[rows], _bits(plain[3]))  # (and rates them with the same scores)
    own, err_op, ref = figures(cb, cs, VC.STAGE_VOTE_IOU, box_voting_rotated(cb, cs, VC.STAGE_VOTE_IOU))
    err = VR.scaled_error(_np64(voted[0]), ref.reshape(-1, 7)[rows])
    assert err_op <= OWN_FACTOR * own + ULP
    bar = OWN_FACTOR * own + ULP
    print(f"box-voting-stage1 dir={with_dir} iou={with_iou}: {len(voted[0])} survivors, {int(moved.sum())} moved; tail {err:.3e}, "
          f"fp32 statement {own:.3e}, bar {bar:.3e}")
    assert err <= bar
    # native_proposals equals the op-by-op tails: inference_from_maps, and proposals_padded + finalize
    cls_map, reg_map = on.maps_from_fused(maps)
    extra = on.extra_from_fused(maps)
    stated = on.inference_from_maps(cls_map.clone(), reg_map, anchors, *extra)
    padded = on.finalize(*on.proposals_padded(cls_map, reg_map, anchors, *extra))
    stated_off = off.inference_from_maps(cls_map.clone(), reg_map, anchors, *extra)
    for other in (stated, padded):
        assert len(other[0]) == len(voted[0])
        np.testing.assert_allclose(_sorted_rows(other), _sorted_rows(voted), rtol=STATEMENT_TOL, atol=STATEMENT_TOL)
        assert torch.equal(other[3], stated_off[3]) and torch.equal(other[1], stated_off[1]) and torch.equal(other[2], stated_off[2])
    assert not torch.equal(stated[0], stated_off[0])


# ---------------------------------------------------------------------------------------------------------------------- stage 2
def test_stage2_votes_and_refined_stays():
    c = VC.refine_case()
    B, n_cls, topk = c["geom"]
    off, on = _heads(False, False)
    d, p, conf = dev(c["deltas"]), dev(c["proposals"]), dev(c["conf"])
    refined_off, plain = off.native_refine_nms(d, p, conf)
    refined_on, voted = on.native_refine_nms(d, p, conf)
    np.testing.assert_array_equal(_bits(refined_on), _bits(refined_off))  # `refined` is the un-voted decode either way
    assert len(voted[0]) == len(plain[0]) > 0
    assert torch.equal(voted[1], plain[1]) and torch.equal(voted[2], plain[2])
    np.testing.assert_array_equal(_bits(voted[3]), _bits(plain[3]))
    moved = (_bits(voted[0]) != _bits(plain[0])).any(-1)
    assert moved.any(), "no survivor had a voter beside itself: the case checks nothing"
    # the tail votes the refined candidates with sigmoid(conf): the op on the same bits gives the same bits (same kernel, same order)
    from vision3d_amd.ops import box_voting_rotated
    cb, cs = refined_off.reshape(B * n_cls, topk, 7), torch.sigmoid(conf).reshape(B * n_cls, topk)
    rows = _candidate_rows(cb.reshape(-1, 7), plain[0]).cpu().numpy()
    # (the weights: the tail's own scores where it returns them -- the survivors --, torch's sigmoid of the same logit elsewhere)
    print(f"box-voting-stage2: scores of the tail with other bits than torch.sigmoid: {int((_bits(plain[3]) != _bits(cs.reshape(-1))[rows]).sum())}")
    cs = cs.clone()
    cs.view(-1)[torch.from_numpy(rows).to(cs.device)] = plain[3]
    own, err, ref = figures(cb, cs, VC.STAGE_VOTE_IOU, box_voting_rotated(cb, cs, VC.STAGE_VOTE_IOU))
    err_tail = VR.scaled_error(_np64(voted[0]), ref.reshape(-1, 7)[rows])
    bar = OWN_FACTOR * own + ULP
    print(f"box-voting-stage2: {len(voted[0])} survivors, {int(moved.sum())} moved; tail {err_tail:.3e}, op {err:.3e}, fp32 statement {own:.3e}, "
          f"bar {bar:.3e}")
    assert err <= bar and err_tail <= bar
    # the torch fallback of PV_RCNN.inference: batched NMS on the refined boxes, the statement's vote, the score cut
    from vision3d_amd.ops import batched_nms_rotated
    boxes, scores = refined_off.reshape(-1, 7), cs.reshape(-1)
    group = torch.arange(B * n_cls, device=boxes.device).repeat_interleave(topk)
    keep = batched_nms_rotated(boxes[:, [0, 1, 3, 4, 6]].contiguous(), scores, group, 0.01)
    stated = on._voted(boxes, scores, B * n_cls)[keep]
    mask = on._above_score_thresh(scores[keep], (group % n_cls)[keep])
    assert int(mask.sum()) == len(voted[0])
    np.testing.assert_allclose(stated[mask].cpu().numpy(), voted[0].cpu().numpy(), rtol=STATEMENT_TOL, atol=STATEMENT_TOL)


# ------------------------------------------------------------------------------------------------------------------------- graph
MODEL_BOUNDS = [0, -8.0, -3, 12.8, 8.0, 1]  # a 40 x 32 map, 20 000 points: the smallest cloud of the graph tests (test_gpu_iou_head.py)


def test_captured_graph_votes_like_eager():
    import direction_cases as DC
    from gpu_util import randomize_bn
    from vision3d_amd import synth
    from vision3d_amd.core import AnchorGenerator
    from vision3d_amd.detector import Second
    results = {}
    for vote in (False, True):
        cfg = DC.make_cfg(1, enabled=False, bounds=MODEL_BOUNDS, thresh=(0.05,))
        cfg.BOX_VOTING.ENABLED = vote
        torch.manual_seed(0)
        model = Second(cfg).cuda()
        randomize_bn(model, 0)
        model.eval()
        anchors = AnchorGenerator(cfg).anchors.cuda()
        clouds = [torch.from_numpy(synth.make_cloud(3, n_points=20000)).cuda()]
        with torch.no_grad():
            eager = [t.clone() for t in model.inference_points(clouds, anchors)]
            if vote:
                graphed = model.graphed_inference(anchors, [len(c) for c in clouds])
                replays = [[t.clone() for t in graphed(clouds)] for _ in range(2)]
        results[vote] = eager
    assert len(results[True][0]) == len(results[False][0]) > 0
    for k in (1, 2, 3):
        assert torch.equal(results[True][k], results[False][k])
    print(f"box-voting-graph: {len(eager[0])} detections, {int((results[True][0] != results[False][0]).any(-1).sum())} moved by the vote")
    for replay in replays:
        for a, b in zip(replay, results[True]):
            np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())

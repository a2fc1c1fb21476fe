"""GPU: the IoU-aware confidence head of the anchor head (cfg.IOU_HEAD) -- loss and gradient (csrc/proposal_loss.hip
v3d_proposal_iou_loss_fwd_bwd / _scale), the rectified score of the proposal stage (csrc/proposal.hip v3d_proposals_iou_topk / _flag)
and the model -- against the float64 statements of tests/iou_head_ref.py and the torch statements.  tests/test_host_iou_head.py proves
every ordered case here decided by margin on the reference alone.

Yardstick of the fp32 comparisons (the own_factor rule of tests/gpu_util.py): the fp32 torch statement run on the same device and
case.  A kernel's error against float64 may be at most OWN_FACTOR = 2 times that statement's own error against float64, plus
IOU_ERROR = 2.0e-7, what the rotated IoU of a pair itself measures in fp32 (profiles/iou_loss.txt).  Loss terms: relative to
max(1, |term|); gradients: relative to the largest gradient of the map under upstream gradients (2, 3, 5, 7); the target: absolute (it
lies in [0, 1]).  The rectified score is a number in [0, 1] too and has no IoU in it: twice the statement's own error plus one unit in
the last place of the score format at 1 (2^-23 = 1.2e-7; the statement can be exact where the kernel rounds once).  Every figure is
printed before it is asserted; tools/mb_iou_head.py writes the largest of each over the cases into profiles/iou_head.txt.
"""
import math

import numpy as np
import pytest
import torch

import direction_ref as D
import iou_head_cases as IC
import iou_head_ref as IH
import proposal_cases as C
from gpu_util import dev

pytestmark = pytest.mark.gpu

OWN_FACTOR, IOU_ERROR, SCORE_ULP = 2.0, 2.0e-7, 2.0 ** -23
UPSTREAM = (2.0, 3.0, 5.0, 7.0)
YAW_TOL = 1e-5  # tests/test_gpu_direction.py


# -------------------------------------------------------------------------------------------------------------------------- loss
def _u8(a):
    return dev(np.ascontiguousarray(a).astype(np.uint8))


def native_loss(c, upstream=UPSTREAM):
    """v3d_proposal_iou_loss_fwd_bwd + _scale through FusedProposalIoULossFunction -> (losses (4 scalars), target, maps.grad)"""
    from vision3d_amd.detector.proposal import FusedProposalIoULossFunction
    maps = dev(c["maps"]).requires_grad_(True)
    g_dir = dev(c["G_dir"]) if c["with_dir"] else None
    *losses, target = FusedProposalIoULossFunction.apply(maps, dev(c["anchors"]), dev(c["G_cls"]), _u8(c["M_cls"]), dev(c["G_reg"]),
                                                         _u8(c["M_reg"]), g_dir, c["sin_yaw"], c["n_cls"], c["n_yaw"], 0.25, 2.0, True)
    sum(u * l for u, l in zip(upstream, losses)).backward()
    return [l.detach() for l in losses], target, maps.grad


def existing_loss(c):
    """The entry points from before the head, on the class / box (/ direction) channels: (losses, dmaps) with upstream gradients 1"""
    from vision3d_amd.detector.proposal import FusedProposalDirLossFunction, FusedProposalLossFunction
    na = c["n_cls"] * c["n_yaw"]
    maps = dev(c["maps"])[:, :na * (8 + c["with_dir"])].contiguous().requires_grad_(True)
    args = (maps, dev(c["G_cls"]), _u8(c["M_cls"]), dev(c["G_reg"]), _u8(c["M_reg"]))
    if c["with_dir"]:
        losses = FusedProposalDirLossFunction.apply(*args, dev(c["G_dir"]), c["sin_yaw"], c["n_cls"], c["n_yaw"], 0.25, 2.0)
    else:
        losses = FusedProposalLossFunction.apply(*args, c["n_cls"], c["n_yaw"], 0.25, 2.0)
    sum(losses).backward()
    return [l.detach() for l in losses], maps.grad


def statement(c, dtype):
    maps, out, target = IC.torch_statement(c, dtype, "cuda", native_iou=False)
    keys = ["cls_loss", "reg_loss"] + (["dir_loss"] if c["with_dir"] else []) + ["iou_loss"]
    up = dict(zip(("cls_loss", "reg_loss", "dir_loss", "iou_loss"), UPSTREAM))
    sum(up[k] * out[k] for k in keys).backward()
    losses = {k: float(out[k].detach()) for k in keys}
    losses.setdefault("dir_loss", 0.0)
    return losses, target.double().cpu().numpy(), maps.grad.double().cpu().numpy()


def loss_figures(case):
    """-> {name: (the fp32 torch statement's error against float64, the kernel's)} and the kernel's raw outputs"""
    c = IC.loss_case(*case)
    ref = IC.loss_reference(case)
    gref = sum(u * g for u, g in zip(UPSTREAM, ref["grads"]))
    gmax = max(float(np.abs(gref).max()), 1e-30)
    own_l, own_t, own_g = statement(c, torch.float32)
    losses, target, grad = native_loss(c)
    got_l = dict(zip(("cls_loss", "reg_loss", "dir_loss", "iou_loss"), (float(l) for l in losses)))
    got_t, got_g = target.double().cpu().numpy(), grad.double().cpu().numpy()
    na = c["n_cls"] * c["n_yaw"]
    groups = dict(cls=slice(0, na), box=slice(na, 8 * na), iou=slice((8 + c["with_dir"]) * na, None))
    if c["with_dir"]:
        groups["dir"] = slice(8 * na, 9 * na)
    fig = {"iou_target": (float(np.abs(own_t - ref["target"]).max()), float(np.abs(got_t - ref["target"]).max()))}
    for k in ("cls_loss", "reg_loss", "dir_loss", "iou_loss"):
        fig[k] = tuple(abs(x[k] - ref[k]) / max(1.0, abs(ref[k])) for x in (own_l, got_l))
    for k, sl in groups.items():
        fig[k + "_gradient"] = tuple(float(np.abs(g[:, sl] - gref[:, sl]).max()) / gmax for g in (own_g, got_g))
    return fig, c, ref, (losses, target, grad)


@pytest.mark.parametrize("case", IC.LOSS_CASES, ids=C.case_id)
def test_loss_target_and_gradient_against_the_float64_statement(case):
    fig, c, ref, (losses, target, grad) = loss_figures(case)
    print("iou-head-loss-figures", dict(case=C.case_id(case), **{k: (f"{a:.2e}", f"{b:.2e}") for k, (a, b) in fig.items()}))
    pos = dev(c["M_reg"][..., 0])
    na = c["n_cls"] * c["n_yaw"]
    iou_group = grad[:, (8 + c["with_dir"]) * na:].reshape(target.shape)
    assert float(target[~pos].abs().max()) == 0.0 and float(iou_group[~pos].abs().max()) == 0.0, "exactly 0 off the positives"
    assert torch.isfinite(grad).all() and all(torch.isfinite(l) for l in losses)
    assert float(target.min()) >= 0.0 and float(target.max()) <= 1.0
    if not c["with_dir"]:
        assert float(losses[2]) == 0.0
    if c["variant"] == "no_positives":
        assert float(losses[1]) == 0.0 and float(losses[3]) == 0.0 and float(grad[:, na:].abs().max()) == 0.0
    if c["variant"] == "disjoint":
        assert float(target.max()) == 0.0
    if c["variant"] == "bad_row":
        assert int((target[pos] == 0).sum()) >= int(pos.sum()) // 2
    for k, (own, got) in fig.items():
        assert got <= OWN_FACTOR * own + IOU_ERROR, (k, own, got)


@pytest.mark.parametrize("case", IC.LOSS_CASES, ids=C.case_id)
def test_class_box_direction_terms_are_bit_equal_to_the_existing_entry_points(case):
    c = IC.loss_case(*case)
    losses, _, grad = native_loss(c, (1.0, 1.0, 1.0, 1.0))
    old_losses, old_grad = existing_loss(c)
    for a, b in zip(losses, old_losses):
        assert torch.equal(a, b)
    assert torch.equal(grad[:, :old_grad.shape[1]], old_grad)


@pytest.mark.parametrize("case", [(2, 5, 7, 3, "plain", True), (2, 20, 24, 3, "plain", False), (2, 20, 24, 1, "bad_row", True)], ids=C.case_id)
def test_two_runs_are_bit_equal(case):
    c = IC.loss_case(*case)
    (a, ta, ga), (b, tb, gb) = native_loss(c), native_loss(c)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(ta, tb) and torch.equal(ga, gb)


SCALE_CASES = [(2, 5, 7, 1, "plain", False), (2, 5, 7, 3, "plain", True), (2, 5, 7, 3, "plain", False), (2, 20, 24, 1, "plain", True)]


@pytest.mark.parametrize("case", SCALE_CASES, ids=C.case_id)
def test_upstream_gradients_scale_the_channel_groups_exactly(case):
    """Under upstream gradients (2, 3, 5, 7) the backward returns the (1, 1, 1, 1) gradient times 2 on the class channels, 3 on the box
    channels, 5 on the direction channels (where the head has them) and 7 on the IoU channels: one exact fp32 multiply per element."""
    c = IC.loss_case(*case)
    _, _, g1 = native_loss(c, (1.0, 1.0, 1.0, 1.0))
    _, _, g2 = native_loss(c, UPSTREAM)
    na = c["n_cls"] * c["n_yaw"]
    d = int(c["with_dir"])
    want = g1.clone()
    bounds = [(0, na, 2.0), (na, 8 * na, 3.0)] + ([(8 * na, 9 * na, 5.0)] if d else []) + [((8 + d) * na, (9 + d) * na, 7.0)]
    for lo, hi, f in bounds:
        assert float(want[:, lo:hi].abs().max()) > 0
        want[:, lo:hi] *= f
    assert torch.equal(g2, want)


def test_proposal_loss_takes_the_native_pass_and_equals_the_statement():
    from vision3d_amd.detector import ProposalLoss
    c = IC.loss_case(2, 20, 24, 3, "plain", True)
    cfg = IC.make_cfg(3, with_dir=True)
    maps = dev(c["maps"]).requires_grad_(True)
    item = IC.loss_item(c, maps)
    fused = dict(item, _head_maps=(maps, item["P_cls"], item["P_reg"], item["P_dir"], item["P_iou"]))
    out = ProposalLoss(cfg)(fused)
    assert type(out["iou_loss"].grad_fn).__name__ == "FusedProposalIoULossFunctionBackward", "the native pass ran"
    stated = ProposalLoss(cfg)(item)
    assert sorted(out) == sorted(stated) == ["cls_loss", "dir_loss", "iou_loss", "loss", "reg_loss"]
    for k in out:
        assert abs(float(out[k].detach()) - float(stated[k].detach())) <= 1e-5 * max(1.0, abs(float(stated[k].detach()))), k
    replaced = dict(fused, P_iou=item["P_iou"] * 1.0)  # an output that is no longer the view made from the fused maps: torch expressions
    assert type(ProposalLoss(cfg)(replaced)["iou_loss"].grad_fn).__name__ != "FusedProposalIoULossFunctionBackward"
    t = ProposalLoss(cfg).iou_targets(item)
    assert t.shape == item["P_cls"].shape and not t.requires_grad
    np.testing.assert_allclose(t.cpu().numpy(), IC.loss_reference((2, 20, 24, 3, "plain", True))["target"], rtol=0, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------------------ decode
def _layer(geom, with_dir, power, enabled=True, thresh=None):
    from vision3d_amd.detector.proposal import ProposalLayer
    B, n_cls, n_yaw, H, W, topk = geom
    return ProposalLayer(IC.make_cfg(n_cls, n_yaw, topk, enabled=enabled, power=power, with_dir=with_dir, thresh=thresh))


DECODE_PARAMS = [(case, d, p) for case in IC.DECODE_CASES for d in (False, True) for p in IC.POWERS]


@pytest.mark.parametrize("case,with_dir,power", DECODE_PARAMS, ids=[C.case_id((*c, d, p)) for c, d, p in DECODE_PARAMS])
def test_decode(case, with_dir, power):
    """native_topk: the selected anchors and their order are the reference's (the decoded boxes name the anchors: random anchors are
    distinct), s' under the yardstick rule, boxes as tests/test_gpu_direction.py holds them; POWER = 0 bit-equal to the entry without
    the IoU channel; a short map keeps its sentinels at score -1 behind the real rows."""
    from vision3d_amd.detector.proposal import rectified_scores
    c = IC.decode_case(*case, with_dir)
    ref = c["by_power"][power]
    B, n_cls, n_yaw, H, W, topk = c["geom"]
    real = c["real"]
    na = n_cls * n_yaw
    head = _layer(c["geom"], with_dir, power)
    maps, anchors = dev(c["maps"]), dev(c["anchors"])
    boxes, scores = head.native_topk(maps, anchors)
    boxes2, scores2 = head.native_topk(maps, anchors)
    torch.cuda.synchronize()
    assert torch.equal(boxes, boxes2) and torch.equal(scores, scores2), "two runs are bit-equal"
    got_b = boxes.cpu().numpy().reshape(B, n_cls, topk, 7)
    got_s = scores.cpu().numpy().reshape(B, n_cls, topk)
    assert (got_s[..., real:] == -1.0).all(), "sentinels keep score -1 and stand last"
    np.testing.assert_allclose(got_b[..., :real, :6], ref["boxes"][..., :6], rtol=1e-5, atol=1e-6)
    if with_dir:
        assert np.abs(got_b[..., :real, 6] - ref["boxes"][..., 6]).max() <= YAW_TOL
        assert (got_b[..., :real, 6] >= np.float32(D.OFFSET) - 1e-6).all() and (got_b[..., :real, 6] < D.OFFSET + 2 * math.pi + 1e-6).all()
    else:
        np.testing.assert_allclose(got_b[..., :real, 6], ref["boxes"][..., 6], rtol=1e-5, atol=1e-6)
    # the fp32 torch statement of the score rule on the reference's selection
    n = n_yaw * H * W
    idx = dev(ref["idx"])
    cls_logit = maps[:, :na].reshape(B, n_cls, n).gather(2, idx)
    z = maps[:, na * (8 + with_dir):].reshape(B, n_cls, n).gather(2, idx)
    stated = rectified_scores(torch.sigmoid(cls_logit), z, power).cpu().numpy().astype(np.float64)
    own, err = float(np.abs(stated - ref["scores"]).max()), float(np.abs(got_s[..., :real] - ref["scores"]).max())
    print("iou-head-score-figures", dict(case=C.case_id((*case, with_dir, power)), own=f"{own:.2e}", kernel=f"{err:.2e}"))
    assert err <= OWN_FACTOR * own + SCORE_ULP
    assert (np.diff(got_s[..., :real], axis=-1) <= 0).all()
    if power > 0 and c["hand"] is not None and real >= 7:
        tied = ref["scores"][0, 0, 1:] == ref["scores"][0, 0, :-1]
        assert (got_s[0, 0, 1:real][tied] == got_s[0, 0, :real - 1][tied]).all(), "equal in the reference: identical logits, equal bits"
        assert (got_s[0, 0, :real] == 0).sum() == (ref["scores"][0, 0] == 0).sum() >= 2, "a NaN and a -inf IoU logit give s' = 0"
    if power == 0 and real == topk:
        plain = _layer(c["geom"], with_dir, 0, enabled=False)
        boxes0, scores0 = plain.native_topk(maps[:, :na * (8 + with_dir)].contiguous(), anchors)
        assert torch.equal(boxes, boxes0) and torch.equal(scores, scores0)


def test_a_short_map_is_refused_without_the_head_as_before():
    c = IC.decode_case(IC.SHORT_ROW, 1, 1, False)
    plain = _layer(c["geom"], False, 0, enabled=False)
    B, n_cls, n_yaw, H, W, topk = c["geom"]
    with pytest.raises(RuntimeError):
        plain.native_topk(dev(c["maps"])[:, :n_cls * n_yaw * 8].contiguous(), dev(c["anchors"]))


def test_short_map_through_the_whole_stage():
    """6 anchors for TOPK = 10: the four sentinels keep score -1 and fall at the cut"""
    c = IC.decode_case(IC.SHORT_ROW, 1, 1, False)
    ref = c["by_power"][4]
    head = _layer(c["geom"], False, 4, thresh=(0.0,))
    got = head.finalize_native(*head.native_proposals(dev(c["maps"]), dev(c["anchors"])))
    want = IH.R._tail(ref["boxes"], ref["scores"], 1, 1, c["real"], (0.0,), 0.01)
    assert 0 < len(got[0]) == len(want["cand"]) <= c["real"] and float(got[3].min()) > 0
    np.testing.assert_allclose(got[3].cpu().numpy(), want["scores"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(got[0].cpu().numpy(), want["boxes"], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------- whole stage
STAGE_PARAMS = [(row, d, p) for row in C.STAGE_CASES for d in (False, True) for p in IC.POWERS]


@pytest.mark.parametrize("row,with_dir,power", STAGE_PARAMS, ids=[C.case_id(p) for p in STAGE_PARAMS])
def test_whole_stage(row, with_dir, power):
    """Kept candidates, their order and their scores equal the reference's; the keep list equals the torch statement's."""
    c = IC.stage_case(row, with_dir, power)
    ref = c["ref"]
    head = _layer(c["geom"], with_dir, power, thresh=c["thresh"])
    maps, anchors = dev(c["maps"]), dev(c["anchors"])
    got = head.finalize_native(*head.native_proposals(maps, anchors))
    assert len(got[0]) == len(ref["cand"]) > 0
    np.testing.assert_array_equal(got[1].cpu().numpy(), ref["batch"])
    np.testing.assert_array_equal(got[2].cpu().numpy(), ref["cls"])
    np.testing.assert_allclose(got[3].cpu().numpy(), ref["scores"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(got[0][:, :6].cpu().numpy(), ref["boxes"][:, :6], rtol=1e-5, atol=1e-6)
    assert np.abs(got[0][:, 6].cpu().numpy() - ref["boxes"][:, 6]).max() <= YAW_TOL
    # the op-by-op statement keeps the same candidates (equal scores: the two order ties differently -- compared as sets, rows sorted
    # by their x, then y)
    cls_map, reg_map = head.maps_from_fused(maps)
    stated = head.inference_from_maps(cls_map.clone(), reg_map, anchors, *head.extra_from_fused(maps))
    assert len(stated[0]) == len(got[0])
    rows = lambda r: (lambda a: a[np.lexsort((a[:, 1], a[:, 0]))])(np.concatenate((r[0].cpu().numpy(), r[3].cpu().numpy()[:, None]), 1))
    np.testing.assert_allclose(rows(stated), rows(got), rtol=1e-5, atol=1e-5)
    if power > 0:
        with pytest.raises(RuntimeError, match="IoU map"):
            head.inference_from_maps(cls_map.clone(), reg_map, anchors, head.dir_from_fused(maps))


# ------------------------------------------------------------------------------------------------------------------------- model
MODEL_BOUNDS = [0, -8.0, -3, 12.8, 8.0, 1]  # a 40 x 32 map


def _model(enabled=True, with_dir=False, power=4, drop_key=False):
    from vision3d_amd.detector import Second
    cfg = IC.make_cfg(1, enabled=enabled, power=power, with_dir=with_dir, bounds=MODEL_BOUNDS, thresh=(0.05,))
    if drop_key:
        del cfg["IOU_HEAD"]
    torch.manual_seed(0)
    return cfg, Second(cfg).cuda()


def _train_item(cfg, clouds):
    from vision3d_amd.core import AnchorGenerator, Preprocessor, ProposalTargetAssigner
    assigner = ProposalTargetAssigner(cfg)
    gts = [np.array([[4.2, -2.1, -1.0, 1.6, 3.9, 1.56, 0.05], [9.3, 3.3, -1.0, 1.6, 3.9, 1.56, 1.55 - math.pi]], np.float32),
           np.array([[6.1, 0.7, -1.0, 1.6, 3.9, 1.56, 3.2]], np.float32)]
    targets = [assigner(dict(boxes=torch.from_numpy(g), class_idx=torch.zeros(len(g), dtype=torch.long),
                             box_ignore=torch.zeros(len(g), dtype=torch.bool))) for g in gts]
    item = Preprocessor(cfg, seed=0)(dict(points=[torch.from_numpy(c).cuda() for c in clouds], anchors=AnchorGenerator(cfg).anchors.cuda()))
    keys = ("G_cls", "G_reg", "M_cls", "M_reg") + (("G_dir",) if cfg.DIRECTION.ENABLED else ())
    item.update({k: torch.stack([t[k] for t in targets]) for k in keys})
    return item


@pytest.mark.parametrize("with_dir", [False, True])
def test_enabled_model_trains_through_the_native_loss(with_dir):
    from vision3d_amd import synth
    from vision3d_amd.detector import ProposalLoss
    cfg, model = _model(with_dir=with_dir)
    model.train()
    item = _train_item(cfg, [synth.make_cloud(s, n_points=20000) for s in (0, 1)])
    assert int(item["M_reg"].sum()) > 0 and torch.is_tensor(item["anchors"])
    out = model(item)
    maps = out["_head_maps"]
    assert isinstance(maps, tuple) and maps[0].shape == (2, 18 + 2 * with_dir, 40, 32) and maps[0].dtype == torch.float32
    assert out["P_iou"].shape == out["P_cls"].shape == (2, 1, 2, 40, 32) and out["P_iou"] is maps[-1] and ("P_dir" in out) == with_dir
    losses = ProposalLoss(cfg)(out)
    assert type(losses["iou_loss"].grad_fn).__name__ == "FusedProposalIoULossFunctionBackward", "the loss took the native pass"
    assert torch.isfinite(losses["loss"]) and float(losses["iou_loss"].detach()) > 0 and ("dir_loss" in losses) == with_dir
    losses["loss"].backward()
    for p in (model.head.conv_iou.weight, model.head.conv_cls.weight, model.head.conv_reg.weight, model.rpn.down_block[1].weight):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
    stated = ProposalLoss(cfg)({k: v for k, v in out.items() if k != "_head_maps"})
    for k in losses:
        assert abs(float(losses[k].detach()) - float(stated[k].detach())) <= 1e-5 * max(1.0, abs(float(stated[k].detach()))), k


def _spread_logits(model, item):
    """unit spread of the class logits (no fp32 score ties between the two top-k's) and an IoU head with logits of both signs"""
    model.head.conv_cls.weight.normal_(0, 0.05)
    model.head.conv_iou.weight.normal_(0, 0.05)
    logits = model.head.conv_cls(model.feature_extract(item))
    assert float(logits.std()) > 1e-3
    model.head.conv_cls.weight.mul_(1.0 / logits.std())
    model.head.conv_cls.bias.zero_()
    z = model.head.conv_iou(model.feature_extract(item))
    model.head.conv_iou.weight.mul_(1.0 / z.std())


@pytest.mark.parametrize("with_dir", [False, True])
def test_enabled_model_inference_paths_agree_and_equal_the_statement(with_dir):
    """inference(item), inference_points and one graphed_inference capture + replay give equal arrays; they equal the op-by-op statement
    on the model's own maps, which differs from the same model's class-score order."""
    from gpu_util import randomize_bn
    from vision3d_amd import synth
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    cfg, model = _model(with_dir=with_dir)
    randomize_bn(model, 0)
    model.eval()
    anchors = AnchorGenerator(cfg).anchors.cuda()
    cloud = synth.make_cloud(3, n_points=20000)
    clouds = [torch.from_numpy(cloud).cuda()] if isinstance(cloud, np.ndarray) else [cloud.cuda()]
    item = Preprocessor(cfg)(dict(points=[cloud], anchors=anchors))
    with torch.no_grad():
        _spread_logits(model, item)
        got = [t.clone() for t in model.inference(item)]
        out = model(item)
        assert out["P_iou"].shape == out["P_cls"].shape == (1, 1, 2, 40, 32) and "_head_maps" not in out
        extra = ((out["P_dir"],) if with_dir else (None,)) + (out["P_iou"],)
        want = model.head.inference_from_maps(out["P_cls"].clone(), out["P_reg"], anchors, *extra)
        from_points = [t.clone() for t in model.inference_points(clouds, anchors)]
        from_torch = model.inference_points(clouds, anchors, proposals="torch")
        graphed = model.graphed_inference(anchors, [len(c) for c in clouds])
        from_graph = [t.clone() for t in graphed(clouds)]
    assert len(got[0]) == len(want[0]) > 1
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    np.testing.assert_allclose(got[3].cpu().numpy(), want[3].cpu().numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(got[0].cpu().numpy(), want[0].cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert len(from_torch[0]) == len(got[0])
    for other in (from_points, from_graph):
        for a, b in zip(other, got):
            np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert float(got[3].max()) < float(torch.sigmoid(out["P_cls"]).max()), "the scores are rectified"


def test_pillar_model_eager_path():
    """The pillar SECOND builds the same head: eager forward and inference carry the IoU map; inference equals the statement."""
    from vision3d_amd import synth
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    from vision3d_amd.core.config import pillar_car_cfg
    from vision3d_amd.detector import Second
    cfg = pillar_car_cfg()
    cfg.IOU_HEAD.ENABLED = True
    cfg.DIRECTION.ENABLED = True
    for a in cfg.ANCHORS:
        a["score_thresh"] = 0.05
    torch.manual_seed(0)
    model = Second(cfg).cuda().eval()
    anchors = AnchorGenerator(cfg).anchors.cuda()
    item = Preprocessor(cfg)(dict(points=[synth.make_cloud(0, n_points=16384)], anchors=anchors))
    with torch.no_grad():
        _spread_logits(model, item)
        out = model(dict(item))
        got = model.inference(item)
        want = model.head.inference_from_maps(out["P_cls"].clone(), out["P_reg"], anchors, out["P_dir"], out["P_iou"])
    assert out["P_iou"].shape == out["P_dir"].shape == out["P_cls"].shape == (1, 1, 2, 200, 176)
    assert len(got[0]) == len(want[0]) > 0
    np.testing.assert_allclose(got[3].cpu().numpy(), want[3].cpu().numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(got[0].cpu().numpy(), want[0].cpu().numpy(), rtol=1e-5, atol=1e-5)


def test_pipelined_inference_equals_eager():
    from gpu_util import randomize_bn
    from vision3d_amd import synth
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    cfg, model = _model(with_dir=True)
    randomize_bn(model, 0)
    model.eval()
    anchors = AnchorGenerator(cfg).anchors.cuda()
    cloud = synth.make_cloud(3, n_points=20000)
    clouds = [torch.from_numpy(cloud).cuda()]
    with torch.no_grad():
        _spread_logits(model, Preprocessor(cfg)(dict(points=[cloud], anchors=anchors)))
        want = [t.clone() for t in model.inference_points(clouds, anchors)]
        pipe = model.pipelined_inference(anchors, [len(clouds[0])], depth=2)
        pipe.submit(clouds)
        got = [t.clone() for t in pipe.collect()]
    assert len(want[0]) > 0
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())


def _stage_launches(head, maps, anchors):
    from torch.profiler import ProfilerActivity, profile
    head.native_proposals(maps, anchors)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        head.native_proposals(maps, anchors)
        torch.cuda.synchronize()
    return sum(ev.count for ev in prof.key_averages() if "prop_" in ev.key or "nms" in ev.key.lower())


def test_disabled_model_is_todays():
    """Keys, outputs bit for bit and the launch count of the stage: a config with the key disabled against one written before the key
    existed; the enabled head's stage takes the same number of launches."""
    from gpu_util import randomize_bn
    from vision3d_amd import synth
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    (cfg, model), (old_cfg, old) = _model(enabled=False), _model(drop_key=True)
    assert "IOU_HEAD" not in old_cfg
    assert sorted(k for k in model.state_dict() if k.startswith("head.")) == ["head.conv_cls.bias", "head.conv_cls.weight", "head.conv_reg.bias",
                                                                             "head.conv_reg.weight"]
    assert sorted(model.state_dict()) == sorted(old.state_dict())
    assert all(torch.equal(v, old.state_dict()[k]) for k, v in model.state_dict().items())
    for m in (model, old):
        randomize_bn(m, 0)
    anchors = AnchorGenerator(cfg).anchors.cuda()
    item = Preprocessor(cfg)(dict(points=[synth.make_cloud(3, n_points=20000)], anchors=anchors))
    model.eval(), old.eval()
    with torch.no_grad():
        a, b = model.inference(dict(item)), old.inference(dict(item))
        oa, ob = model(dict(item)), old(dict(item))
    assert len(a[0]) > 0 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert "P_iou" not in oa and torch.equal(oa["P_cls"], ob["P_cls"]) and torch.equal(oa["P_reg"], ob["P_reg"])
    model.train()
    out = model(_train_item(cfg, [synth.make_cloud(s, n_points=20000) for s in (0, 1)]))
    assert out["_head_maps"][0].shape == (2, 16, 40, 32) and len(out["_head_maps"]) == 3 and "P_iou" not in out
    # launches of the proposal stage on one map: disabled == before the key == enabled
    c = IC.decode_case((2, 40, 40, 256), 1, 1, False)
    maps, anc = dev(c["maps"]), dev(c["anchors"])
    plain, on = _layer(c["geom"], False, 4, enabled=False), _layer(c["geom"], False, 4)
    n_plain, n_on = _stage_launches(plain, maps[:, :16].contiguous(), anc), _stage_launches(on, maps, anc)
    print("iou-head-stage-launches", dict(disabled=n_plain, enabled=n_on))
    assert n_plain == n_on > 0

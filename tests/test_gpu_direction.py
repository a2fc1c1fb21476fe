"""GPU: the direction classifier and sine yaw loss of the anchor head (cfg.DIRECTION) -- targets (csrc/targets.hip
v3d_direction_targets), loss and gradient (csrc/proposal_loss.hip v3d_proposal_dir_loss_fwd_bwd), decode (csrc/proposal.hip
v3d_proposals_dir_topk / _flag) and the model -- against the float64 statements of tests/direction_ref.py and the torch statements.
tests/test_host_direction.py proves every case here well-posed on the reference alone.

Bounds of the loss test.  Focal term and the six unchanged box columns: those of tests/test_gpu_proposal_loss.py, 2e-6 relative on a
loss term and 1e-6 of the largest gradient.  Sine yaw term and BCE term: four times the error of the fp32 torch statement against
float64 on the same inputs (kernel sinf / cosf / expf / log1pf against torch's), measured by the test itself, never less than the
project bound.  Measured on an MI355X over LOSS_CASES (profiles/direction_head.txt): MEASURED_FP32_ERRORS below.
"""
import math

import numpy as np
import pytest
import torch

import direction_cases as DC
import direction_ref as D
import proposal_cases as C
from gpu_util import dev

pytestmark = pytest.mark.gpu

# largest error over LOSS_CASES, relative to max(1, |term|) for the loss terms and to the largest gradient of the map for the gradients:
# (the fp32 torch statement's, the fused kernel's) -- from profiles/direction_head.txt; the test measures them again on every run
MEASURED_FP32_ERRORS = {"reg_loss (sin yaw)": (4.38e-8, 2.98e-8), "dir_loss": (4.87e-8, 1.18e-7), "yaw_gradient (sin yaw)": (5.45e-7, 5.44e-7),
                        "dir_gradient": (1.35e-7, 1.42e-7), "cls_loss": (None, 6.60e-8), "cls_gradient": (None, 5.51e-7),
                        "box6_gradient": (6.00e-8, 7.36e-8), "decode yaw (rad)": (None, 8.90e-7)}
# (every figure lies below the project bound, so the bound that holds in every case is the project's: 2e-6 / 1e-6)
TERM_BOUND, GRAD_BOUND = 2e-6, 1e-6  # tests/test_gpu_proposal_loss.py
YAW_TOL = 1e-5


# ----------------------------------------------------------------------------------------------------------------------- targets
@pytest.mark.parametrize("case", DC.TARGET_CASES, ids=C.case_id)
def test_targets_equal_the_torch_statement_and_the_reference(case):
    from vision3d_amd.core import ProposalTargetAssigner
    n_gt, n_cls = case
    c = DC.target_case(*case)
    assigner = ProposalTargetAssigner(c["cfg"])
    assert tuple(assigner.anchors.shape) == (n_cls, 2, 5, 7, 7)
    item = dict(boxes=torch.from_numpy(c["boxes"]), class_idx=torch.from_numpy(c["class_idx"]), box_ignore=torch.zeros(n_gt, dtype=torch.bool))
    fused, ref = assigner(dict(item)), assigner.forward_torch(dict(item))
    for k in ("G_cls", "M_cls", "M_reg", "G_dir"):
        assert fused[k].dtype == ref[k].dtype and fused[k].shape == ref[k].shape, k
        assert torch.equal(fused[k], ref[k]), k
    assert fused["G_dir"].dtype == torch.int8 and fused["G_dir"].shape == fused["G_cls"].shape
    box_idx, _ = assigner.match_all_classes(item["boxes"].cuda(), item["class_idx"].cuda(), item["box_ignore"].cuda())
    want = D.targets(c["boxes"][:, 6].astype(np.float64), box_idx.cpu().numpy(), fused["M_reg"].cpu().numpy())
    got = fused["G_dir"].cpu().numpy()
    np.testing.assert_array_equal(got, want)
    pos = fused["M_reg"][..., 0].cpu().numpy()
    assert not got[~pos].any(), "G_dir is 0 off the positives"
    assert int(pos.sum()) >= n_gt, "every ground truth has a positive anchor"
    if n_gt == 3:
        assert set(got[pos].tolist()) == {0, 1}, "both bits among the positives"
    if n_gt == 0:
        assert not got.any()


# -------------------------------------------------------------------------------------------------------------------------- loss
def _fused(c, upstream=(2.0, 3.0, 5.0)):
    from vision3d_amd.detector import ProposalLoss
    cfg = DC.make_cfg(c["n_cls"], c["n_yaw"], sin_yaw=c["sin_yaw"])
    maps = dev(c["maps"]).requires_grad_(True)
    item = {k: dev(c[k]) for k in ("G_cls", "M_cls", "G_reg", "M_reg", "G_dir")}
    out = ProposalLoss(cfg)(dict(item, _head_maps=maps, P_cls=None, P_reg=None, P_dir=None))
    assert type(out["dir_loss"].grad_fn).__name__ == "FusedProposalDirLossFunctionBackward", "the native pass ran"
    (upstream[0] * out["cls_loss"] + upstream[1] * out["reg_loss"] + upstream[2] * out["dir_loss"]).backward()
    return out, maps.grad


def _statement(c, dtype, upstream=(2.0, 3.0, 5.0)):
    maps, out = DC.torch_statement(c, dtype, "cuda")
    (upstream[0] * out["cls_loss"] + upstream[1] * out["reg_loss"] + upstream[2] * out["dir_loss"]).backward()
    return {k: float(v.detach()) for k, v in out.items()}, maps.grad.double()


def _channel_groups(c):
    """-> dict of channel index arrays: class, the six unchanged box columns, the yaw column, direction"""
    n_cls, n_yaw = c["n_cls"], c["n_yaw"]
    na = n_cls * n_yaw
    box = na + ((np.arange(n_cls)[:, None, None] * 7 + np.arange(7)[None, :, None]) * n_yaw + np.arange(n_yaw)[None, None])
    return dict(cls=np.arange(na), box6=box[:, :6].reshape(-1), yaw=box[:, 6].reshape(-1), dir=np.arange(8 * na, 9 * na))


@pytest.mark.parametrize("case", DC.LOSS_CASES, ids=C.case_id)
def test_loss_and_gradient_against_the_float64_statement(case):
    """Upstream gradients (2, 3, 5).  The figures are printed before they are asserted (the docstring of this file)."""
    c = DC.loss_case(*case)
    ref, gref = _statement(c, torch.float64)
    own, gown = _statement(c, torch.float32)
    got, ggot = _fused(c)
    got = {k: float(v.detach()) for k, v in got.items()}
    ggot = ggot.double()
    gmax = max(float(gref.abs().max()), 1e-30)
    groups = _channel_groups(c)
    rel = lambda a, k: abs(a[k] - ref[k]) / max(1.0, abs(ref[k]))
    gerr = lambda g, ch: float((g[:, ch] - gref[:, ch]).abs().max()) / gmax
    sine = c["sin_yaw"]
    figures = dict(case=C.case_id(case), cls_loss=rel(got, "cls_loss"), reg_loss=rel(got, "reg_loss"), reg_loss_fp32_torch=rel(own, "reg_loss"),
                   dir_loss=rel(got, "dir_loss"), dir_loss_fp32_torch=rel(own, "dir_loss"), cls_gradient=gerr(ggot, groups["cls"]),
                   box6_gradient=gerr(ggot, groups["box6"]), yaw_gradient=gerr(ggot, groups["yaw"]),
                   yaw_gradient_fp32_torch=gerr(gown, groups["yaw"]), dir_gradient=gerr(ggot, groups["dir"]),
                   dir_gradient_fp32_torch=gerr(gown, groups["dir"]))
    print("direction-loss-figures", figures)
    assert figures["cls_loss"] <= TERM_BOUND
    assert figures["reg_loss"] <= (max(TERM_BOUND, 4 * figures["reg_loss_fp32_torch"]) if sine else TERM_BOUND)
    assert figures["dir_loss"] <= max(TERM_BOUND, 4 * figures["dir_loss_fp32_torch"])
    want_total = ref["cls_loss"] + 1.0 * ref["reg_loss"] + 0.2 * ref["dir_loss"]
    assert abs(ref["loss"] - want_total) <= 1e-12 * max(1.0, abs(want_total)), "loss = cls + LAMBDA reg + LOSS_WEIGHT dir"
    assert abs(got["loss"] - ref["loss"]) <= 3 * max(TERM_BOUND, 4 * figures["reg_loss_fp32_torch"], 4 * figures["dir_loss_fp32_torch"]) * max(1.0, abs(ref["loss"]))
    assert figures["cls_gradient"] <= GRAD_BOUND + 1e-12 and figures["box6_gradient"] <= GRAD_BOUND + 1e-12
    assert figures["yaw_gradient"] <= (max(GRAD_BOUND, 4 * figures["yaw_gradient_fp32_torch"]) if sine else GRAD_BOUND) + 1e-12
    assert figures["dir_gradient"] <= max(GRAD_BOUND, 4 * figures["dir_gradient_fp32_torch"]) + 1e-12
    if c["variant"] == "no_positives":
        na = c["n_cls"] * c["n_yaw"]
        assert got["reg_loss"] == 0.0 and got["dir_loss"] == 0.0 and float(ggot[:, na:].abs().max()) == 0.0


@pytest.mark.parametrize("case", [DC.LOSS_CASES[1], DC.LOSS_CASES[8]], ids=C.case_id)
def test_two_runs_are_bit_equal(case):
    c = DC.loss_case(*case)
    (a, ga), (b, gb) = _fused(c), _fused(c)
    for k in ("cls_loss", "reg_loss", "dir_loss", "loss"):
        assert torch.equal(a[k].detach(), b[k].detach()), k
    assert torch.equal(ga, gb)


@pytest.mark.parametrize("case", [DC.LOSS_CASES[0], DC.LOSS_CASES[1]], ids=C.case_id)
def test_upstream_gradients_scale_the_three_channel_groups_exactly(case):
    """Under upstream gradients (2, 3, 5) the backward returns the (1, 1, 1) gradient times 2 on the class channels, 3 on the box
    channels and 5 on the direction channels: one exact fp32 multiply per element.  5 x 7: two frames, no multiple of a wave."""
    c = DC.loss_case(*case)
    _, g1 = _fused(c, (1.0, 1.0, 1.0))
    _, g2 = _fused(c, (2.0, 3.0, 5.0))
    na = c["n_cls"] * c["n_yaw"]
    want = g1.clone()
    for lo, hi, f in ((0, na, 2.0), (na, 8 * na, 3.0), (8 * na, 9 * na, 5.0)):
        assert float(want[:, lo:hi].abs().max()) > 0
        want[:, lo:hi] *= f
    assert torch.equal(g2, want)


# ------------------------------------------------------------------------------------------------------------------------ decode
def _layers(geom, thresh=None):
    """-> (a ProposalLayer with the direction classifier, the plain one) for a case's geometry"""
    from vision3d_amd.detector.proposal import ProposalLayer
    B, n_cls, n_yaw, H, W, topk = geom
    return (ProposalLayer(DC.make_cfg(n_cls, n_yaw, topk, thresh=thresh)), ProposalLayer(DC.make_cfg(n_cls, n_yaw, topk, enabled=False, thresh=thresh)))


def _yaw_error(got, want):
    return np.abs(np.asarray(got, np.float64) - want)


@pytest.mark.parametrize("case", DC.DECODE_CASES, ids=C.case_id)
def test_decode(case):
    """native_topk: components 0-5 and the scores bit-equal to today's v3d_proposals_topk on the class / box channels, the yaw within
    1e-5 of the decode rule on the float64 raw yaw; at (1, 1) the first five candidates carry the hand-set logits."""
    c = DC.decode_case(*case)
    B, n_cls, n_yaw, H, W, topk = c["geom"]
    na = n_cls * n_yaw
    with_dir, plain = _layers(c["geom"])
    maps, anchors = dev(c["maps"]), dev(c["anchors"])
    boxes, scores = with_dir.native_topk(maps, anchors)
    boxes0, scores0 = plain.native_topk(maps[:, :na * 8].contiguous(), anchors)
    torch.cuda.synchronize()
    assert torch.equal(boxes[..., :6], boxes0[..., :6]) and torch.equal(scores, scores0)
    got = boxes.cpu().numpy().reshape(B, n_cls, topk, 7)
    np.testing.assert_allclose(got[..., :6], c["boxes"][..., :6], rtol=1e-5, atol=1e-6)
    err = _yaw_error(got[..., 6], c["yaw"])
    print("direction-decode-figures", dict(case=C.case_id(case), yaw_error=float(err.max())))
    assert err.max() <= YAW_TOL
    assert (got[..., 6] >= np.float32(D.OFFSET) - 1e-6).all() and (got[..., 6] < D.OFFSET + 2 * math.pi + 1e-6).all()
    if c["hand"] is not None:
        base = np.remainder(c["boxes"][0, 0, :5, 6] - D.OFFSET, math.pi) + D.OFFSET
        bits = np.round((got[0, 0, :5, 6] - base) / math.pi).astype(np.int64)
        assert bits.tolist() == DC.HAND_BITS.tolist(), "+0.0, -0.0, NaN and -1e-30 give bit 0; 1e-30 gives bit 1"
    # the torch statement of the same decode, on the reference's selection
    idx = dev(c["idx"])
    cls_map, reg_map = with_dir.maps_from_fused(maps)
    stated = with_dir._decode(reg_map, anchors, idx, with_dir.dir_from_fused(maps)).cpu().numpy()
    assert _yaw_error(stated[..., 6], c["yaw"]).max() <= YAW_TOL
    boxes2, scores2 = with_dir.native_topk(maps, anchors)
    assert torch.equal(boxes, boxes2) and torch.equal(scores, scores2), "two runs are bit-equal"


def test_whole_stage():
    """Kept candidates, their order and scores equal those of the plain stage on the same class / box channels (and the reference's);
    the yaws follow the decode rule."""
    c = DC.stage_case()
    ref = c["ref"]
    B, n_cls, n_yaw, H, W, topk = c["geom"]
    na = n_cls * n_yaw
    with_dir, plain = _layers(c["geom"], c["thresh"])
    maps, anchors = dev(c["maps"]), dev(c["anchors"])
    got = with_dir.finalize_native(*with_dir.native_proposals(maps, anchors))
    got0 = plain.finalize_native(*plain.native_proposals(maps[:, :na * 8].contiguous(), anchors))
    assert len(got[0]) == len(got0[0]) == len(ref["cand"]) > 0
    assert torch.equal(got[0][:, :6], got0[0][:, :6])
    for a, b in zip(got[1:], got0[1:]):
        assert torch.equal(a, b)
    np.testing.assert_array_equal(got[1].cpu().numpy(), ref["batch"])
    np.testing.assert_array_equal(got[2].cpu().numpy(), ref["cls"])
    np.testing.assert_allclose(got[3].cpu().numpy(), ref["scores"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(got[0][:, :6].cpu().numpy(), ref["boxes"][:, :6], rtol=1e-5, atol=1e-6)
    assert _yaw_error(got[0][:, 6].cpu().numpy(), c["yaw"][ref["cand"]]).max() <= YAW_TOL
    # the op-by-op statement with the direction map keeps the same candidates
    cls_map, reg_map = with_dir.maps_from_fused(maps)
    stated = with_dir.inference_from_maps(cls_map.clone(), reg_map, anchors, with_dir.dir_from_fused(maps))
    assert len(stated[0]) == len(got[0])
    # (equal lattice scores: the two statements order ties differently -- compared as sets, rows sorted by their x, then y)
    rows = lambda t: (lambda a: a[np.lexsort((a[:, 1], a[:, 0]))])(t.cpu().numpy())
    np.testing.assert_allclose(rows(stated[0]), rows(got[0]), rtol=1e-5, atol=1e-5)
    with pytest.raises(RuntimeError, match="direction map"):
        with_dir.inference_from_maps(cls_map.clone(), reg_map, anchors)


# ------------------------------------------------------------------------------------------------------------------------- model
MODEL_BOUNDS = [0, -8.0, -3, 12.8, 8.0, 1]  # a 40 x 32 map


def _model(enabled):
    from vision3d_amd.detector import Second
    cfg = DC.make_cfg(1, enabled=enabled, bounds=MODEL_BOUNDS, thresh=(0.05,))
    torch.manual_seed(0)
    return cfg, Second(cfg).cuda()


def _train_item(cfg, clouds):
    from vision3d_amd.core import Preprocessor, ProposalTargetAssigner
    assigner = ProposalTargetAssigner(cfg)
    gts = [np.array([[4.2, -2.1, -1.0, 1.6, 3.9, 1.56, 0.05], [9.3, 3.3, -1.0, 1.6, 3.9, 1.56, 1.55 - math.pi]], np.float32),
           np.array([[6.1, 0.7, -1.0, 1.6, 3.9, 1.56, 3.2]], np.float32)]
    targets = [assigner(dict(boxes=torch.from_numpy(g), class_idx=torch.zeros(len(g), dtype=torch.long),
                             box_ignore=torch.zeros(len(g), dtype=torch.bool))) for g in gts]
    item = Preprocessor(cfg, seed=0)(dict(points=[torch.from_numpy(c).cuda() for c in clouds]))
    keys = ("G_cls", "G_reg", "M_cls", "M_reg") + (("G_dir",) if cfg.DIRECTION.ENABLED else ())
    item.update({k: torch.stack([t[k] for t in targets]) for k in keys})
    return item


def test_enabled_model_trains_through_the_native_loss():
    from vision3d_amd import synth
    from vision3d_amd.detector import ProposalLoss
    cfg, model = _model(True)
    model.train()
    item = _train_item(cfg, [synth.make_cloud(s, n_points=20000) for s in (0, 1)])
    assert int(item["M_reg"].sum()) > 0 and set(item["G_dir"][item["M_reg"][..., 0]].tolist()) == {0, 1}
    out = model(item)
    maps = out["_head_maps"]
    assert isinstance(maps, tuple) and maps[0].shape == (2, 18, 40, 32) and maps[0].dtype == torch.float32
    assert out["P_dir"].shape == out["P_cls"].shape == (2, 1, 2, 40, 32) and out["P_dir"] is maps[3]
    losses = ProposalLoss(cfg)(out)
    assert type(losses["dir_loss"].grad_fn).__name__ == "FusedProposalDirLossFunctionBackward", "the loss took the native pass"
    assert torch.isfinite(losses["loss"]) and float(losses["dir_loss"].detach()) > 0
    losses["loss"].backward()
    for p in (model.head.conv_dir.weight, model.head.conv_cls.weight, model.head.conv_reg.weight, model.rpn.down_block[1].weight):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
    # ... and equals the torch expressions on the same outputs
    stated = ProposalLoss(cfg)({k: v for k, v in out.items() if k != "_head_maps"})
    for k in ("cls_loss", "reg_loss", "dir_loss", "loss"):
        assert abs(float(losses[k].detach()) - float(stated[k].detach())) <= 1e-5 * max(1.0, abs(float(stated[k].detach()))), k


def test_enabled_model_inference_equals_the_statement_with_the_direction_map():
    from vision3d_amd import synth
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    from gpu_util import randomize_bn
    cfg, model = _model(True)
    randomize_bn(model, 0)  # (a fresh model's features vanish: non-trivial BatchNorm statistics, as tests/test_gpu_second.py builds its model)
    model.eval()
    anchors = AnchorGenerator(cfg).anchors.cuda()
    item = Preprocessor(cfg)(dict(points=[synth.make_cloud(3, n_points=20000)], anchors=anchors))
    with torch.no_grad():
        # unit spread of the class logits (no fp32 score ties between the two top-k's) and a direction head with logits of both signs
        model.head.conv_cls.weight.normal_(0, 0.05)
        model.head.conv_dir.weight.normal_(0, 0.05)
        logits = model.head.conv_cls(model.feature_extract(item))
        assert float(logits.std()) > 1e-3
        model.head.conv_cls.weight.mul_(1.0 / logits.std())
        model.head.conv_cls.bias.zero_()
        boxes, bidx, cidx, scores = model.inference(item)
        out = model(item)
        assert out["P_dir"].shape == out["P_cls"].shape == (1, 1, 2, 40, 32) and "_head_maps" not in out
        want = model.head.inference_from_maps(out["P_cls"].clone(), out["P_reg"], anchors, out["P_dir"])
    assert len(boxes) == len(want[0]) > 0
    assert torch.equal(bidx, want[1]) and torch.equal(cidx, want[2])
    np.testing.assert_allclose(scores.cpu().numpy(), want[3].cpu().numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(boxes.cpu().numpy(), want[0].cpu().numpy(), rtol=1e-5, atol=1e-5)
    yaw = boxes[:, 6].cpu().numpy()
    assert (yaw >= np.float32(D.OFFSET) - 1e-6).all() and (yaw < D.OFFSET + 2 * math.pi + 1e-6).all()


def test_disabled_model_is_todays():
    from vision3d_amd import synth
    cfg, model = _model(False)
    assert sorted(k for k in model.state_dict() if k.startswith("head.")) == ["head.conv_cls.bias", "head.conv_cls.weight", "head.conv_reg.bias",
                                                                             "head.conv_reg.weight"]
    model.train()
    out = model(_train_item(cfg, [synth.make_cloud(s, n_points=20000) for s in (0, 1)]))
    assert out["_head_maps"][0].shape == (2, 16, 40, 32) and len(out["_head_maps"]) == 3 and "P_dir" not in out

"""GPU: a PV-RCNN train step through both stages -- PV_RCNN.train_forward + ProposalLoss + RefinementLoss + backward -- on a
device-preprocessed synthetic batch.  A randomly initialised head proposes nothing that overlaps a ground truth, so the instance's
`stage1_proposals` is replaced by RoIs jittered from the ground truth (synth.jitter_rois); everything else is the model's own."""
import numpy as np
import pytest
import torch

from vision3d_amd import synth
from vision3d_amd.core.config import second_car_cfg

pytestmark = pytest.mark.gpu

B = 2


def _batch(cfg):
    from vision3d_amd.core import AnchorGenerator, Preprocessor, ProposalTargetAssigner
    clouds = synth.make_kitti_batch(B)
    gts = [torch.from_numpy(synth.make_gt_boxes(s)) for s in range(B)]
    item = Preprocessor(cfg, seed=0)(dict(points=clouds))
    item["anchors"] = AnchorGenerator(cfg).anchors.cuda()
    item["boxes"] = gts
    item["class_idx"] = [torch.zeros(len(g), dtype=torch.long) for g in gts]
    assigner = ProposalTargetAssigner(cfg)
    per_frame = [assigner(dict(boxes=g, class_idx=c, box_ignore=torch.zeros(len(g), dtype=torch.bool))) for g, c in zip(gts, item["class_idx"])]
    for k in ("G_cls", "G_reg", "M_cls", "M_reg"):
        item[k] = torch.stack([t[k] for t in per_frame]).cuda()
    rng = np.random.default_rng(123)
    topk = cfg.PROPOSAL.TOPK
    rois = torch.from_numpy(np.stack([synth.jitter_rois(g.numpy(), topk, rng) for g in gts])).cuda()
    item["refine_draws"] = torch.from_numpy(rng.random((B, topk)).astype(np.float32)).cuda()
    samples = torch.from_numpy(rng.random((B, topk, cfg.GRIDPOOL.NUM_GRIDPOINTS, 3)).astype(np.float32)).cuda()
    return item, rois, samples


def _model(cfg, rois, seed=0):
    from vision3d_amd.detector import PV_RCNN
    torch.manual_seed(seed)
    model = PV_RCNN(cfg).cuda().train()
    topk = cfg.PROPOSAL.TOPK
    model.stage1_proposals = lambda item: (rois, torch.ones(rois.shape[:2], device=rois.device),
                                           torch.zeros(topk, dtype=torch.long, device=rois.device))
    return model


def _step(model, cfg, item, samples, seed=1):
    from vision3d_amd.detector import ProposalLoss, RefinementLoss
    torch.manual_seed(seed)  # (the padding draws of the sparse levels come from the global generator)
    out = model.train_forward(dict(item), samples)
    return out, ProposalLoss(cfg)(out), RefinementLoss(cfg)(out)


def _grads(model):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}


def test_train_step_reaches_every_stage2_parameter_and_repeats():
    cfg = second_car_cfg()
    item, rois, samples = _batch(cfg)
    model = _model(cfg, rois)
    out, l1, l2 = _step(model, cfg, item, samples)
    assert int(out["M_rreg"].sum()) > 0 and int(out["M_rcls"].sum()) > 0
    assert out["R_reg"].shape == (B, cfg.PROPOSAL.TOPK, 7) and out["R_cls"].shape == (B, cfg.PROPOSAL.TOPK, 1)
    assert not out["proposals"].requires_grad
    # the stage-2 loss alone: nothing reaches the stage-1 head (the proposals are constants), everything of stage 2 is reached
    l2["loss"].backward(retain_graph=True)
    g2 = _grads(model)
    for n, g in g2.items():
        if n.startswith("proposal_layer."):
            assert g is None or not bool(g.any()), n
        if n.startswith(("refinement_layer.", "roi_grid_pool.", "pnets.")):
            assert g is not None and bool(torch.isfinite(g).all()) and bool(g.ne(0).any()), n
    assert any(bool(g.ne(0).any()) for n, g in g2.items() if n.startswith("cnn.") and g is not None)
    # + the stage-1 loss: now the head has its gradient
    l1["loss"].backward()
    g12 = _grads(model)
    for n, g in g12.items():
        assert g is not None and bool(torch.isfinite(g).all()), n
        if n.startswith("proposal_layer."):
            assert bool(g.ne(0).any()), n
    # a second model from the same seed, samples and draws: bit-equal losses; gradients to 1e-4 (the scatter-add backward of the
    # torch gathers uses atomics)
    model_b = _model(cfg, rois)
    out_b, l1_b, l2_b = _step(model_b, cfg, item, samples)
    for k in ("loss", "refine_cls_loss", "refine_reg_loss"):
        assert torch.equal(l2[k].detach(), l2_b[k].detach()), k
    assert torch.equal(l1["loss"].detach(), l1_b["loss"].detach())
    (l1_b["loss"] + l2_b["loss"]).backward()
    # rtol 1e-4 per parameter tensor in the 2-norm: the differences come from fp32 sums taken in another order, whose error is
    # relative to the summed magnitudes, not to each element (elements that are cancellation residue have no relative accuracy of
    # their own) -- the form tests/test_gpu_proposal_loss.py uses for the gradients behind a reordered backward
    rel = {n: float((g - g12[n]).norm() / g12[n].norm().clamp_min(1e-30)) for n, g in _grads(model_b).items()}
    print("largest per-tensor relative gradient differences between two runs:", sorted(rel.items(), key=lambda t: -t[1])[:5])
    for n, r in rel.items():
        assert r <= 1e-4, (n, r)


def test_ten_adam_steps_lower_the_stage2_loss_and_inference_still_answers():
    cfg = second_car_cfg()
    item, rois, samples = _batch(cfg)
    model = _model(cfg, rois)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    history = []
    for _ in range(10):
        opt.zero_grad()
        _, l1, l2 = _step(model, cfg, item, samples)
        (l1["loss"] + l2["loss"]).backward()
        opt.step()
        history.append(float(l2["loss"].detach()))
    print("stage-2 loss over ten Adam steps:", [round(v, 5) for v in history])
    assert all(np.isfinite(history)) and history[-1] < history[0]
    del model.stage1_proposals  # the class's own method again
    model.eval()
    with torch.no_grad():
        boxes, batch_idx, class_idx, scores = model.inference(dict(item))
    n = boxes.shape[0]
    assert boxes.shape == (n, 7) and batch_idx.shape == (n,) and class_idx.shape == (n,) and scores.shape == (n,)
    assert bool(torch.isfinite(boxes).all()) and bool(torch.isfinite(scores).all())

"""GPU: PV-RCNN's Predicted Keypoint Weighting (csrc/keypoint_weight.hip, detector/keypoint_weighting.py) -- the native tail of the
head against the float64 restatement (tests/keypoint_weighting_ref.py) under the bar of the torch float32 statements' own error, the
labels of the fused loss exactly against v3d_points_in_boxes, loss and gradient against the restatement, and the module inside
PV_RCNN (native against op-by-op inference, the pipelined form, a train step, and bit-identical outputs when disabled)."""
import numpy as np
import pytest
import torch

import keypoint_weighting_ref as R
from gpu_util import assert_fp32_class, dev
from vision3d_amd import synth
from vision3d_amd.core.config import second_car_cfg

pytestmark = pytest.mark.gpu


def pkw_cfg(**kw):
    cfg = second_car_cfg()
    cfg.PKW.merge_from_dict(dict(ENABLED=True, **kw))
    return cfg


# ---- kernel A
def _weight_case(rows, c, h, seed):
    rng = np.random.default_rng(seed)
    hidden = np.maximum(rng.normal(0, 1, (rows, h)), 0).astype(np.float32)  # (behind a ReLU)
    w2 = rng.normal(0, 2.0 / np.sqrt(h), h).astype(np.float32)
    b2 = np.array([0.3], np.float32)
    feats = rng.normal(0, 1, (rows, c)).astype(np.float32)
    return hidden, w2, b2, feats


@pytest.mark.parametrize("rows,c,h", [(1, 512, 256), (67, 512, 256), (130, 36, 20)])
@pytest.mark.parametrize("block", [False, True])
def test_keypoint_weight_kernel(rows, c, h, block):
    """A tail wave (67, 130 rows: no multiple of the workgroup's 4), one row, widths below one wave's span of 256 columns (36, 20);
    `block`: the rows are a column block of a wider matrix, whose other columns must come back untouched."""
    from vision3d_amd.detector.keypoint_weighting import keypoint_weight
    hidden, w2, b2, feats = _weight_case(rows, c, h, seed=rows)
    logits64 = hidden.astype(np.float64) @ w2.astype(np.float64) + np.float64(b2[0])
    weighted64 = feats.astype(np.float64) * R.sigmoid(logits64)[:, None]
    assert float(np.abs(logits64).max()) > 1.0 or rows == 1
    th, tw, tb, tf = dev(hidden), dev(w2), dev(b2), dev(feats)
    own_logits = th @ tw + tb  # the torch float32 statements on the same inputs
    own_weighted = tf * torch.sigmoid(own_logits)[:, None]

    def run():
        if block:
            wide = torch.full((rows, c + 24), -7.0, device="cuda")
            wide[:, 8:8 + c] = tf
            view = wide[:, 8:8 + c]
        else:
            wide = view = tf.clone()
        logits = keypoint_weight(th, tw, tb, view)
        return logits, view.clone(), wide

    logits, weighted, wide = run()
    if block:
        assert bool((wide[:, :8] == -7.0).all()) and bool((wide[:, 8 + c:] == -7.0).all()), "columns outside the block changed"
    print(f"[keypoint_weight {rows}x{c}x{h} block={block}] max |logit err| {np.abs(logits.cpu().numpy() - logits64).max():.3e} "
          f"(torch fp32: {np.abs(own_logits.cpu().numpy() - logits64).max():.3e})")
    assert_fp32_class(logits.cpu().numpy(), own_logits.cpu().numpy(), "logits", ref64=logits64, own_factor=2.0)
    assert_fp32_class(weighted.cpu().numpy(), own_weighted.cpu().numpy(), "weighted rows", ref64=weighted64, own_factor=2.0)
    logits_b, weighted_b, _ = run()
    assert torch.equal(logits, logits_b) and torch.equal(weighted, weighted_b), "two runs differ"


def test_keypoint_weighting_module_native_against_torch_and_float64():
    """KeypointWeighting.weight_point_major (linear_rows + the kernel, in place on a column view) and `forward` against forward_torch
    and the float64 restatement; a head with two hidden layers takes the torch statements."""
    from vision3d_amd.detector import KeypointWeighting
    torch.manual_seed(11)
    module = KeypointWeighting(pkw_cfg(), 512).cuda().eval()
    with torch.no_grad():
        for m in module.mlp:
            if isinstance(m, torch.nn.Linear):
                m.weight.normal_(0, 1.5 / m.in_features ** 0.5)
                m.bias.normal_(0, 0.5)
    layers = [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in module.mlp if isinstance(m, torch.nn.Linear)]
    feats = torch.randn(2, 67, 512, device="cuda", generator=torch.Generator(device="cuda").manual_seed(12))
    want_w, want_l = R.weight(feats.cpu().numpy(), layers)
    with torch.no_grad():
        own_w, own_l = module.forward_torch(feats.transpose(1, 2))
        pm = feats.clone()
        assert module.native_ok(pm)
        logits = module.weight_point_major(pm)
        fw, fl = module(feats.transpose(1, 2))
    assert torch.equal(fl, logits) and torch.equal(fw.transpose(1, 2), pm)
    assert_fp32_class(logits.cpu().numpy(), own_l.cpu().numpy(), "module logits", ref64=want_l, own_factor=2.0)
    assert_fp32_class(pm.cpu().numpy(), own_w.transpose(1, 2).cpu().numpy(), "module weighted", ref64=want_w, own_factor=2.0)
    assert torch.is_grad_enabled() and not module.native_ok(feats)  # under autograd: the torch statements
    deep = KeypointWeighting(pkw_cfg(MLPS=[64, 32]), 512).cuda().eval()
    with torch.no_grad():
        assert not deep.native_ok(feats)
        a, b = deep(feats.transpose(1, 2)), deep.forward_torch(feats.transpose(1, 2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- kernel B
def _pib_any(kp, boxes, class_idx, extra=None):
    """any over each frame's boxes (class >= 0) of v3d_points_in_boxes; `extra`: the boxes' wlh grown in float32 on the host."""
    from vision3d_amd.core.geometry import points_in_boxes_mask
    out = np.zeros(kp.shape[:2], bool)
    for b in range(kp.shape[0]):
        bx = boxes[b][class_idx[b] >= 0]
        if extra is not None:
            bx = R.grow(bx, extra)
        if len(bx):
            out[b] = points_in_boxes_mask(dev(kp[b]), dev(bx), True).any(1).cpu().numpy()
    return out


def _item(kp, boxes, class_idx, logits=None):
    item = dict(keypoints=dev(kp), boxes=[dev(b) for b in boxes], class_idx=[torch.from_numpy(c).cuda() for c in class_idx])
    if logits is not None:
        item["K_cls"] = dev(logits.astype(np.float32)).requires_grad_(True)
    return item


@pytest.mark.parametrize("extra", [(0.0, 0.0, 0.0), R.EXTRA, R.BIG_EXTRA])
def test_labels_equal_points_in_boxes_exactly(extra):
    from vision3d_amd.detector.keypoint_weighting import keypoint_labels, keypoint_labels_torch
    kp, boxes, class_idx = R.make_label_case()
    want = R.labels(kp, boxes, class_idx, extra)
    if any(extra):  # the restatement alone decides that the case is not trivial
        assert min(int((want == v).sum()) for v in (0, 1, R.IGNORE)) >= 5
    item = _item(kp, boxes, class_idx)
    got = keypoint_labels(item["keypoints"], item["boxes"], item["class_idx"], extra)
    assert got.dtype == torch.uint8 and got.shape == (3, 70)
    got = got.cpu().numpy()
    fg = _pib_any(kp, boxes, class_idx)
    near = _pib_any(kp, boxes, class_idx, extra)
    np.testing.assert_array_equal(got == 1, fg)
    np.testing.assert_array_equal(got == R.IGNORE, near & ~fg)
    np.testing.assert_array_equal(got == 0, ~near & ~fg)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(keypoint_labels_torch(item["keypoints"], item["boxes"], item["class_idx"], extra).cpu().numpy(), want)


@pytest.mark.parametrize("alpha,gamma", [(0.25, 2.0), (0.4, 1.5)])
def test_seg_loss_and_gradient_against_float64(alpha, gamma):
    from vision3d_amd.detector import KeypointSegLoss
    kp, boxes, class_idx = R.make_label_case()
    logits = np.random.default_rng(5).normal(0, 2.5, kp.shape[:2]).astype(np.float32)
    cfg = pkw_cfg(FOCAL_ALPHA=alpha, FOCAL_GAMMA=gamma, LOSS_WEIGHT=0.5)
    loss = KeypointSegLoss(cfg)
    lab = R.labels(kp, boxes, class_idx, R.EXTRA)
    want = R.loss(logits, lab, alpha, gamma)

    def fused():
        item = _item(kp, boxes, class_idx, logits)
        out = loss(item)
        counts = out["keypoint_seg_loss"].grad_fn.counts.clone()
        (3.0 * out["loss"]).backward()
        return out, item, counts

    out, item, counts = fused()
    own_item = _item(kp, boxes, class_idx, logits)
    own = loss.forward_torch(own_item)
    (3.0 * own["loss"]).backward()
    np.testing.assert_array_equal(item["K_label"].cpu().numpy(), lab)
    assert item["K_label"].dtype == torch.uint8 and torch.equal(own_item["K_label"], item["K_label"])
    assert counts.tolist() == [float(want["n_fg"]), float(want["n_ignored"])]
    got_l, own_l = float(out["keypoint_seg_loss"].detach()), float(own["keypoint_seg_loss"].detach())
    e, e_own = abs(got_l - want["keypoint_seg_loss"]) / want["keypoint_seg_loss"], abs(own_l - want["keypoint_seg_loss"]) / want["keypoint_seg_loss"]
    print(f"[seg loss a={alpha} g={gamma}] fused {got_l:.9g} torch {own_l:.9g} float64 {want['keypoint_seg_loss']:.12g}: rel err {e:.2e} (torch: {e_own:.2e})")
    assert e <= max(2e-4, 2 * e_own)  # (gpu_util's rule on one number: strict relative error, 2e-4 or twice the torch statement's own)
    assert float(out["loss"].detach()) == pytest.approx(0.5 * got_l, rel=1e-6)
    g64 = 1.5 * want["d_logits"]
    assert_fp32_class(item["K_cls"].grad.cpu().numpy(), own_item["K_cls"].grad.cpu().numpy(), "d_logits", ref64=g64, own_factor=2.0)
    assert not item["K_cls"].grad.cpu().numpy()[lab == R.IGNORE].any()
    out_b, item_b, counts_b = fused()
    assert torch.equal(out["keypoint_seg_loss"].detach(), out_b["keypoint_seg_loss"].detach()) and torch.equal(counts, counts_b)
    assert torch.equal(item["K_cls"].grad, item_b["K_cls"].grad) and torch.equal(item["K_label"], item_b["K_label"])


def test_upstream_gradient_scales_the_stored_gradient_exactly():
    """Backward under an upstream gradient of 2 (and of 3) is the stored gradient -- what a backward under 1 returns -- times it, one
    exact fp32 multiply per element.  B = 2, K = 257: 514 rows, two workgroups and two elements over; one scalar for the whole buffer."""
    from vision3d_amd.detector import KeypointSegLoss
    kp, boxes, class_idx = R.make_label_case(K=257)
    kp, boxes, class_idx = kp[1:], boxes[1:], class_idx[1:]
    logits = np.random.default_rng(7).normal(0, 2.5, kp.shape[:2]).astype(np.float32)
    loss = KeypointSegLoss(pkw_cfg())
    grads = {}
    for up in (1.0, 2.0, 3.0):
        item = _item(kp, boxes, class_idx, logits)
        (up * loss(item)["keypoint_seg_loss"]).backward()
        grads[up] = item["K_cls"].grad
    assert grads[1.0].shape == (2, 257) and float(grads[1.0].abs().max()) > 0
    assert torch.equal(grads[2.0], 2.0 * grads[1.0]) and torch.equal(grads[3.0], 3.0 * grads[1.0])


def test_seg_loss_without_ground_truth_and_with_an_empty_frame():
    from vision3d_amd.detector import KeypointSegLoss
    kp, boxes, class_idx = R.make_label_case()
    logits = np.random.default_rng(6).normal(0, 2.5, kp.shape[:2]).astype(np.float32)
    loss = KeypointSegLoss(pkw_cfg())
    empty = [np.zeros((0, 7), np.float32)] * 3, [np.zeros(0, np.int64)] * 3
    item = _item(kp, *empty, logits)
    out = loss(item)  # n_gt == 0
    want = R.loss(logits, np.zeros(kp.shape[:2], np.uint8))
    assert not bool(item["K_label"].any()) and out["keypoint_seg_loss"].grad_fn.counts.tolist() == [0.0, 0.0]
    assert float(out["keypoint_seg_loss"].detach()) == pytest.approx(want["keypoint_seg_loss"], rel=2e-4)
    out["loss"].backward()
    own_item = _item(kp, *empty, logits)
    loss.forward_torch(own_item)["loss"].backward()
    assert_fp32_class(item["K_cls"].grad.cpu().numpy(), own_item["K_cls"].grad.cpu().numpy(), "d_logits without ground truth",
                      ref64=want["d_logits"], own_factor=2.0)
    # frame 0 of the label case owns an empty range of the offsets: all of its labels are 0
    item = _item(kp, boxes, class_idx, logits)
    loss(item)
    assert not bool(item["K_label"][0].any()) and bool(item["K_label"][1:].any())


# ---- the module inside PV_RCNN
def _frames(cfg, batch, seed0=40):
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    anchors = AnchorGenerator(cfg).anchors.cuda()
    clouds = [synth.make_cloud(seed0 + i) for i in range(batch)]
    return lambda: Preprocessor(cfg, seed=0)(dict(points=clouds, anchors=anchors))


def _pv_rcnn(cfg, seed):
    from vision3d_amd.detector import PV_RCNN
    torch.manual_seed(seed)
    model = PV_RCNN(cfg).cuda().eval()
    with torch.no_grad():  # scores that straddle the class threshold and overlapping boxes, as tests/test_gpu_pointops.py sets them
        model.proposal_layer.conv_cls.bias.fill_(0.3)
        model.refinement_layer.mlp[-1].bias[7] = 0.2
        model.refinement_layer.mlp[-1].weight.mul_(30.0)
        if hasattr(model, "keypoint_weighting"):  # weights that move the scores away from 1/2
            for m in model.keypoint_weighting.mlp:
                if isinstance(m, torch.nn.Linear):
                    m.weight.normal_(0, 1.5 / m.in_features ** 0.5)
            model.keypoint_weighting.mlp[-1].bias.fill_(-2.0)  # (most keypoints are background: the usual focal-loss prior)
    return model


def test_pv_rcnn_inference_native_weighting_equals_the_torch_statements():
    batch = 2
    cfg = pkw_cfg()
    model = _pv_rcnn(cfg, 21)
    make = _frames(cfg, batch)
    n = cfg.NUM_CLASSES * cfg.PROPOSAL.TOPK
    samples = torch.rand((batch, n, cfg.GRIDPOOL.NUM_GRIDPOINTS, 3), generator=torch.Generator().manual_seed(22)).cuda()
    outs = {}
    with torch.no_grad():
        for native in (True, False):
            model.native_tail = model.keypoint_weighting.native = native
            model.cnn.pad_generator = torch.Generator(device="cuda").manual_seed(23)
            item = make()
            dets = model.inference(item, samples)
            outs[native] = (dets, item["proposals"].clone(), item["boxes_refined"].clone(), item["K_cls"].clone(), item["keypoint_features"].clone())
        # the float64 yardstick of K_cls: the restated head on the unweighted features of the same frame
        model.native_tail = model.keypoint_weighting.native = True
        model.cnn.pad_generator = torch.Generator(device="cuda").manual_seed(23)
        item = model.proposal(make())
        raw = model._keypoint_features(item, item["_cnn_features"], item["_bev_map"]).clone()
    layers = [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in model.keypoint_weighting.mlp if isinstance(m, torch.nn.Linear)]
    want_w, want_l = R.weight(raw.transpose(1, 2).cpu().numpy(), layers)
    (da, pa, ra, ka, fa), (db, pb, rb, kb, fb) = outs[True], outs[False]
    print(f"[K_cls] min {float(ka.min()):.4f} max {float(ka.max()):.4f} std {float(ka.std()):.4f}; smallest |K_cls| {float(ka.abs().min()):.3e}")
    assert ka.shape == (batch, cfg.NUM_KEYPOINTS) and float(ka.std()) > 1e-3  # (the scores differ from keypoint to keypoint)
    assert_fp32_class(ka.cpu().numpy(), kb.cpu().numpy(), "K_cls", ref64=want_l, own_factor=2.0)
    assert_fp32_class(fa.transpose(1, 2).cpu().numpy(), fb.transpose(1, 2).cpu().numpy(), "weighted keypoint features", ref64=want_w, own_factor=2.0)
    # stage-2 outputs: the bars of tests/test_gpu_pointops.py::test_pv_rcnn_native_proposal_tail_equals_the_torch_statements
    torch.testing.assert_close(pa, pb, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(ra, rb, rtol=1e-5, atol=1e-5)
    assert len(da[0]) == len(db[0]) and 0 < len(da[0]) < batch * n, (len(da[0]), len(db[0]))
    assert torch.equal(da[1], db[1]) and torch.equal(da[2], db[2])
    torch.testing.assert_close(da[3], db[3], rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(da[0], db[0], rtol=1e-5, atol=1e-5)


def test_pv_rcnn_pipelined_inference_equals_inference_with_weighting():
    cfg = pkw_cfg()
    model = _pv_rcnn(cfg, 0)
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    anchors = AnchorGenerator(cfg).anchors.cuda()
    pre = Preprocessor(cfg, seed=0)
    clouds = [[torch.from_numpy(synth.make_cloud(s, 16384)).cuda()] for s in range(3)]
    samples = torch.rand(1, cfg.NUM_CLASSES * model.proposal_layer.TOPK, cfg.GRIDPOOL.NUM_GRIDPOINTS, 3, device="cuda")
    item = lambda i: pre(dict(points=clouds[i], anchors=anchors))
    with torch.no_grad():
        want, logits = [], []
        for i in range(len(clouds)):
            it = item(i)
            want.append([t.clone() for t in model.inference(it, samples)])
            logits.append(it["K_cls"].clone())
        got, prev, items = [], None, [item(i) for i in range(len(clouds))]
        st = model.inference_begin(items[0], 0)
        for i in range(len(clouds)):
            nxt = model.inference_begin(items[i + 1], (i + 1) % 2) if i + 1 < len(clouds) else None
            h = model.inference_end(st, samples)
            if prev is not None:
                got.append([t.clone() for t in model.inference_collect(prev)])
            prev, st = h, nxt
        got.append([t.clone() for t in model.inference_collect(prev)])
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert torch.equal(a, b)
    for it, l in zip(items, logits):
        assert torch.equal(it["K_cls"], l)


def test_pv_rcnn_disabled_equals_a_configuration_without_the_key():
    make = _frames(second_car_cfg(), 1)
    outs = []
    for drop in (True, False):
        cfg = second_car_cfg()
        if drop:
            del cfg["PKW"]
        model = _pv_rcnn(cfg, 21)
        model.cnn.pad_generator = torch.Generator(device="cuda").manual_seed(23)
        n = cfg.NUM_CLASSES * cfg.PROPOSAL.TOPK
        samples = torch.rand((1, n, cfg.GRIDPOOL.NUM_GRIDPOINTS, 3), generator=torch.Generator().manual_seed(22)).cuda()
        with torch.no_grad():
            item = make()
            dets = model.inference(item, samples)
        assert "K_cls" not in item
        outs.append([t.clone() for t in dets] + [item["keypoint_features"].clone(), item["R_reg"].clone(), item["R_cls"].clone()])
    assert len(outs[0][0]) > 0
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_train_step_with_keypoint_seg_loss():
    """train_forward + ProposalLoss + RefinementLoss + KeypointSegLoss, backward: the head's parameters get finite, nonzero
    gradients; the gradient of the fused loss on them against the torch statement's (`_fused` off) and a float64 evaluation of the
    head and the loss on the same features, under the 2 x own rule."""
    from vision3d_amd.core import AnchorGenerator, Preprocessor, ProposalTargetAssigner
    from vision3d_amd.detector import PV_RCNN, KeypointSegLoss, KeypointWeighting, ProposalLoss, RefinementLoss
    B = 2
    cfg = pkw_cfg()
    gts = [torch.from_numpy(synth.make_gt_boxes(s)) for s in range(B)]
    item = Preprocessor(cfg, seed=0)(dict(points=synth.make_kitti_batch(B)))
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
    torch.manual_seed(0)
    model = PV_RCNN(cfg).cuda().train()
    model.stage1_proposals = lambda it: (rois, torch.ones(rois.shape[:2], device=rois.device), torch.zeros(topk, dtype=torch.long, device=rois.device))
    seg_loss = KeypointSegLoss(cfg)
    seen = []  # the features the head saw
    hook = model.keypoint_weighting.mlp[0].register_forward_pre_hook(lambda m, args: seen.append(args[0].detach()))
    torch.manual_seed(1)
    out = model.train_forward(dict(item), samples)
    hook.remove()
    assert out["K_cls"].shape == (B, cfg.NUM_KEYPOINTS) and out["K_cls"].requires_grad
    assert out["K_label"].dtype == torch.uint8 and out["K_label"].shape == (B, cfg.NUM_KEYPOINTS)
    label_from_model = out["K_label"].clone()
    l1, l2, l3 = ProposalLoss(cfg)(out), RefinementLoss(cfg)(out), seg_loss(out)
    assert isinstance(l3["keypoint_seg_loss"].grad_fn, torch.autograd.function.BackwardCFunction), "the fused loss did not run"
    assert torch.equal(out["K_label"], label_from_model)
    n_fg = int((out["K_label"] == 1).sum())
    print("keypoint labels of the train step (0 / 1 / 255):", int((out["K_label"] == 0).sum()), n_fg, int((out["K_label"] == 255).sum()))
    assert n_fg >= 5
    (l1["loss"] + l2["loss"] + l3["loss"]).backward(retain_graph=True)
    params = dict(model.keypoint_weighting.named_parameters())
    for name, p in params.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.ne(0).any()), name
    # the segmentation loss alone on the same graph: fused, and the torch statement
    fused = torch.autograd.grad(seg_loss(out)["loss"], list(params.values()), retain_graph=True)
    seg_loss._fused = lambda it: None
    stated_loss = seg_loss(out)
    assert not isinstance(stated_loss["keypoint_seg_loss"].grad_fn, torch.autograd.function.BackwardCFunction)
    stated = torch.autograd.grad(stated_loss["loss"], list(params.values()), retain_graph=True)
    # float64: the head and the loss evaluated in double on the features the head saw
    assert len(seen) == 1 and seen[0].shape == (B, cfg.NUM_KEYPOINTS, 512)
    feats = seen[0].transpose(1, 2).double()
    head64 = KeypointWeighting(cfg, feats.shape[1]).cuda().double()
    head64.load_state_dict(model.keypoint_weighting.state_dict())
    _, logits64 = head64.forward_torch(feats)
    item64 = dict(K_cls=logits64, keypoints=out["keypoints"], boxes=out["boxes"], class_idx=out["class_idx"])
    yard = torch.autograd.grad(seg_loss.forward_torch(item64)["loss"], list(head64.parameters()))
    for (name, _), gf, gs, g64 in zip(params.items(), fused, stated, yard):
        assert_fp32_class(gf.cpu().numpy().reshape(-1), gs.cpu().numpy().reshape(-1), f"gradient of the segmentation loss on {name}",
                          ref64=g64.cpu().numpy().reshape(-1), own_factor=2.0)

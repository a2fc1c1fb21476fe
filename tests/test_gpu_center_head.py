"""GPU: the centre heatmap head (cfg.CENTERHEAD) -- csrc/center_head.hip and the torch statements run on the device against the float64
restatement tests/center_head_ref.py, on the seeded cases of tests/center_head_cases.py (their margins are asserted on the CPU by
tests/test_host_center_head.py).  The bars and their derivation: tests/center_head_checks.py.

Largest errors observed on an MI355X are recorded in DESIGN.md section 7."""
import functools

import numpy as np
import pytest
import torch

import center_head_cases as K
import center_head_checks as C
from gpu_util import dev

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def train_case(H, W):
    return K.train_case(H, W)


@functools.lru_cache(maxsize=None)
def decode_case(name):
    return K.decode_case(name)


def make_cfg(H, W, n_cls=2, topk=100):
    """A config whose centre-head map is (H, W) with the geometry of center_head_cases.geometry."""
    from vision3d_amd.core.config import _defaults
    from vision3d_amd.detector.center_head import center_geometry
    cfg = _defaults()
    cfg.NUM_CLASSES = n_cls
    cfg.PROPOSAL.TOPK = topk
    cfg.CENTERHEAD.ENABLED = True
    px, py, x_lo, y_lo = K.geometry(H, W)
    cfg.GRID_BOUNDS = [x_lo, y_lo, -3, px * (W + 0.5), -y_lo, 1]
    geom, shape = center_geometry(cfg)
    assert shape == (H, W) and geom == K.geometry(H, W)
    return cfg


def native_targets(case):
    from vision3d_amd.core.center_targets import center_targets
    boxes = [dev(b) for b in case["boxes"]]
    classes = [dev(c) for c in case["class_idx"]]
    return center_targets(boxes, classes, case["n_cls"], case["H"], case["W"], case["geom"])


def to_np(ts):
    return tuple(t.cpu().numpy() for t in ts)


# ---- targets

@pytest.mark.parametrize("shape", K.TRAIN_SHAPES)
def test_targets_match_the_restatement(shape):
    case = train_case(*shape)
    C.check_targets(to_np(native_targets(case)), case["tgt"], f"native {shape}")


@pytest.mark.parametrize("shape", K.TRAIN_SHAPES)
def test_targets_torch_statement_on_the_device(shape):
    from vision3d_amd.core.center_targets import CenterTargetAssigner
    case = train_case(*shape)
    assigner = CenterTargetAssigner(make_cfg(*shape))
    got = assigner.forward_torch([dev(b) for b in case["boxes"]], [dev(c) for c in case["class_idx"]])
    C.check_targets(to_np(got), case["tgt"], f"torch on device {shape}")


def test_assigner_takes_the_native_call_and_repeats_bit_for_bit():
    from vision3d_amd.core import center_targets as T
    shape = K.TRAIN_SHAPES[1]
    case = train_case(*shape)
    assigner = T.CenterTargetAssigner(make_cfg(*shape))
    item = assigner(dict(boxes=[dev(b) for b in case["boxes"]], class_idx=[dev(c) for c in case["class_idx"]]))
    first = tuple(item[k] for k in ("G_heat", "G_ind", "G_mask", "G_cls", "G_creg"))
    C.check_targets(to_np(first), case["tgt"], "assigner")
    assert first[0].dtype == torch.float32 and first[1].dtype == torch.int32 and first[2].dtype == torch.uint8
    again = native_targets(case)
    for a, b in zip(first, again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # all frames empty: exact zeros, nothing masked
    heat, ind, mask, cls, reg = T.center_targets([torch.zeros((0, 7), device="cuda")] * 2, [torch.zeros(0, dtype=torch.int32, device="cuda")] * 2,
                                                 2, 20, 24, K.geometry(20, 24))
    assert not heat.any() and not mask.any() and (ind == -1).all() and not reg.any()


# ---- loss

def fused_loss(case, upstream=(1.0, 1.0)):
    from vision3d_amd.detector.center_head import center_loss_fused
    tgt = case["tgt"]
    maps = dev(case["maps"]).requires_grad_()
    hm, rl = center_loss_fused(maps, dev(tgt["heat"], torch.float32), dev(tgt["ind"]), dev(tgt["mask"]), dev(tgt["reg"], torch.float32),
                               case["n_cls"])
    (upstream[0] * hm + upstream[1] * rl).backward()
    return hm.detach(), rl.detach(), maps.grad


def split(grad, n_cls):
    g = grad.cpu().numpy()
    d_hm, d_reg = g.copy(), g.copy()
    d_hm[:, n_cls:] = 0
    d_reg[:, :n_cls] = 0
    return d_hm, d_reg


@pytest.mark.parametrize("shape", K.TRAIN_SHAPES)
def test_loss_and_gradient_match_the_restatement(shape):
    case = train_case(*shape)
    hm, rl, grad = fused_loss(case)
    C.check_loss(hm.item(), rl.item(), *split(grad, case["n_cls"]), case["loss"], case["n_cls"], f"native {shape}")
    hm2, rl2, grad2 = fused_loss(case)
    assert torch.equal(hm, hm2) and torch.equal(rl, rl2) and torch.equal(grad.view(torch.int32), grad2.view(torch.int32))
    # an upstream scale of 0.5 on both terms: half the gradient, exactly
    _, _, half = fused_loss(case, (0.5, 0.5))
    assert torch.equal(half, 0.5 * grad)


def test_upstream_gradients_scale_the_two_channel_groups_exactly():
    """Backward under upstream gradients (2, 3) is the stored gradient -- what a backward under (1, 1) returns -- times 2 on the heat
    channels and 3 on the box channels, one exact fp32 multiply per element.  The first two frames of the 33 x 47 case: an odd number of
    cells (1 551), so the boundary between the channel groups falls inside a wave in both frames."""
    case = train_case(33, 47)
    n_cls = case["n_cls"]
    two = dict(case, maps=case["maps"][:2], tgt={k: case["tgt"][k][:2] for k in ("heat", "ind", "mask", "reg")})
    assert int(two["tgt"]["mask"].sum()) > 0
    _, _, stored = fused_loss(two)
    _, _, grad = fused_loss(two, (2.0, 3.0))
    want = stored.clone()
    assert float(want[:, :n_cls].abs().max()) > 0 and float(want[:, n_cls:].abs().max()) > 0
    want[:, :n_cls] *= 2.0
    want[:, n_cls:] *= 3.0
    assert torch.equal(grad, want)


@pytest.mark.parametrize("shape", K.TRAIN_SHAPES)
def test_center_loss_module_fused_and_torch_paths(shape, monkeypatch):
    """CenterLoss on an item as Second.forward leaves it (fused maps + the views made from them): the native pass; the same item without
    `_head_maps`: the torch expression on the device.  Both against float64; backward through 0.5 * loss is half the gradient."""
    from vision3d_amd.detector import center_head as M
    from vision3d_amd.detector.center_head import CenterLoss
    case = train_case(*shape)
    n_cls, tgt = case["n_cls"], case["tgt"]
    cfg = make_cfg(*shape)
    cfg.TRAIN.LAMBDA = 2.0
    loss = CenterLoss(cfg)
    ref = case["loss"]
    want = ref["d_hm"] + 2.0 * ref["d_reg"]
    targets = dict(G_heat=dev(tgt["heat"], torch.float32), G_ind=dev(tgt["ind"]), G_mask=dev(tgt["mask"]), G_creg=dev(tgt["reg"], torch.float32))
    calls, grads, orig = [], {}, M.center_loss_fused
    monkeypatch.setattr(M, "center_loss_fused", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    for path in ("fused", "torch"):
        for scale in (1.0, 0.5):
            maps = dev(case["maps"]).requires_grad_()
            p_cls, p_reg = maps[:, :n_cls], maps[:, n_cls:]
            item = dict(P_cls=p_cls, P_reg=p_reg, **targets)
            if path == "fused":
                item["_head_maps"] = (maps, p_cls, p_reg)
            n_before = len(calls)
            out = loss(item)
            assert (len(calls) > n_before) == (path == "fused")
            (scale * out["loss"]).backward()
            grads[path, scale] = maps.grad
            if scale == 1.0:
                C.check_loss(out["cls_loss"].item(), out["reg_loss"].item(), *split(maps.grad, n_cls),
                             dict(ref, d_reg=2.0 * ref["d_reg"]), n_cls, f"CenterLoss {path} {shape}")
                assert abs(out["loss"].item() - (ref["hm"] + 2.0 * ref["reg"])) <= 1e-5 * (ref["hm"] + 2.0 * ref["reg"])
                assert np.abs(maps.grad.cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()
    assert torch.equal(grads["fused", 0.5], 0.5 * grads["fused", 1.0])
    # P_cls replaced after the forward: the fused maps no longer speak for the item
    maps = dev(case["maps"]).requires_grad_()
    item = dict(P_cls=maps[:, :n_cls] * 1.0, P_reg=maps[:, n_cls:], _head_maps=(maps, maps[:, :n_cls], maps[:, n_cls:]), **targets)
    assert loss._fused(item) is None


# ---- decode

@pytest.mark.parametrize("name", K.DECODE_CASES)
def test_decode_matches_the_restatement_and_the_torch_statement(name):
    from vision3d_amd.detector.center_head import CenterHead, center_decode
    case = decode_case(name)
    maps = dev(case["maps"])
    boxes, scores = center_decode(maps, case["n_cls"], case["geom"], case["topk"])
    C.check_decode(boxes.cpu().numpy(), scores.cpu().numpy(), case, f"native {name}")
    b2, s2 = center_decode(maps, case["n_cls"], case["geom"], case["topk"])
    assert torch.equal(boxes.view(torch.int32), b2.view(torch.int32)) and torch.equal(scores.view(torch.int32), s2.view(torch.int32))
    head = CenterHead(make_cfg(case["H"], case["W"], case["n_cls"], case["topk"]))
    tb, ts = head.decode_torch(maps)
    tb, ts = tb.cpu().numpy(), ts.cpu().numpy()
    C.check_decode(tb, ts, case, f"torch on device {name}")
    # native against the torch statement, to the same bars
    C.check_decode(boxes.cpu().numpy(), scores.cpu().numpy(), case, f"native vs torch {name}",
                   ref=dict(boxes=tb.astype(np.float64), scores=ts.astype(np.float64), cells=C.cells_of(tb, ts, case)))
    if name == "tie":
        cells = case["ref"]["cells"]
        assert cells[1, 0, :2].tolist() == [28, 29] and cells[2, 1, :2].tolist() == [54, 63]


def test_decode_and_tail_replayed_from_a_graph_equal_eager():
    from vision3d_amd.detector.center_head import CenterHead
    case = decode_case("train_33x47")
    head = CenterHead(make_cfg(case["H"], case["W"], case["n_cls"], case["topk"])).cuda()
    maps = dev(case["maps"])
    other = dev(decode_case("train_33x47")["maps"][[2, 0, 1]].copy())
    want = head.proposals_padded(other)  # (also the warm-up outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = head.proposals_padded(maps)
    maps.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, want):
        assert torch.equal(a, b)
    got = head.finalize(*out)
    assert len(got[0]) > 0 and (got[3] > 0.3).all()


# ---- model

def small_model():
    from vision3d_amd.core.config import _defaults
    from vision3d_amd.detector import Second
    cfg = _defaults()
    cfg.NUM_CLASSES = 2
    cfg.CENTERHEAD.ENABLED = True
    cfg.GRID_BOUNDS = [0, -8.0, -3, 12.8, 8.0, 1]  # a 40 x 32 map
    for a in cfg.ANCHORS:
        a["score_thresh"] = 0.05  # (the prior bias puts fresh scores near 0.1)
    torch.manual_seed(0)
    model = Second(cfg).cuda()
    with torch.no_grad():
        model.head.conv_cls.weight.mul_(20.0)  # logits with some spread: distinct peaks
    return cfg, model


def test_second_with_the_centre_head_inference_and_one_training_step():
    from vision3d_amd import synth
    from vision3d_amd.core import Preprocessor
    from vision3d_amd.core.center_targets import CenterTargetAssigner
    from vision3d_amd.detector.center_head import CenterHead, CenterLoss
    cfg, model = small_model()
    assert isinstance(model.head, CenterHead) and model.head.map_shape == (40, 32)
    clouds = [synth.make_cloud(s, n_points=20000) for s in (0, 1)]
    model.eval()
    with torch.no_grad():
        item = Preprocessor(cfg)(dict(points=clouds))
        boxes, bidx, cidx, scores = model.inference(item)
        out = model(item)
        assert out["P_cls"].shape == (2, 2, 40, 32) and out["P_reg"].shape == (2, 8, 40, 32)
        maps = torch.cat((out["P_cls"], out["P_reg"]), 1).contiguous()
        want = model.head.finalize(*model.head.proposals_padded(maps))
    assert len(boxes) > 0 and boxes.shape[1] == 7
    for a, b in zip((boxes, bidx, cidx, scores), want):
        assert torch.equal(a, b)
    # ---- one training step
    model.train()
    item = Preprocessor(cfg)(dict(points=clouds))
    gt = [torch.tensor([[4.2, -2.1, -1.0, 1.6, 3.9, 1.5, 0.3], [9.3, 3.3, -0.8, 0.6, 0.8, 1.7, 1.2]], device="cuda"),
          torch.tensor([[6.1, 0.7, -1.0, 1.7, 4.1, 1.6, -2.0]], device="cuda")]
    item.update(boxes=gt, class_idx=[torch.tensor([0, 1], device="cuda"), torch.tensor([0], device="cuda")])
    item = CenterTargetAssigner(cfg)(model(item))
    assert int(item["G_mask"].sum()) == 3 and item["G_heat"].shape == item["P_cls"].shape
    losses = CenterLoss(cfg)(item)
    losses["loss"].backward()
    for p in (model.head.conv_cls.weight, model.head.conv_reg.weight, model.rpn.down_block[1].weight):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0
    assert torch.isfinite(losses["loss"]) and losses["cls_loss"] > 0 and losses["reg_loss"] > 0

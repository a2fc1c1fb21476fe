"""CPU: the centre heatmap head (cfg.CENTERHEAD) -- the float64 restatement on hand cases, the margins of the cases the GPU tests
compare and the rejection rate of their generator, the torch statements on host tensors against the restatement, the config key
(disabled: today's SECOND), the refusals, and the C entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import center_head_cases as K
import center_head_checks as C
import center_head_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_cfg(H, W, n_cls=2, topk=100):
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


@pytest.fixture(scope="module", params=K.TRAIN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def case(request):
    return K.train_case(*request.param)


# ---- the restatement on hand cases

def test_radius_roots_by_hand():
    # a = b = 10 cells, o = 0.1: s = 20; r1 = (20 + sqrt(400 - 400 * 0.9 / 1.1)) / 2, r2 = (40 + sqrt(1600 - 1440)) / 2, r3 = (-4 + sqrt(16 + 144)) / 2
    r1, r2, r3 = R.radius_roots(4.0, 4.0, 0.4, 0.4, 0.1)
    assert r1 == pytest.approx((20 + (400 - 400 * 0.9 / 1.1) ** 0.5) / 2, abs=1e-12)
    assert r2 == pytest.approx(20 + 160 ** 0.5 / 2, abs=1e-12) and r3 == pytest.approx(-2 + 160 ** 0.5 / 2, abs=1e-12)


def test_one_object_by_hand():
    geom = (0.4, 0.4, 0.0, -4.0)
    box = np.asarray([[2.1, -1.9, -1.0, 4.0, 4.0, 1.5, 0.5]], np.float32)  # fx = 5.25, fy = 5.25; radius int(4.32) = 4, sigma = 1.5
    t = R.targets([box], [np.asarray([1])], 2, 20, 24, geom)
    assert t["ind"][0, 0] == 5 * 24 + 5 and t["mask"][0, 0] == 1 and t["cls"][0, 0] == 1 and t["mask"].sum() == 1
    assert t["heat"][0, 1, 5, 5] == 1.0 and not t["heat"][0, 0].any()
    assert t["heat"][0, 1, 5, 9] == pytest.approx(np.exp(-16 / 4.5), abs=1e-15) and t["heat"][0, 1, 5, 10] == 0
    assert t["heat"][0, 1, 1, 1] == pytest.approx(np.exp(-32 / 4.5), abs=1e-15) and t["heat"][0, 1, 0, 5] == 0
    np.testing.assert_allclose(t["reg"][0, 0], [0.25, 0.25, -1.0, np.log(4.0), np.log(4.0), np.log(1.5), np.sin(0.5), np.cos(0.5)], atol=2e-6)
    assert t["window"][0, 1].sum() == 81
    # not live: outside, unknown class, flat
    for bad, c in (([-0.1, 0, 0, 1, 1, 1, 0], 0), ([2, 0, 0, 1, 1, 1, 0], 2), ([2, 0, 0, 1, 0, 1, 0], 0), ([2, 0, 0, np.inf, 1, 1, 0], 0)):
        t = R.targets([np.asarray([bad], np.float32)], [np.asarray([c])], 2, 20, 24, geom)
        assert t["mask"].sum() == 0 and (t["ind"] == -1).all() and not t["heat"].any() and not t["reg"].any()


def test_loss_gradient_is_the_derivative_of_the_restated_loss(case):
    """Central differences of the float64 loss on a handful of entries (heat cells of both kinds, an object cell's box channels)."""
    tgt, ref, n_cls = case["tgt"], case["loss"], case["n_cls"]
    maps = case["maps"].astype(np.float64)
    f = lambda m: R.loss(m, tgt["heat"], tgt["ind"], tgt["mask"], tgt["reg"], n_cls, lam=1.0)["loss"]
    b, i = np.argwhere(tgt["mask"] > 0)[0]
    cell = np.unravel_index(tgt["ind"][b, i], maps.shape[2:])
    spots = [(b, tgt["cls"][b, i]) + cell, (b, n_cls + 3) + cell, (b, n_cls + 6) + cell, (0, 0, 1, 2), (2, 1, 7, 9)]
    for s in spots:
        hi, lo = maps.copy(), maps.copy()
        hi[s] += 1e-5
        lo[s] -= 1e-5
        # (the loss is a sum of a few hundred: its float64 rounding, 1e-13, over the step leaves 1e-8 of noise in the quotient)
        assert (f(hi) - f(lo)) / 2e-5 == pytest.approx(ref["dmaps"][s], rel=1e-5, abs=1e-7)
    assert tgt["heat"][spots[0]] == 1.0


def test_peaks_and_order_by_hand():
    x = np.asarray([[1.0, 1.0, 0.0], [0.0, 0.5, 0.0], [3.0, 0.0, 2.0]])
    np.testing.assert_array_equal(R.peaks(x), [[1, 1, 0], [0, 0, 0], [1, 0, 1]])
    maps = np.zeros((1, 9, 3, 3))
    maps[0, 0] = x
    maps[0, 1] = [0.3, -0.2, 0.0], [0, 0, 0], [0.5, 0, 0]  # dx
    d = R.decode(maps, 1, (0.4, 0.4, 0.0, -0.6), 5)
    np.testing.assert_array_equal(d["cells"][0, 0], [6, 8, 0, 1, -1])
    np.testing.assert_allclose(d["boxes"][0, 0], [0.5 * 0.4, 2 * 0.4 - 0.6, 0, 1, 1, 1, np.pi / 2][:6] + [0.0])  # atan2(0, 0) = 0
    assert d["scores"][0, 4] == 0 and not d["boxes"][0, 4].any()


# ---- the compared cases

def test_compared_cases_keep_their_margins_and_cover_the_branches(case):
    tgt, ref = case["tgt"], case["loss"]
    H, W = case["H"], case["W"]
    assert tgt["fmargin"] >= 1e-3 and tgt["rmargin"] >= 1e-6 and ref["reg_margin"] >= 1e-3
    logits = case["maps"][:, :case["n_cls"]]
    assert len(np.unique(logits)) == logits.size
    n = [len(b) for b in case["boxes"]]
    assert n[1] == 0 and tgt["mask"][1].sum() == 0 and not tgt["heat"][1].any()  # the empty frame
    assert tgt["mask"][0].sum() == n[0] - 3  # outside the grid, class n_cls, w = 0
    iy, ix = np.divmod(tgt["ind"][0][tgt["mask"][0] > 0], W)
    assert (ix == 0).any() and (ix == W - 1).any() and (iy == 0).any() and (iy == H - 1).any()  # windows clipped at the four borders
    for b in (0, 2):  # two objects in one cell
        live = tgt["ind"][b][tgt["mask"][b] > 0]
        assert len(np.unique(live)) == len(live) - 1
    # overlapping windows of one class: a cell whose value is the larger of two splats
    a, c = case["boxes"][0][5:6], case["boxes"][0][6:7]
    one, two = (R.targets([bx], [np.asarray([1])], 2, H, W, case["geom"]) for bx in (a, c))
    both = one["window"][0, 1] & two["window"][0, 1]
    assert both.sum() >= 10 and (tgt["heat"][0, 1][both] >= np.maximum(one["heat"][0, 1], two["heat"][0, 1])[both]).all()
    assert (one["heat"][0, 1][both] > two["heat"][0, 1][both]).any() and (one["heat"][0, 1][both] < two["heat"][0, 1][both]).any()
    radii = {int(max(2, min(R.radius_roots(w, l, K.PX, K.PY, 0.1)))) for bx in case["boxes"] for w, l in bx[:, 3:5] if w > 0}
    assert 2 in radii and max(radii) >= 5  # the minimum radius and a window of 11 x 11 cells or more


def test_generator_rejects_at_most_two_percent_of_its_draws():
    drawn = rejected = 0
    for H, W in K.TRAIN_SHAPES:
        for seed in range(100):
            boxes, class_idx = K.draw_targets(H, W, seed)
            tgt = R.targets(boxes, class_idx, 2, H, W, K.geometry(H, W))
            ok, _ = K.margins_ok(tgt, K.draw_maps(H, W, seed, 2, len(boxes), tgt), 2)
            drawn, rejected = drawn + 1, rejected + (not ok)
    print(f"[center cases] {rejected} of {drawn} draws rejected")
    assert rejected <= 0.02 * drawn


@pytest.mark.parametrize("name", K.DECODE_CASES)
def test_decode_cases_cover_their_branches(name):
    d = K.decode_case(name)
    cells = d["ref"]["cells"]
    pads = (cells < 0).sum(-1)
    if name in ("pads", "tie", "train_20x24"):
        assert (pads > 0).all() and (pads < d["topk"]).all()
    else:
        assert not pads.any()  # more peaks than TOPK: the selection truncates
    if name == "tie":
        assert cells[1, 0, :2].tolist() == [28, 29] and cells[2, 1, :2].tolist() == [54, 63]
    if name == "slices":
        assert d["H"] * d["W"] > 8 * 4096 and len(np.unique(cells[0, 0] // 4096)) >= 5  # winners from most slices of the selection


# ---- the torch statements on host tensors

def test_torch_targets_on_host_tensors(case):
    from vision3d_amd.core.center_targets import CenterTargetAssigner
    assigner = CenterTargetAssigner(make_cfg(case["H"], case["W"]))
    item = assigner(dict(boxes=[torch.from_numpy(b) for b in case["boxes"]], class_idx=[torch.from_numpy(c) for c in case["class_idx"]]))
    got = tuple(item[k].numpy() for k in ("G_heat", "G_ind", "G_mask", "G_cls", "G_creg"))
    C.check_targets(got, case["tgt"], "torch on host")
    assert got[1].dtype == np.int32 and got[2].dtype == np.uint8 and got[3].dtype == np.int32 and got[4].shape == (3, 128, 8)


def test_torch_targets_beyond_128_objects():
    from vision3d_amd.core.center_targets import CenterTargetAssigner
    rng = np.random.default_rng(3)
    g = K.geometry(20, 24)
    boxes = np.asarray([K._box(rng, g, int(rng.integers(0, 24)), int(rng.integers(0, 20))) for _ in range(130)], np.float32)
    item = CenterTargetAssigner(make_cfg(20, 24))(dict(boxes=[torch.from_numpy(boxes)], class_idx=[torch.zeros(130, dtype=torch.long)]))
    assert item["G_mask"].shape == (1, 130) and int(item["G_mask"].sum()) == 130 and int((item["G_heat"][0, 0] == 1).sum()) >= 100
    assert item["G_creg"].shape == (1, 130, 8) and not item["G_heat"][0, 1].any()


def test_torch_loss_on_host_tensors(case):
    from vision3d_amd.detector.center_head import CenterLoss
    tgt, n_cls = case["tgt"], case["n_cls"]
    loss = CenterLoss(make_cfg(case["H"], case["W"]))
    grads = []
    for k in ("cls_loss", "reg_loss"):
        maps = torch.from_numpy(case["maps"]).requires_grad_()
        item = dict(P_cls=maps[:, :n_cls], P_reg=maps[:, n_cls:], G_heat=torch.from_numpy(tgt["heat"]).float(), G_ind=torch.from_numpy(tgt["ind"]),
                    G_mask=torch.from_numpy(tgt["mask"]), G_creg=torch.from_numpy(tgt["reg"]).float())
        out = loss(item)
        out[k].backward()
        grads.append(maps.grad.numpy())
    C.check_loss(out["cls_loss"].item(), out["reg_loss"].item(), grads[0], grads[1], case["loss"], n_cls, "torch on host")
    assert out["loss"].item() == pytest.approx(case["loss"]["loss"], rel=1e-5)


@pytest.mark.parametrize("name", K.DECODE_CASES)
def test_torch_decode_on_host_tensors(name):
    from vision3d_amd.detector.center_head import CenterHead
    d = K.decode_case(name)
    head = CenterHead(make_cfg(d["H"], d["W"], d["n_cls"], d["topk"]))
    boxes, scores = head.decode(torch.from_numpy(d["maps"]))  # host tensors: the torch statements
    C.check_decode(boxes.numpy(), scores.numpy(), d, f"torch on host {name}")


# ---- config, model surface, refusals

def test_config_key_and_disabled_model_is_todays_second():
    from vision3d_amd.core.config import _defaults, second_car_cfg
    from vision3d_amd.detector import Second
    from vision3d_amd.detector.proposal import ProposalLayer
    want = dict(ENABLED=False, MIN_OVERLAP=0.1, MIN_RADIUS=2, FOCAL_ALPHA=2.0, FOCAL_BETA=4.0, CODE_WEIGHTS=[1.0] * 8, NMS_IOU=0.01)
    assert dict(_defaults().CENTERHEAD) == want and dict(second_car_cfg().CENTERHEAD) == want
    old = second_car_cfg()
    del old["CENTERHEAD"]  # a config written before the key existed
    shapes = []
    for cfg in (second_car_cfg(), old):
        torch.manual_seed(0)
        model = Second(cfg)
        assert type(model.head) is ProposalLayer
        shapes.append({k: tuple(v.shape) for k, v in model.state_dict().items()})
    assert shapes[0] == shapes[1]
    assert [k for k in shapes[0] if k.startswith("head.")] == ["head.conv_cls.weight", "head.conv_cls.bias", "head.conv_reg.weight", "head.conv_reg.bias"]
    assert shapes[0]["head.conv_cls.weight"] == (2, 128, 1, 1) and shapes[0]["head.conv_reg.weight"] == (14, 128, 1, 1)


def test_enabled_head_parameters_and_map_views():
    from vision3d_amd.core.config import _defaults
    from vision3d_amd.detector import CenterHead, Second
    cfg = _defaults()
    cfg.CENTERHEAD.ENABLED = True
    torch.manual_seed(0)
    model = Second(cfg)
    head = model.head
    assert isinstance(head, CenterHead) and head.map_shape == (200, 176) and head.geom == (0.4, 0.4, 0.0, -40.0)
    sd = {k: tuple(v.shape) for k, v in model.state_dict().items() if k.startswith("head.")}
    assert sd == {"head.conv_cls.weight": (3, 128, 1, 1), "head.conv_cls.bias": (3,), "head.conv_reg.weight": (8, 128, 1, 1),
                  "head.conv_reg.bias": (8,)}
    assert torch.allclose(head.conv_cls.bias, torch.full((3,), -float(np.log(9.0)))) and not head.conv_reg.bias.any()
    assert 0.005 < float(head.conv_reg.weight.detach().std()) < 0.015 and 0.005 < float(head.conv_cls.weight.detach().std()) < 0.02
    maps = torch.arange(2 * 11 * 4 * 5, dtype=torch.float32).reshape(2, 11, 4, 5)
    heat, reg = head.maps_from_fused(maps)
    assert heat.shape == (2, 3, 4, 5) and reg.shape == (2, 8, 4, 5) and heat.data_ptr() == maps.data_ptr() and torch.equal(reg, maps[:, 3:])
    model.eval()
    with torch.no_grad():
        p_cls, p_reg = head(torch.randn(1, 128, 6, 7))  # host tensors: the torch convolutions
    assert p_cls.shape == (1, 3, 6, 7) and p_reg.shape == (1, 8, 6, 7)


def test_entry_points_that_do_not_take_the_head_yet_refuse_it():
    from vision3d_amd.core.config import _defaults
    from vision3d_amd.detector import PV_RCNN, Second
    from vision3d_amd.detector.graph import GraphedSecond
    cfg = _defaults()
    cfg.CENTERHEAD.ENABLED = True
    with pytest.raises(ValueError, match="CENTERHEAD"):
        PV_RCNN(cfg)
    model = Second(cfg)
    for call in (lambda: model.graphed_inference(None, [100]), lambda: model.pipelined_inference(None, [100]),
                 lambda: GraphedSecond(model, None, [100])):
        with pytest.raises(ValueError, match="CENTERHEAD"):
            call()
    for key in ("PKW", "VOXELPOOL"):
        both = _defaults()
        both.CENTERHEAD.ENABLED = True
        both[key].ENABLED = True
        with pytest.raises(ValueError, match="CENTERHEAD"):
            Second(both)
    with pytest.raises(ValueError, match="CODE_WEIGHTS"):
        bad = _defaults()
        bad.CENTERHEAD.ENABLED, bad.CENTERHEAD.CODE_WEIGHTS = True, [1.0] * 7
        Second(bad)


# ---- the C entry points

def test_entry_points_declared_bound_and_exported():
    from vision3d_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vision3d_hip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(L.LIB_PATH)
    for name in ("v3d_center_targets", "v3d_center_loss_workspace", "v3d_center_loss_fwd_bwd", "v3d_center_loss_scale",
                 "v3d_center_decode_workspace", "v3d_center_decode"):
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/vision3d_hip.h"
        assert name in L.exported_symbols()
        assert hasattr(handle, name)
    lib = L.lib()
    assert lib.v3d_center_loss_workspace() >= (512 + 64) * 8
    assert lib.v3d_center_decode_workspace(1, 3, 200, 176) >= 3 * 9 * 1024 * 8
    # sizes are host data: every call refuses beyond its limits before it touches a pointer or the device
    off = (ctypes.c_int32 * 2)(0, 0)
    big = (ctypes.c_int32 * 2)(0, 129)
    geom = (ctypes.c_double * 4)(0.4, 0.4, 0.0, -40.0)
    targets = lambda off, B, n_cls: lib.v3d_center_targets(0, 0, off, B, n_cls, 200, 176, geom, 0.1, 2, 0, 0, 0, 0, 0, 0)
    assert targets(big, 1, 3) == -3 and targets(off, 65, 3) == -3 and targets(off, 1, 9) == -3
    assert targets(off, 1, 3) == -1 and targets(off, 1, 0) == -1  # within the limits: null outputs are invalid arguments
    loss = lambda B, n_cls: lib.v3d_center_loss_fwd_bwd(0, 0, 0, 0, 0, B, n_cls, 200, 176, 2.0, 4.0, 0, 0, 0, 0, 0, 0)
    assert loss(65, 3) == -3 and loss(1, 9) == -3 and loss(1, 3) == -1
    assert lib.v3d_center_loss_scale(0, 65, 3, 200, 176, 0, 0, 0) == -3 and lib.v3d_center_loss_scale(0, 1, 3, 200, 176, 0, 0, 0) == -1
    decode = lambda B, n_cls, topk: lib.v3d_center_decode(0, B, n_cls, 200, 176, geom, topk, 0, 0, 0, 0, 0)
    assert decode(65, 3, 100) == -3 and decode(1, 9, 100) == -3 and decode(1, 3, 1025) == -3 and decode(1, 3, 100) == -1
    assert lib.v3d_center_decode(0, 1, 3, 4097, 4096, geom, 100, 0, 0, 0, 0, 0) == -3

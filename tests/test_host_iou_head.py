"""CPU only: the IoU-aware confidence head of the anchor head (cfg.IOU_HEAD).  Config and refusals, the head's state_dict keys and
the order of the fused convolutions, the torch statement of the loss against the float64 restatement (tests/iou_head_ref.py), the
per-anchor expressions of csrc/iou_head_device.h compiled by g++ against it, the score rule on hand cases -- and every ordered case of
tests/test_gpu_iou_head.py decided by margin ON THE REFERENCE ALONE: within a group distinct rectified scores differ by at least 1e-5
relative (equal ones come from identical logits and fall to position), thresholds keep that distance, every NMS decision of a stage
scene is clear of its threshold.  No case is left out.

Bars of the host build (fp32): the IoU of a pair is right to a few 1e-7 (profiles/iou_loss.txt: 2.0e-7), the BCE adds a few roundings
of numbers of order one; HOST_VALUE = 1e-5, the bar of tests/test_host_iou_loss.py, sits a decade above that and a decade below a wrong
formula."""
import ctypes as C_
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import iou_head_cases as IC
import iou_head_ref as IH
import proposal_cases as C
import proposal_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_VALUE = 1e-5
UPSTREAM = (2.0, 3.0, 5.0, 7.0)


# ------------------------------------------------------------------------------------------------------------------------ config
def test_config_defaults_and_an_old_config_is_disabled():
    from vision3d_amd.core.config import _defaults, cfg, iou_head_config, second_car_cfg
    for c in (cfg, _defaults(), second_car_cfg()):
        assert dict(c.IOU_HEAD) == dict(ENABLED=False, LOSS_WEIGHT=1.0, POWER=4)
        assert iou_head_config(c) == dict(ENABLED=False, LOSS_WEIGHT=1.0, POWER=4)
    old = _defaults()
    del old["IOU_HEAD"]  # a config written before the key existed
    assert iou_head_config(old) == dict(ENABLED=False, LOSS_WEIGHT=1.0, POWER=4)
    from vision3d_amd.detector.proposal import ProposalLayer, ProposalLoss
    assert sorted(ProposalLayer(old).state_dict()) == ["conv_cls.bias", "conv_cls.weight", "conv_reg.bias", "conv_reg.weight"]
    assert not ProposalLoss(old).iou_head["ENABLED"]
    part = _defaults()
    part.IOU_HEAD = dict(ENABLED=True)  # keys left out take their defaults
    assert iou_head_config(part) == dict(ENABLED=True, LOSS_WEIGHT=1.0, POWER=4)


def test_state_dict_keys_seed_and_the_fused_convolutions():
    from vision3d_amd.detector.proposal import ProposalLayer, fused_convs
    base = ["conv_cls.bias", "conv_cls.weight", "conv_reg.bias", "conv_reg.weight"]
    for n_cls in (1, 3):
        for with_dir in (False, True):
            off = ProposalLayer(IC.make_cfg(n_cls, enabled=False, with_dir=with_dir))
            on = ProposalLayer(IC.make_cfg(n_cls, with_dir=with_dir))
            assert sorted(off.state_dict()) == sorted(base + (["conv_dir.bias", "conv_dir.weight"] if with_dir else []))
            assert sorted(set(on.state_dict()) - set(off.state_dict())) == ["conv_iou.bias", "conv_iou.weight"]
            assert fused_convs(off) == [off.conv_cls, off.conv_reg] + ([off.conv_dir] if with_dir else [])
            assert fused_convs(on) == [on.conv_cls, on.conv_reg] + ([on.conv_dir] if with_dir else []) + [on.conv_iou]
            assert on.conv_iou.out_channels == n_cls * 2 and on.conv_iou.kernel_size == (1, 1)
            assert float(on.conv_iou.bias.detach().abs().max()) == 0.0 and 0.005 < float(on.conv_iou.weight.detach().std()) < 0.02
            assert sum(c.out_channels for c in fused_convs(on)) == n_cls * 2 * (9 + with_dir)
    # conv_iou draws behind every other head: the same seed gives the same cls / reg / dir values
    for with_dir in (False, True):
        torch.manual_seed(3)
        a = ProposalLayer(IC.make_cfg(1, enabled=False, with_dir=with_dir)).state_dict()
        torch.manual_seed(3)
        b = ProposalLayer(IC.make_cfg(1, with_dir=with_dir)).state_dict()
        assert all(torch.equal(a[k], b[k]) for k in a)


def test_fused_layout_round_trip():
    """fuse / maps_from_fused / dir_from_fused / iou_from_fused agree on [cls | reg | (dir) | iou] and on the IoU channel formula"""
    from vision3d_amd.detector.proposal import ProposalLayer
    for n_cls in (1, 3):
        for with_dir in (False, True):
            head = ProposalLayer(IC.make_cfg(n_cls, with_dir=with_dir)).train()
            out = head(torch.randn(2, 128, 3, 4))
            assert len(out) == 3 + with_dir
            maps = head.fuse(*out)
            na = n_cls * 2
            assert maps.shape == (2, na * (9 + with_dir), 3, 4)
            assert torch.equal(head.iou_from_fused(maps), out[-1]) and torch.equal(head.maps_from_fused(maps)[1], out[1])
            if with_dir:
                assert torch.equal(head.dir_from_fused(maps), out[2])
            for c in range(n_cls):
                for yaw in range(2):
                    assert torch.equal(maps[:, na * (8 + with_dir) + c * 2 + yaw], out[-1][:, c, yaw])
            _, _, p_dir, p_iou = IH.split_maps(maps.detach().numpy(), n_cls, 2, with_dir)
            np.testing.assert_array_equal(p_iou, out[-1].detach().numpy())


def test_refusals():
    from vision3d_amd.core.config import _defaults
    from vision3d_amd.detector import PV_RCNN, Second
    from vision3d_amd.detector.proposal import ProposalLayer, ProposalLoss
    cfg = _defaults()
    cfg.IOU_HEAD.ENABLED = True
    cfg.CENTERHEAD.ENABLED = True
    with pytest.raises(ValueError, match="cfg.IOU_HEAD.ENABLED: the centre heatmap head"):
        Second(cfg)
    cfg = _defaults()
    cfg.IOU_HEAD.ENABLED = True
    with pytest.raises(ValueError, match="cfg.IOU_HEAD.ENABLED: PV_RCNN"):
        PV_RCNN(cfg)
    cfg = _defaults()
    cfg.IOU_HEAD.ENABLED = True
    cfg.BOX_DOF = 8
    with pytest.raises(ValueError, match="cfg.IOU_HEAD.ENABLED.*BOX_DOF"):
        ProposalLayer(cfg)
    for power in (-1, 9, 2.0, "4", None, True):
        cfg = _defaults()
        cfg.IOU_HEAD.ENABLED = True
        cfg.IOU_HEAD.POWER = power
        for build in (ProposalLayer, ProposalLoss, Second):
            with pytest.raises(ValueError, match="cfg.IOU_HEAD.POWER"):
                build(cfg)
    for power in range(9):
        assert ProposalLayer(IC.make_cfg(1, power=power)).iou_head["POWER"] == power
    off = _defaults()
    off.IOU_HEAD.POWER = 99  # a disabled head does not read its keys
    ProposalLayer(off)


class _FakeMap:
    """what dense_train.why_unsupported reads of its input: a bf16 channels_last CUDA map (a stand-in that carries no device)"""
    is_cuda, dtype, shape = True, torch.bfloat16, (1, 128, 8, 8)

    def dim(self):
        return 4

    def is_contiguous(self, memory_format=None):
        return True


def test_dense_train_refuses_the_wider_heads_by_name():
    from vision3d_amd import dense_train
    from vision3d_amd.detector.proposal import ProposalLayer
    from vision3d_amd.detector.second import RPN
    rpn = RPN().train()
    for n_cls, with_dir, width in ((1, False, 18), (1, True, 20), (3, False, 54), (3, True, 60)):
        why = dense_train.why_unsupported(rpn, ProposalLayer(IC.make_cfg(n_cls, with_dir=with_dir)), _FakeMap())
        assert why is not None and f"width {width}" in why, why


def test_collate_and_second_need_nothing_new():
    """The target needs no new tensor: G_reg, M_reg and the item's anchors are all there."""
    from vision3d_amd.core.preprocess import TrainPreprocessor
    assert TrainPreprocessor.collate_mapping(None, "anchors", [1, 2]) == [1, 2]


# -------------------------------------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("case", IC.LOSS_CASES, ids=C.case_id)
def test_torch_statement_equals_the_reference_in_float64(case):
    c = IC.loss_case(*case)
    ref = IC.loss_reference(case)
    maps, out, target = IC.torch_statement(c, torch.float64)
    assert sorted(out) == sorted(["cls_loss", "reg_loss", "iou_loss", "loss"] + (["dir_loss"] if c["with_dir"] else []))
    np.testing.assert_allclose(target.numpy(), ref["target"], rtol=0, atol=1e-12)
    assert not target.requires_grad and float(target[~torch.from_numpy(c["M_reg"][..., 0])].abs().max()) == 0.0
    keys = ["cls_loss", "reg_loss"] + (["dir_loss"] if c["with_dir"] else []) + ["iou_loss", "loss"]
    for k in keys:
        assert abs(float(out[k].detach()) - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), k
    up = dict(zip(("cls_loss", "reg_loss", "dir_loss", "iou_loss"), UPSTREAM))
    sum(up[k] * out[k] for k in keys[:-1]).backward()
    want = sum(u * g for u, g in zip(UPSTREAM, ref["grads"]))
    gmax = max(float(np.abs(want).max()), 1e-30)
    assert float(np.abs(maps.grad.numpy() - want).max()) <= 1e-12 * gmax
    # no gradient reaches the box channels through the target: the box group is the box term's alone
    na = c["n_cls"] * c["n_yaw"]
    np.testing.assert_allclose(maps.grad.numpy()[:, na:8 * na], UPSTREAM[1] * ref["grads"][1][:, na:8 * na], rtol=0, atol=1e-12 * gmax)
    if c["variant"] == "no_positives":
        assert ref["iou_loss"] == 0.0 and float(out["iou_loss"].detach()) == 0.0
    if c["variant"] == "identical":
        assert np.abs(ref["target"][c["M_reg"][..., 0]] - 1.0).max() < 1e-9
    if c["variant"] == "disjoint":
        assert ref["target"].max() == 0.0
    if c["variant"] == "bad_row":
        pos = c["M_reg"][..., 0]
        assert (ref["target"][pos] == 0).sum() >= pos.sum() // 2 and ref["target"].max() > 0.05 and np.isfinite(want).all()
    if c["variant"] in ("alone", "last"):
        assert int(c["M_reg"].sum()) == 1
    if c["variant"] == "run64":
        flat = c["M_reg"].reshape(-1)
        assert int(flat.sum()) == 64 and flat[64:128].all()
    if c["variant"] == "last":
        assert c["M_reg"].reshape(-1)[-1]


def test_loss_total_and_weights():
    c = IC.loss_case(2, 5, 7, 3, "plain", True)
    ref = IC.loss_reference((2, 5, 7, 3, "plain", True))
    assert abs(ref["loss"] - (ref["cls_loss"] + ref["reg_loss"] + 0.2 * ref["dir_loss"] + ref["iou_loss"])) < 1e-15
    from vision3d_amd.detector import ProposalLoss
    cfg = IC.make_cfg(3, with_dir=True, weight=0.25)
    maps = torch.from_numpy(c["maps"]).double()
    out = ProposalLoss(cfg)(IC.loss_item(c, maps))
    want = ref["cls_loss"] + ref["reg_loss"] + 0.2 * ref["dir_loss"] + 0.25 * ref["iou_loss"]
    assert abs(float(out["loss"]) - want) <= 1e-12
    assert 0.05 < ref["target"][c["M_reg"][..., 0]].mean() < 0.95, "the targets of a plain case spread over (0, 1)"


@pytest.fixture(scope="module")
def host_head():
    so = os.path.join(HERE, "host", "_build", "libiou_head_host.so")
    src = os.path.join(HERE, "host", "iou_head_host_shim.cpp")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-std=c++17", "-o", so, src])
    return C_.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(C_.c_void_p)


@pytest.mark.parametrize("case", IC.LOSS_CASES, ids=C.case_id)
def test_header_expressions_compiled_for_the_host(host_head, case):
    c = IC.loss_case(*case)
    ref = IC.loss_reference(case)
    pos = c["M_reg"][..., 0]
    n = int(pos.sum())
    if n == 0:
        return
    _, p_reg, _, p_iou = IH.split_maps(c["maps"], c["n_cls"], c["n_yaw"], c["with_dir"])
    anc = np.broadcast_to(c["anchors"][None], p_reg.shape)
    p, g, an, z = (np.ascontiguousarray(x[pos], np.float32) for x in (p_reg, c["G_reg"], anc, p_iou))
    outs = []
    for strided in (0, 1):
        t, bce, grad = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.float32)
        host_head.host_iou_head(_ptr(p), _ptr(g), _ptr(an), _ptr(z), n, strided, _ptr(t), _ptr(bce), _ptr(grad))
        outs.append((t, bce, grad))
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    t, bce, grad = outs[0]
    w_t = ref["target"][pos]
    z64 = z.astype(np.float64)
    assert np.abs(t - w_t).max() <= HOST_VALUE and t.min() >= 0.0 and t.max() <= 1.0
    np.testing.assert_allclose(bce, IH.soft_bce(z64, w_t), rtol=HOST_VALUE, atol=HOST_VALUE * np.maximum(1.0, np.abs(z64)).max())
    np.testing.assert_allclose(grad, IH._sigmoid(z64) - w_t, rtol=0, atol=HOST_VALUE)
    assert np.isfinite(bce).all() and np.isfinite(grad).all()
    box = np.empty((n, 7), np.float32)
    host_head.host_iou_head_decode(_ptr(p), _ptr(an), n, _ptr(box))
    want = IH.relative_boxes(p, an)
    with np.errstate(over="ignore"):
        fin = np.isfinite(want.astype(np.float32)).all(-1)
    np.testing.assert_allclose(box[fin], want[fin], rtol=1e-5, atol=1e-6)
    assert np.isinf(box[~fin]).any(-1).all()


# ------------------------------------------------------------------------------------------------------------------- score rule
def test_score_rule_on_hand_cases():
    from vision3d_amd.detector.proposal import rectified_scores
    s = np.array([0.75, 0.75, 0.75, 0.75, 0.75, 0.5, -1.0], np.float32)
    z = np.concatenate((IC.HAND_Z, np.array([1.0, 2.0], np.float32)))
    q = np.concatenate((IC.HAND_Q, [1 / (1 + math.exp(-1.0)), 0.0]))
    for power in (0, 1, 4):
        want = np.where(s >= 0, s.astype(np.float64) * q ** power, s)
        got = IH.rectify(s, z, power)
        np.testing.assert_allclose(got, want, rtol=1e-15, atol=0)
        assert got[-1] == -1.0, "a sentinel is not rectified"
        for dtype, tol in ((torch.float64, 1e-15), (torch.float32, 2e-7)):
            stated = rectified_scores(torch.from_numpy(s).to(dtype), torch.from_numpy(z), power).numpy()
            np.testing.assert_allclose(stated, want, rtol=tol, atol=0)
            assert stated[-1] == -1.0 and not np.isnan(stated).any()
        if power == 0:
            np.testing.assert_array_equal(got, s.astype(np.float64))
    # exactly: NaN and -inf give 0, +inf leaves the score, +-0 halve it per factor
    np.testing.assert_array_equal(IH.rectify(s[:5], IC.HAND_Z, 4), [0.0, 0.75, 0.0, 0.75 / 16, 0.75 / 16])
    # the power is successive multiplications from the left in the score's own format
    x, zz = torch.tensor([0.3], dtype=torch.float32), torch.tensor([0.4], dtype=torch.float32)
    qq = torch.sigmoid(zz)
    assert torch.equal(rectified_scores(x, zz, 4), (((x * qq) * qq) * qq) * qq)


def test_order_ties_fall_to_position():
    """_rectify: top-k by class score, then a stable descending sort by s'; an exact tie in s' keeps the class-score order"""
    from vision3d_amd.detector.proposal import ProposalLayer
    head = ProposalLayer(IC.make_cfg(1, topk=6, power=1))
    scores = torch.tensor([[[0.9, 0.8, 0.8, 0.7, 0.6, 0.5]]], dtype=torch.float64)
    anchor_idx = torch.tensor([[[11, 5, 7, 3, 2, 9]]])
    iou_map = torch.full((1, 1, 12), -50.0, dtype=torch.float64)
    iou_map[0, 0, [11, 5, 7, 3, 2, 9]] = torch.tensor([-1.0, 0.5, 0.5, 3.0, float("nan"), float("-inf")], dtype=torch.float64)
    rect, idx = head._rectify(scores, anchor_idx, iou_map.reshape(1, 1, 2, 2, 3))
    want = IH.rectify(scores.numpy(), [-1.0, 0.5, 0.5, 3.0, np.nan, -np.inf], 1)
    order = IH.reorder(want)
    assert order.tolist() == [[[3, 1, 2, 0, 4, 5]]], "0.7 * q(3) first; the 0.8 pair tied, in position order; the two zeros last, in position order"
    assert idx.tolist() == [[[3, 5, 7, 11, 2, 9]]]
    np.testing.assert_allclose(rect.numpy(), np.take_along_axis(want, order, 2), rtol=1e-15)
    head0 = ProposalLayer(IC.make_cfg(1, topk=6, power=0))
    same = head0._rectify(scores, anchor_idx, None)  # POWER 0 reads nothing
    assert same[0] is scores and same[1] is anchor_idx
    with pytest.raises(RuntimeError, match="IoU map"):
        head._rectify(scores, anchor_idx, None)


@pytest.mark.parametrize("with_dir", [False, True])
@pytest.mark.parametrize("case", IC.DECODE_CASES, ids=C.case_id)
def test_decode_cases_are_decided_by_margin(case, with_dir):
    c = IC.decode_case(*case, with_dir)
    B, n_cls, n_yaw, H, W, topk = c["geom"]
    for power in IC.POWERS:
        r = c["by_power"][power]
        gap = IH.relative_gaps(r["rect_unordered"])
        print(f"{C.case_id(case)} dir={with_dir} power={power}: smallest relative gap of distinct rectified scores {gap:.3e}")
        assert gap >= IC.SCORE_MARGIN
        assert r["scores"].shape == (B, n_cls, c["real"]) and (np.diff(r["scores"], axis=-1) <= 0).all()
        # equal rectified scores come from identical logits (or an exact zero) and stand in position order
        s, pos, cs, z = r["scores"], r["pos"], r["class_scores"], r["iou_logit"]
        tie = s[..., 1:] == s[..., :-1]
        assert (pos[..., 1:][tie] > pos[..., :-1][tie]).all()
        if power > 0:
            same = (cs[..., 1:] == cs[..., :-1]) & (R.score(z[..., 1:]) == R.score(z[..., :-1]))
            assert (same | (s[..., 1:] == 0))[tie].all()
            if c["hand"] is not None and c["real"] >= 7:
                assert tie.any(), "the hand-built tie is there"
                assert (r["rect_unordered"][0, 0, [0, 2]] == 0).all() and r["rect_unordered"][0, 0, 1] == r["class_scores"].max()
        else:
            assert np.array_equal(pos, np.broadcast_to(np.arange(c["real"]), pos.shape))
    if case[0] == IC.SHORT_ROW:
        assert c["real"] == 6 < topk


STAGE_PARAMS = [(row, d, p) for row in C.STAGE_CASES for d in (False, True) for p in IC.POWERS]


@pytest.mark.parametrize("row,with_dir,power", STAGE_PARAMS, ids=[C.case_id(p) for p in STAGE_PARAMS])
def test_stage_cases_are_decided_by_margin(row, with_dir, power):
    c = IC.stage_case(row, with_dir, power)
    ref = c["ref"]
    B, n_cls, n_yaw, H, W, topk = c["geom"]
    s = ref["candidates"]["scores"]
    for k in range(n_cls):
        with_thresh = np.concatenate((s[0, k], [c["thresh"][k]]))
        assert IH.relative_gaps(with_thresh[None]) >= IC.SCORE_MARGIN
        assert s[0, k].min() < c["thresh"][k] < s[0, k].max(), "the threshold lies inside the range of s'"
    # the stage's output is ordered over ALL groups: the margin holds across them too (equal values: identical logits, position decides)
    assert IH.relative_gaps(s.reshape(1, -1)) >= IC.SCORE_MARGIN
    margin = R.batched_margin(ref["bev"], ref["all_scores"], ref["groups"], c["iou"])
    print(f"{C.case_id((row, with_dir, power))}: NMS margin {margin:.3e}, kept {len(ref['cand'])} of {ref['n_nms']} NMS survivors "
          f"of {B * n_cls * topk}")
    assert margin >= C.STAGE_MARGIN
    assert 0 < len(ref["cand"]) < ref["n_nms"] < B * n_cls * topk, "the NMS suppresses some, the cut drops some and keeps some"

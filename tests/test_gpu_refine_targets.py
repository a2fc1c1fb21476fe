"""GPU: the fused stage-2 target assignment (csrc/refine_targets.hip) against the op-by-op torch statement on the same device and
against the numpy restatement (tests/refine_targets_ref.py): overlaps bit-equal, matches and masks equal, confidence targets to one
float32 ulp below 1 (torch's device division is not known to round like the library's), box targets to the tolerance
tests/test_gpu_targets.py uses for encoded boxes.  What the generated inputs contain is asserted on the CPU
(tests/test_host_refine_targets.py)."""
import numpy as np
import pytest
import torch

import refine_targets_ref as R
from vision3d_amd import synth
from vision3d_amd.core.config import _defaults

pytestmark = pytest.mark.gpu


def make_item(case):
    p, pc, boxes, cls, draws = case
    return dict(proposals=torch.from_numpy(p).cuda(), proposal_class=torch.from_numpy(pc).cuda(), boxes=[torch.from_numpy(b) for b in boxes],
                class_idx=[torch.from_numpy(c) for c in cls], refine_draws=torch.from_numpy(draws).cuda())


def assigner(**train):
    from vision3d_amd.core import RefinementTargetAssigner
    cfg = _defaults().clone()
    cfg.TRAIN.merge_from_dict(train)
    return RefinementTargetAssigner(cfg)


def check(got, want, what):
    """got: the fused outputs; want: forward_torch's tensors or the restatement's arrays."""
    g = {k: got[k].cpu().numpy() for k in ("R_iou", "R_match", "G_conf", "G_rreg", "M_rcls", "M_rreg")}
    w = {k: (want[k].cpu().numpy() if torch.is_tensor(want[k]) else want[k]) for k in g}
    np.testing.assert_array_equal(g["R_iou"].view(np.uint32), w["R_iou"].view(np.uint32), err_msg=what)
    for k in ("R_match", "M_rcls", "M_rreg"):
        assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape, (what, k)
        np.testing.assert_array_equal(g[k], w[k], err_msg=f"{what} {k}")
    np.testing.assert_allclose(g["G_conf"], w["G_conf"], rtol=0, atol=2e-7, err_msg=what)
    np.testing.assert_array_equal(g["G_conf"] == 0, w["G_conf"] == 0, err_msg=what)
    np.testing.assert_array_equal(g["G_conf"] == 1, w["G_conf"] == 1, err_msg=what)
    np.testing.assert_allclose(g["G_rreg"], w["G_rreg"], rtol=1e-5, atol=1e-6, err_msg=what)


def both(a, case, what, **ref_kw):
    fused, stated = a(make_item(case)), a.forward_torch(make_item(case))
    check(fused, stated, what + " vs forward_torch")
    check(fused, R.assign(*case, **ref_kw), what + " vs restatement")
    return fused


@pytest.mark.parametrize("n_cls,batch", R.CONFIGS)
def test_fused_matches_torch_statement_and_restatement(n_cls, batch):
    a = assigner()
    for seed in R.SEEDS:
        out = both(a, synth.make_refine_case(seed, n_cls=n_cls, batch=batch), f"{n_cls} classes, B {batch}, seed {seed}")
        assert int(out["M_rreg"].sum()) > 0 and not bool(out["M_rcls"].all())


def test_other_sampling_and_threshold_settings():
    case = synth.make_refine_case(2, n_cls=3, batch=2)
    both(assigner(REFINEMENT_ROIS_PER_FRAME=0), case, "take all", rois_per_frame=0)
    both(assigner(REFINEMENT_ROIS_PER_FRAME=48, REFINEMENT_FG_FRACTION=0.25, REFINEMENT_FG_IOU=0.6, REFINEMENT_REG_IOU=0.45,
                  REFINEMENT_CONF_IOU=[0.3, 0.7]), case, "other settings", rois_per_frame=48, fg_fraction=0.25, fg_iou=0.6, reg_iou=0.45,
         conf_iou=(0.3, 0.7))
    tied = list(case)
    tied[4] = np.round(case[4] * 4) / 4  # five distinct draws: the index decides
    both(assigner(), tuple(tied), "tied draws")


def test_edge_shapes():
    a = assigner()
    p, pc, boxes, cls, draws = synth.make_refine_case(4, n_cls=3, batch=3, topk=37)  # n = 111: not a multiple of 64
    boxes[1], cls[1] = boxes[1][:0], cls[1][:0]                                       # a frame with no ground truth
    keep = cls[2] != 1
    boxes[2], cls[2] = boxes[2][keep], cls[2][keep]                                    # a class with no ground truth
    out = both(a, (p, pc, boxes, cls, draws), "edges")
    assert not bool(out["R_iou"][1].any()) and bool((out["R_match"][1] == -1).all()) and not bool(out["M_rreg"][1].any())
    assert bool((out["R_match"][2][pc == 1] == -1).all())
    one = synth.make_refine_case(6, n_cls=1, batch=2, gt_per_class=1)
    both(a, one, "one ground truth per frame")
    full = synth.make_refine_case(7, n_cls=1, batch=2, topk=1280, gt_per_class=128)  # ten RoIs from EVERY ground truth, the last included
    out = both(a, full, "128 ground truths per frame")
    assert bool((out["R_match"][0] == 127).any()) and bool((out["R_match"][1] == 255).any()), "the last staged ground truth is matched"


def test_over_limit_inputs_take_the_fallback():
    a = assigner()
    many_gt = synth.make_refine_case(8, n_cls=1, batch=2, topk=1290, gt_per_class=129)  # RoIs from every ground truth, the 129th included
    many_roi = synth.make_refine_case(9, n_cls=1, batch=1, topk=2049, gt_per_class=4)
    for case, what in ((many_gt, "129 ground truths"), (many_roi, "2 049 RoIs")):
        out = a(make_item(case))
        check(out, R.assign(*case), what)
    out = a(make_item(many_gt))
    assert bool((out["R_match"][0] == 128).any()) and bool((out["R_match"][1] == 257).any()), "the ground truth beyond the kernel's limit is matched"


def test_repeatable_and_independent_of_other_frames():
    a = assigner()
    case = synth.make_refine_case(1, n_cls=3, batch=4)
    keys = ("R_iou", "R_match", "G_conf", "G_rreg", "M_rcls", "M_rreg")
    x, y = a(make_item(case)), a(make_item(case))
    for k in keys:
        assert torch.equal(x[k], y[k]), k
    perm = [0, 3, 1, 2]  # frame 0 stays where it is, the others move
    p, pc, boxes, cls, draws = case
    z = a(make_item((p[perm], pc, [boxes[i] for i in perm], [cls[i] for i in perm], draws[perm])))
    for k in keys:
        assert torch.equal(x[k][0], z[k][0]), k
    off = [0] + np.cumsum([len(b) for b in boxes]).tolist()
    for new, old in enumerate(perm):  # the other frames: the same answers, matches re-based on their new place in the list
        new_off = sum(len(boxes[i]) for i in perm[:new])
        for k in keys:
            want = x[k][old]
            if k == "R_match":
                want = torch.where(want >= 0, want - off[old] + new_off, want)
            assert torch.equal(want, z[k][new]), (k, new)

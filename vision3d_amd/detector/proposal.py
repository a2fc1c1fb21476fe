"""BEV proposal head and its loss (interface of vision3d/detector/proposal.py:10-141).

ProposalLayer: 1x1 class/box heads -> (B, n_cls, n_yaw, ny, nx[, 7]); inference = sigmoid, top-k per
(frame, class), VoxelNet decode, multi-class rotated NMS (IoU 0.01) and per-class score threshold.
Index bookkeeping tensors are created on the scores' device (the reference mixes CPU and GPU tensors,
legal only in torch 1.4 -- SURVEY.md H9).

cfg.DIRECTION (opt-in, not in the reference): the direction classifier and sine yaw loss of the SECOND paper.  The encoded yaw
residual is right only modulo pi; one more 1x1 head, conv_dir, gives a logit per anchor that says which half turn (fused map
[cls | reg | dir], forward returns a third map, the decode applies `direction_yaw`), ProposalLoss gains dir_loss and, with SIN_YAW,
takes sin(P_yaw - G_yaw) as the yaw column's smooth-L1 argument.  Definition: DESIGN.md section 7, tests/direction_ref.py.

cfg.IOU_HEAD (opt-in, not in the reference): an IoU-aware confidence, the rectified score of CIA-SSD / SE-SSD / SECOND-IoU.  One more
1x1 head, conv_iou, gives a logit per anchor (fused map [cls | reg | (dir) | iou], forward returns one more map behind the direction
map) trained towards the rotated 3-D IoU of the anchor's decoded box with its object (ProposalLoss.iou_targets, iou_loss); inference
selects the TOPK of a (frame, class) by class score as before and then ranks, suppresses and cuts by `rectified_scores`.
Definition: DESIGN.md section 7, tests/iou_head_ref.py.

cfg.BOX_VOTING (opt-in, not in the reference): IoU-weighted box voting behind the NMS of every tail here -- `native_proposals`
(v3d_proposals_vote_flag) and `native_refine_nms` (v3d_refine_nms_vote) in one more launch each, the torch statements
(`inference_from_maps`, `proposals_padded` + `finalize`) through ops.box_voting_statement.  Boxes move only: scores, indices, order and
count are those of the tail without the vote.  `native_topk` runs no NMS and does not vote.  Definition: DESIGN.md section 7,
ops/box_voting.py, tests/box_voting_ref.py.
"""
import math

import torch
import torch.nn.functional as F
from torch import nn

from .. import _lib as L
from ..core.box_encode import decode
from ..core.config import box_voting_config, iou_head_config
from ..core.proposal_targets import direction_config
from ..ops import batched_nms_rotated, batched_nms_rotated_padded, sigmoid_focal_loss
from ..stamp import cached
from .fused_loss import scale_gradient, take_gradient


def direction_enabled(cfg):
    return bool(direction_config(cfg)["ENABLED"])


def refuse_direction(cfg, what):
    """The models that do not know the direction classifier yet (follow-ups) say so instead of building a head that ignores it."""
    if direction_enabled(cfg):
        raise ValueError(f"cfg.DIRECTION.ENABLED: {what} does not support the direction classifier yet (Second with the anchor head "
                         "does)")


def iou_head_enabled(cfg):
    return bool(iou_head_config(cfg)["ENABLED"])


def refuse_iou_head(cfg, what):
    """The models that have no use for the IoU-aware confidence say so instead of building a head that ignores the key."""
    if iou_head_enabled(cfg):
        raise ValueError(f"cfg.IOU_HEAD.ENABLED: {what} does not take the IoU-aware confidence head (Second with the anchor head does)")


def checked_iou_head(cfg):
    """cfg.IOU_HEAD over its defaults, refused where an enabled head could not mean what it says."""
    opt = iou_head_config(cfg)
    if opt["ENABLED"]:
        power = opt["POWER"]
        if isinstance(power, bool) or not isinstance(power, int) or not 0 <= power <= 8:
            raise ValueError(f"cfg.IOU_HEAD.POWER must be an integer in 0 .. 8 (0: the scores stay as they are), got {power!r}")
        if cfg.BOX_DOF != 7:
            raise ValueError("cfg.IOU_HEAD.ENABLED: the IoU target is defined for 7-DOF boxes (cfg.BOX_DOF)")
    return opt


def box_voting_enabled(cfg):
    return bool(box_voting_config(cfg)["ENABLED"])


def refuse_box_voting(cfg, what):
    """The heads whose decode runs its own fused NMS say so instead of ignoring the key."""
    if box_voting_enabled(cfg):
        raise ValueError(f"cfg.BOX_VOTING.ENABLED: {what} does not vote its boxes yet (the tails of ProposalLayer do)")


def checked_box_voting(cfg):
    """cfg.BOX_VOTING over its defaults (core.config.box_voting_config validates IOU), refused where the vote is not defined."""
    opt = box_voting_config(cfg)
    if opt["ENABLED"] and cfg.BOX_DOF != 7:
        raise ValueError("cfg.BOX_VOTING.ENABLED: the vote is defined for 7-DOF boxes (cfg.BOX_DOF)")
    return opt


def fused_convs(head):
    """The 1x1 convolutions of a head in the channel order of its fused map: [conv_cls | conv_reg], then conv_dir for a ProposalLayer
    with a direction classifier, then conv_iou for one with an IoU-aware confidence: [cls | reg | (dir) | (iou)].  The one statement of
    that order for runtime.DenseHeadPlan, ProposalLayer.native_head and dense_train.DenseTrainPlan."""
    convs = [head.conv_cls, head.conv_reg]
    for name in ("conv_dir", "conv_iou"):
        conv = getattr(head, name, None)
        if conv is not None:
            convs.append(conv)
    return convs


def rectified_scores(scores, iou_logit, power):
    """The score rule of cfg.IOU_HEAD: s' = s * q^POWER, q = sigmoid(IoU logit) with NaN counted as -inf (q = 0), the power as POWER
    successive multiplications from the left; a sentinel (s < 0) keeps its score.  In the dtype of `scores`."""
    z = iou_logit.to(scores.dtype)
    q = torch.sigmoid(torch.where(torch.isnan(z), torch.full_like(z, -math.inf), z))
    out = scores
    for _ in range(int(power)):
        out = out * q
    return torch.where(scores >= 0, out, scores)


def relative_boxes(deltas, anchors):
    """core/box_encode.py:decode WITHOUT the anchor's centre (the IoU is translation invariant; csrc/iou_head_device.h):
    (d_xyz * (diag, diag, a_h), exp(d_wlh) * a_wlh, d_yaw + a_yaw)."""
    diag = torch.sqrt(anchors[..., 3] * anchors[..., 3] + anchors[..., 4] * anchors[..., 4])
    return torch.stack((deltas[..., 0] * diag, deltas[..., 1] * diag, deltas[..., 2] * anchors[..., 5],
                        torch.exp(deltas[..., 3]) * anchors[..., 3], torch.exp(deltas[..., 4]) * anchors[..., 4],
                        torch.exp(deltas[..., 5]) * anchors[..., 5], deltas[..., 6] + anchors[..., 6]), -1)


def direction_yaw(raw, dir_logit, offset):
    """The decode rule of cfg.DIRECTION: remainder(raw - OFFSET, pi) + OFFSET + pi * [dir_logit > 0] (strict: +-0 and NaN give 0), in
    the dtype of `raw`; the result lies in [OFFSET, OFFSET + 2 pi)."""
    pi, off = raw.new_tensor(math.pi), raw.new_tensor(offset)
    return torch.remainder(raw - off, pi) + off + pi * (dir_logit > 0).to(raw.dtype)


_PINNED = {}


def _pinned_pair(device):
    """Two pinned int32 words per device for the per-frame count / overflow read (host code is sequential: copy, sync, read)."""
    key = str(device)
    if key not in _PINNED:
        _PINNED[key] = torch.empty(2, dtype=torch.int32).pin_memory()
    return _PINNED[key]


def _raise_on_flag(word):
    """The frame's summary word (csrc/v3d_internal.h): 1 = a capacity was hit, 2 = an f16s tensor left its calibrated range, 3 = an
    f16s tensor stayed 2^12 below it (precision at risk: recalibrate downward)."""
    if word == 3:
        from ..runtime import RangeUnderflow
        raise RangeUnderflow("f16s arithmetic: a tensor of this frame stayed 2^12 below its calibrated range (the fp32-class precision "
                             "is not guaranteed); recalibrate on this frame and run it again (Second.inference and the graph runners do)")
    if word == 2:
        from ..runtime import RangeOverflow
        raise RangeOverflow("f16s arithmetic: a tensor of this frame exceeded its calibrated range (results invalid); recalibrate "
                            "on this frame and run it again (Second.inference and the graph runners do)")
    if word > 0:
        raise RuntimeError("sparse backbone: a stage exceeded its active-site capacity (rows were dropped); build the "
                           "plan with a larger `growth` (Second.plan_growth / BackbonePlan(growth=...))")


class ProposalLayer(nn.Module):

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        n_anchor = cfg.NUM_CLASSES * cfg.NUM_YAW
        self.conv_cls = nn.Conv2d(cfg.PROPOSAL.C_IN, n_anchor, 1)
        self.conv_reg = nn.Conv2d(cfg.PROPOSAL.C_IN, n_anchor * cfg.BOX_DOF, 1)
        self.TOPK, self.DOF = cfg.PROPOSAL.TOPK, cfg.BOX_DOF
        self.direction = direction_config(cfg)
        self.iou_head = checked_iou_head(cfg)
        self.box_voting = checked_box_voting(cfg)
        self._init_weights()
        if self.direction["ENABLED"]:
            # cfg.DIRECTION (opt-in): one more logit per anchor, the half turn the wrapped yaw residual cannot carry.  Built behind the
            # reference's two heads, so that their initial values do not depend on it
            if cfg.BOX_DOF != 7:
                raise ValueError("cfg.DIRECTION.ENABLED: the direction classifier is defined for 7-DOF boxes")
            self.conv_dir = nn.Conv2d(cfg.PROPOSAL.C_IN, n_anchor, 1)
            nn.init.constant_(self.conv_dir.bias, 0)
            nn.init.normal_(self.conv_dir.weight, std=0.01)
        if self.iou_head["ENABLED"]:
            # cfg.IOU_HEAD (opt-in): one more logit per anchor, the predicted IoU of its decoded box.  Built behind every other head,
            # so that their initial values under a seed do not depend on it
            self.conv_iou = nn.Conv2d(cfg.PROPOSAL.C_IN, n_anchor, 1)
            nn.init.constant_(self.conv_iou.bias, 0)
            nn.init.normal_(self.conv_iou.weight, std=0.01)

    def _init_weights(self):
        # focal-prior bias exactly as the reference writes it: +1.005 (proposal.py:27)
        nn.init.constant_(self.conv_cls.bias, (-math.log(1 - .01) / .01))
        nn.init.constant_(self.conv_reg.bias, 0)
        nn.init.normal_(self.conv_cls.weight, std=0.01)
        nn.init.normal_(self.conv_reg.weight, std=0.01)

    def _generate_group_idx(self, B, n_cls, device=None):
        """(batch_idx, class_idx, group_idx), each (B * n_cls * TOPK,), group = class + n_cls * batch."""
        b = torch.arange(B, device=device).view(B, 1, 1).expand(B, n_cls, self.TOPK)
        c = torch.arange(n_cls, device=device).view(1, n_cls, 1).expand(B, n_cls, self.TOPK)
        return b.reshape(-1), c.reshape(-1), (c + n_cls * b).reshape(-1)

    def _above_score_thresh(self, scores, class_idx):
        thresh = scores.new_tensor([a["score_thresh"] for a in self.cfg.ANCHORS])
        return scores > thresh[class_idx]

    def _multiclass_batch_nms(self, boxes, scores):
        B, n_cls = scores.shape[:2]
        scores = scores.reshape(-1)
        boxes = boxes.reshape(-1, self.DOF)
        bev = boxes[:, [0, 1, 3, 4, 6]].contiguous()
        batch_idx, class_idx, group_idx = self._generate_group_idx(B, n_cls, scores.device)
        keep = batched_nms_rotated(bev, scores, group_idx, iou_threshold=0.01)
        boxes = self._voted(boxes, scores, B * n_cls)
        boxes, batch_idx, class_idx, scores = (x[keep] for x in (boxes, batch_idx, class_idx, scores))
        mask = self._above_score_thresh(scores, class_idx)
        return [x[mask] for x in (boxes, batch_idx, class_idx, scores)]

    def _voted(self, boxes, scores, n_groups):
        """cfg.BOX_VOTING in the torch statements: the (N, 7) group-major candidates, every one voted by its group (the NMS has been
        decided on `boxes` as they came; the keep list then selects voted rows); without the key: `boxes` itself."""
        if not self.box_voting["ENABLED"]:
            return boxes
        from ..ops.box_voting import box_voting_statement
        shape = (n_groups, boxes.shape[0] // n_groups)
        return box_voting_statement(boxes.reshape(*shape, 7), scores.reshape(shape), self.box_voting["IOU"]).reshape(-1, 7)

    def _dir_map(self, dir_map):
        """The direction map a decode of this head needs: None for a head without the classifier, else required."""
        if not self.direction["ENABLED"]:
            return None
        if dir_map is None:
            raise RuntimeError("cfg.DIRECTION.ENABLED: the decode needs the direction map (dir_from_fused) beside the class and box maps")
        return dir_map

    def _split_extra(self, extra):
        """(dir_map, iou_map) from what follows (cls_map, reg_map) in the outputs of `forward`."""
        extra = list(extra)
        dir_map = extra.pop(0) if self.direction["ENABLED"] and extra else None
        iou_map = extra.pop(0) if self.iou_head["ENABLED"] and extra else None
        return dir_map, iou_map

    def _rectify(self, scores, anchor_idx, iou_map):
        """cfg.IOU_HEAD behind the top-k by class score: (scores, anchor_idx) (B, n_cls, TOPK) -> the same candidates with s' =
        rectified_scores in place of the score, in a stable descending order of s' (ties: the position in the class-score order).
        A head without the key, and POWER = 0, change nothing and read nothing."""
        if not self.iou_head["ENABLED"] or self.iou_head["POWER"] == 0:
            return scores, anchor_idx
        if iou_map is None:
            raise RuntimeError("cfg.IOU_HEAD.ENABLED: the proposal stage needs the IoU map (iou_from_fused) beside the class and box maps")
        B, n_cls = scores.shape[:2]
        rect = rectified_scores(scores, iou_map.reshape(B, n_cls, -1).gather(2, anchor_idx), self.iou_head["POWER"])
        rect, order = torch.sort(rect, dim=-1, descending=True, stable=True)
        return rect, anchor_idx.gather(2, order)

    def _decode(self, reg_map, anchors, anchor_idx, dir_map=None):
        B, n_cls = reg_map.shape[:2]
        gidx = anchor_idx[..., None].expand(-1, -1, -1, self.DOF)
        deltas = reg_map.reshape(B, n_cls, -1, self.DOF).gather(2, gidx)
        anc = anchors.reshape(1, n_cls, -1, self.DOF).expand(B, -1, -1, -1).gather(2, gidx)
        boxes = decode(deltas, anc)
        dir_map = self._dir_map(dir_map)
        if dir_map is not None:
            logit = dir_map.reshape(B, n_cls, -1).gather(2, anchor_idx)
            boxes = torch.cat((boxes[..., :6], direction_yaw(boxes[..., 6], logit, self.direction["OFFSET"])[..., None]), -1)
        return boxes

    def inference(self, feature_map, anchors):
        """-> (boxes (K,7), batch_idx (K,), class_idx (K,), scores (K,)), by decreasing score."""
        maps = self(feature_map)  # (cls_map, reg_map[, dir_map][, iou_map])
        return self.inference_from_maps(maps[0], maps[1], anchors, *self._split_extra(maps[2:]))

    def maps_from_fused(self, maps):
        """(B, n_anchor*(1+DOF)[+ n_anchor][+ n_anchor], H, W) = [cls | reg (| dir) (| iou)] channels of the fused 1x1 head ->
        (cls_map, reg_map)."""
        n_anchor = self.cfg.NUM_CLASSES * self.cfg.NUM_YAW
        return (self.reshape_cls(maps[:, :n_anchor].contiguous()),
                self.reshape_reg(maps[:, n_anchor:n_anchor * (1 + self.DOF)].contiguous()))

    def dir_from_fused(self, maps):
        """The direction logits of a fused [cls | reg | dir] map in the shape of cls_map; None for a head without the classifier."""
        if not self.direction["ENABLED"]:
            return None
        n_anchor = self.cfg.NUM_CLASSES * self.cfg.NUM_YAW
        return self.reshape_cls(maps[:, n_anchor * (1 + self.DOF):n_anchor * (2 + self.DOF)].contiguous())

    def iou_from_fused(self, maps):
        """The IoU logits of a fused [cls | reg | (dir) | iou] map in the shape of cls_map; None for a head without cfg.IOU_HEAD."""
        if not self.iou_head["ENABLED"]:
            return None
        n_anchor = self.cfg.NUM_CLASSES * self.cfg.NUM_YAW
        base = n_anchor * (1 + self.DOF + bool(self.direction["ENABLED"]))
        return self.reshape_cls(maps[:, base:base + n_anchor].contiguous())

    def extra_from_fused(self, maps):
        """(dir_map, iou_map) of a fused map: what the torch statements take behind (cls_map, reg_map, anchors)."""
        return self.dir_from_fused(maps), self.iou_from_fused(maps)

    def proposals_padded(self, cls_map, reg_map, anchors, dir_map=None, iou_map=None):
        """Everything up to (and including) NMS with NO host synchronisation: returns the B*n_cls*TOPK
        candidates (boxes, batch_idx, class_idx, scores) plus (keep padded, n_keep) on the device.  This is
        the part that can live inside a captured HIP graph; `finalize` does the variable-length selection.
        For a NaN logit this statement behaves differently from `native_proposals`: torch.topk sorts NaN first, the kernel last."""
        score_map = cls_map.sigmoid()
        B, n_cls = score_map.shape[:2]
        scores, anchor_idx = self._rectify(*score_map.reshape(B, n_cls, -1).topk(self.TOPK, -1), iou_map)
        boxes = self._decode(reg_map, anchors, anchor_idx, dir_map).reshape(-1, self.DOF)
        scores = scores.reshape(-1)
        batch_idx, class_idx, group_idx = self._generate_group_idx(B, n_cls, scores.device)
        # column select without a host-built index tensor (an H2D copy is illegal during graph capture)
        bev = torch.stack((boxes[:, 0], boxes[:, 1], boxes[:, 3], boxes[:, 4], boxes[:, 6]), dim=1)
        keep, n_keep = batched_nms_rotated_padded(bev, scores, group_idx, 0.01)
        return self._voted(boxes, scores, B * n_cls), batch_idx, class_idx, scores, keep, n_keep

    def native_supported(self, batch_size, anchors_per_class=None):
        """csrc/proposal.hip sorts the candidates of all (frame, class) groups in one workgroup (<= 1024 of them) and
        selects each group's top-k in two levels of <= 40 register-resident slices of <= 8192 anchors."""
        ok = batch_size * self.cfg.NUM_CLASSES * self.TOPK <= 1024 and self.DOF == 7 and self.cfg.NUM_CLASSES <= 16
        if anchors_per_class is not None:
            ok = ok and anchors_per_class <= 8192 * min(40, 4096 // self.TOPK)
        return ok

    def native_proposals(self, head_maps, anchors, overflow_flag=None, host_out=None):
        """The whole stage after the 1x1 heads in libvision3d_hip.so (csrc/proposal.hip: 8 launches, no host
        sync): head_maps (B, n_anchor*(1+DOF), H, W) = [cls | reg] channels of the fused head.  Returns padded
        (boxes (N,7), batch_idx, class_idx, scores, n_out int32 on the device); capturable in a HIP graph.
        overflow_flag (a plan's (1,) device word): copied into n_out[1] by the last kernel, so that `finalize_native` reads
        the count and the plan's capacity verdict with ONE 8-byte copy.
        host_out (a PINNED int32 host tensor of two words, kept by the caller): the last kernel stores the pair straight into it
        (pinned memory is device-accessible) -- no copy is enqueued behind the frame at all; `finalize_native` synchronises the
        stream and reads it.
        Non-finite logits: +inf scores 1.0 and -inf 0.0; a NaN class logit of either sign counts as -inf (score 0.0, tied with the
        other zeros by anchor index, selected only when fewer than TOPK other anchors exist) -- never an out-of-range anchor."""
        cfg = self.cfg
        L.require_gpu("proposals", head_maps, anchors)
        maps, anc = L.as_f32("proposals", head_maps), L.as_f32("proposals", anchors)
        B, ctot, H, W = maps.shape
        n_cls, n_yaw = cfg.NUM_CLASSES, cfg.NUM_YAW
        with_dir = bool(self.direction["ENABLED"])  # [cls | reg | dir] maps: v3d_proposals_dir_flag applies the direction decode rule
        with_iou = bool(self.iou_head["ENABLED"])   # [cls | reg | (dir) | iou] maps: v3d_proposals_iou_flag rectifies the scores
        if ctot != n_cls * n_yaw * (1 + self.DOF + with_dir + with_iou) or self.DOF != 7 or anc.numel() != n_cls * n_yaw * H * W * 7:
            raise RuntimeError("proposals: head map / anchor grid shapes disagree")
        N = B * n_cls * self.TOPK
        dev = maps.device
        boxes = torch.empty((N, 7), dtype=torch.float32, device=dev)
        batch_idx = torch.empty((N,), dtype=torch.int64, device=dev)
        class_idx = torch.empty((N,), dtype=torch.int64, device=dev)
        scores = torch.empty((N,), dtype=torch.float32, device=dev)
        if host_out is not None:
            if not (host_out.is_pinned() and host_out.dtype == torch.int32 and host_out.numel() == 2 and overflow_flag is not None):
                raise RuntimeError("proposals: host_out is a pinned int32 pair, and needs the plan's flag word beside the count")
            n_out = host_out
        else:
            n_out = torch.empty((1 if overflow_flag is None else 2,), dtype=torch.int32, device=dev)  # written by the last kernel
        lib = L.lib()
        vote = bool(self.box_voting["ENABLED"])     # cfg.BOX_VOTING: v3d_proposals_vote_flag takes any of the three maps and votes
        ws = L.workspace((lib.v3d_proposals_vote_workspace if vote else lib.v3d_proposals_workspace)(B, n_cls, self.TOPK), dev)
        thresh = L.host_f32([a["score_thresh"] for a in cfg.ANCHORS[:n_cls]])
        entry, extra = (lib.v3d_proposals_dir_flag, (float(self.direction["OFFSET"]),)) if with_dir else (lib.v3d_proposals_flag, ())
        if with_iou:
            entry, extra = lib.v3d_proposals_iou_flag, (float(self.direction["OFFSET"]), int(with_dir), int(self.iou_head["POWER"]))
        if vote:
            entry, extra = lib.v3d_proposals_vote_flag, (float(self.direction["OFFSET"]), int(with_dir), int(with_iou),
                                                         int(self.iou_head["POWER"]), float(self.box_voting["IOU"]))
        with L.device_guard(dev):
            L.check(entry(L.ptr(maps), L.ptr(anc), B, n_cls, n_yaw, H, W, self.TOPK, thresh, 0.01, L.ptr(boxes),
                          L.ptr(batch_idx), L.ptr(class_idx), L.ptr(scores), L.ptr(n_out), L.ptr(overflow_flag),
                          L.ptr(ws), ws.numel(), L.stream_ptr(), *extra), "proposals")
        return boxes, batch_idx, class_idx, scores, n_out

    def native_topk(self, head_maps, anchors):
        """The decoded top-k candidates BEFORE NMS (v3d_proposals_topk): boxes (B, n_cls * TOPK, 7), scores (B, n_cls * TOPK), in the
        order of `scores.topk` + `_decode` of the torch statement (ties: anchor index ascending).  No host synchronisation."""
        cfg = self.cfg
        L.require_gpu("proposals_topk", head_maps, anchors)
        maps, anc = L.as_f32("proposals_topk", head_maps), L.as_f32("proposals_topk", anchors)
        B, ctot, H, W = maps.shape
        n_cls, n_yaw = cfg.NUM_CLASSES, cfg.NUM_YAW
        with_dir, with_iou = bool(self.direction["ENABLED"]), bool(self.iou_head["ENABLED"])
        if ctot != n_cls * n_yaw * (1 + self.DOF + with_dir + with_iou) or self.DOF != 7 or anc.numel() != n_cls * n_yaw * H * W * 7:
            raise RuntimeError("proposals_topk: head map / anchor grid shapes disagree")
        N = B * n_cls * self.TOPK
        boxes = torch.empty((B, n_cls * self.TOPK, 7), dtype=torch.float32, device=maps.device)
        scores = torch.empty((B, n_cls * self.TOPK), dtype=torch.float32, device=maps.device)
        lib = L.lib()
        ws = L.workspace(lib.v3d_proposals_workspace(B, n_cls, self.TOPK), maps.device)
        entry, extra = (lib.v3d_proposals_dir_topk, (float(self.direction["OFFSET"]),)) if with_dir else (lib.v3d_proposals_topk, ())
        if with_iou:  # (the candidates of a group then come in the order of the rectified score, which is what `scores` holds)
            entry, extra = lib.v3d_proposals_iou_topk, (float(self.direction["OFFSET"]), int(with_dir), int(self.iou_head["POWER"]))
        with L.device_guard(maps.device):
            L.check(entry(L.ptr(maps), L.ptr(anc), B, n_cls, n_yaw, H, W, self.TOPK, L.ptr(boxes), L.ptr(scores), L.ptr(ws),
                          ws.numel(), L.stream_ptr(), *extra), "proposals_topk")
        assert N == boxes.shape[0] * boxes.shape[1]
        return boxes, scores

    def native_refine_nms(self, deltas, proposals, conf, iou_threshold=0.01, finalize=True):
        """Stage-2 tail (v3d_refine_nms): deltas / proposals (B, n_cls * TOPK, 7) and conf (B, n_cls * TOPK[, 1]) in the layout of
        `native_topk` -> (refined boxes (B, n, 7), [boxes, batch_idx, class_idx, scores] of the survivors by decreasing score).  One
        host read (the count); finalize=False: no host read -- the second value is (boxes, batch_idx, class_idx, scores, n_out) padded,
        n_out the device word (PV_RCNN.inference_end reads it through an event)."""
        cfg = self.cfg
        d, p, c = (L.as_f32("refine_nms", t) for t in (deltas, proposals, conf))
        L.require_gpu("refine_nms", d, p, c)
        B, n = p.shape[:2]
        n_cls = cfg.NUM_CLASSES
        if n != n_cls * self.TOPK or d.shape != p.shape or c.numel() != B * n or p.shape[-1] != 7:
            raise RuntimeError("refine_nms: candidates are not in the (B, n_cls * TOPK) layout of native_topk")
        N, dev = B * n, p.device
        refined = torch.empty((B, n, 7), dtype=torch.float32, device=dev)
        boxes = torch.empty((N, 7), dtype=torch.float32, device=dev)
        batch_idx = torch.empty((N,), dtype=torch.int64, device=dev)
        class_idx = torch.empty((N,), dtype=torch.int64, device=dev)
        scores = torch.empty((N,), dtype=torch.float32, device=dev)
        n_out = torch.empty((1,), dtype=torch.int32, device=dev)
        lib = L.lib()
        vote = bool(self.box_voting["ENABLED"])  # cfg.BOX_VOTING: v3d_refine_nms_vote -- `refined` stays the un-voted decode
        ws = L.workspace((lib.v3d_proposals_vote_workspace if vote else lib.v3d_refine_nms_workspace)(B, n_cls, self.TOPK), dev)
        thresh = L.host_f32([a["score_thresh"] for a in cfg.ANCHORS[:n_cls]])
        entry, extra = (lib.v3d_refine_nms_vote, (float(self.box_voting["IOU"]),)) if vote else (lib.v3d_refine_nms, ())
        with L.device_guard(dev):
            L.check(entry(L.ptr(d), L.ptr(p), L.ptr(c), B, n_cls, self.TOPK, thresh, float(iou_threshold), L.ptr(refined),
                          L.ptr(boxes), L.ptr(batch_idx), L.ptr(class_idx), L.ptr(scores), L.ptr(n_out), L.ptr(ws), ws.numel(),
                          L.stream_ptr(), *extra), "refine_nms")
        if not finalize:
            return refined, (boxes, batch_idx, class_idx, scores, n_out)
        return refined, self.finalize_native(boxes, batch_idx, class_idx, scores, n_out)

    @staticmethod
    def finalize_native(boxes, batch_idx, class_idx, scores, n_out, overflow_flag=None, done=None):
        """The one host read of the frame (the reference synchronises inside its NMS): the number of proposals and, when
        the frame came through a BackbonePlan, that plan's capacity-overflow word in the same synchronisation -- a stage
        that hit its active-site capacity has dropped rows, so the BEV map is wrong and the frame must not be returned.
        done (an event recorded behind the frame): waited for instead of the whole stream -- a later frame may already be queued there."""
        if not n_out.is_cuda:  # the pinned pair the last kernel wrote itself (native_proposals host_out): wait for the frame, read
            if done is not None:
                done.synchronize()
            else:
                torch.cuda.current_stream(boxes.device).synchronize()
            n, ovf = int(n_out[0]), int(n_out[1])
            _raise_on_flag(ovf)
        elif overflow_flag is None and n_out.numel() == 1:
            n = int(n_out.item())
        else:
            host = _pinned_pair(n_out.device)
            if n_out.numel() == 2:  # the proposal stage already put the plan's verdict next to the count: one copy
                host.copy_(n_out, non_blocking=True)
            else:
                host[0:1].copy_(n_out, non_blocking=True)
                host[1:2].copy_(overflow_flag, non_blocking=True)
            torch.cuda.current_stream(n_out.device).synchronize()
            n, ovf = int(host[0]), int(host[1])
            _raise_on_flag(ovf)
        return [boxes[:n], batch_idx[:n], class_idx[:n], scores[:n]]

    def inference_native(self, head_maps, anchors, overflow_flag=None):
        if not self.native_supported(head_maps.shape[0], anchors.numel() // (7 * self.cfg.NUM_CLASSES)):  # too large: op-by-op
            cls_map, reg_map = self.maps_from_fused(head_maps)
            out = self.inference_from_maps(cls_map, reg_map, anchors, *self.extra_from_fused(head_maps))
            if overflow_flag is not None:
                _raise_on_flag(int(overflow_flag.item()))
            return out
        return self.finalize_native(*self.native_proposals(head_maps, anchors, overflow_flag))

    def finalize(self, boxes, batch_idx, class_idx, scores, keep, n_keep):
        keep = keep[: int(n_keep.item())]
        boxes, batch_idx, class_idx, scores = (x[keep] for x in (boxes, batch_idx, class_idx, scores))
        mask = self._above_score_thresh(scores, class_idx)
        return [x[mask] for x in (boxes, batch_idx, class_idx, scores)]

    def inference_from_maps(self, cls_map, reg_map, anchors, dir_map=None, iou_map=None):
        score_map = cls_map.sigmoid_()
        B, n_cls = score_map.shape[:2]
        scores, anchor_idx = self._rectify(*score_map.view(B, n_cls, -1).topk(self.TOPK, -1), iou_map)
        boxes = self._decode(reg_map, anchors, anchor_idx, dir_map)
        return self._multiclass_batch_nms(boxes, scores)

    def reshape_cls(self, cls_map):
        B, _, ny, nx = cls_map.shape
        return cls_map.view(B, self.cfg.NUM_CLASSES, self.cfg.NUM_YAW, ny, nx)

    def reshape_reg(self, reg_map):
        B, _, ny, nx = reg_map.shape
        return reg_map.view(B, self.cfg.NUM_CLASSES, self.cfg.BOX_DOF, -1, ny, nx).permute(0, 1, 3, 4, 5, 2)

    def forward(self, feature_map):
        """-> (cls_map, reg_map), then dir_map for a head with a direction classifier, then iou_map for one with cfg.IOU_HEAD."""
        if not self.training and not torch.is_grad_enabled() and feature_map.is_cuda:
            maps = self.native_head(feature_map)  # inference on the GPU: csrc/dense_conv.hip, not MIOpen
            return self.maps_from_fused(maps) + tuple(m for m in self.extra_from_fused(maps) if m is not None)
        out = self.reshape_cls(self.conv_cls(feature_map)), self.reshape_reg(self.conv_reg(feature_map))
        if self.direction["ENABLED"]:
            out += (self.reshape_cls(self.conv_dir(feature_map)),)
        if self.iou_head["ENABLED"]:
            out += (self.reshape_cls(self.conv_iou(feature_map)),)
        return out

    def fuse(self, cls_map, reg_map, *extra):
        """The module outputs back in the fused layout [cls | reg (| dir) (| iou)] (B, n_anchor * (8 + groups), H, W), fp32 and
        contiguous: what maps_from_fused / dir_from_fused / iou_from_fused split and the native loss reads.  extra: the maps `forward`
        returns behind the first two, in its order."""
        B, _, _, H, W = cls_map.shape
        parts = [cls_map.reshape(B, -1, H, W), reg_map.permute(0, 1, 5, 2, 3, 4).reshape(B, -1, H, W)]
        for m in extra:
            if m is not None:
                parts.append(m.reshape(B, -1, H, W))
        return torch.cat([p.float() for p in parts], 1)

    def native_head(self, feature_map):
        """fp32 (B, C_IN, H, W) cuda -> fused [cls | reg] maps (B, n_anchor * (1 + DOF), H, W) fp32 on the streaming split-precision
        MFMA 1x1 kernel (csrc/dense_conv.hip:conv1x1_bf16x3_small_cout_kernel) in f16s arithmetic -- the input's scale entry is
        taken from the tensor's own maximum per call, so nothing can leave the range --; the packed weight image is cached until a
        head tensor changes.  (Second's inference paths get the same maps from DenseHeadPlan, which feeds the kernel split planes
        directly; this entry is for callers that hold an fp32 feature map: PV_RCNN.proposal, `model.head(features)`.)"""
        from ..runtime import conv2d_split, pack_conv_weight, to_split_nhwc
        convs = fused_convs(self)

        def build():
            with torch.no_grad():
                w = torch.cat([c.weight for c in convs], 0)
                bias = torch.cat([c.bias for c in convs], 0).float().contiguous()
                return pack_conv_weight(w, None, "fp32"), bias, w.shape[1], w.shape[0]
        img, bias, cin, cout = cached(self, "_native_head", (t for c in convs for t in (c.weight, c.bias)), build)
        hi, lo = to_split_nhwc(feature_map.float(), "fp32")
        return conv2d_split(hi, lo, img, bias, False, cin, cout, 1, out_split=False, out_nchw=True, pr=(hi.v3d_entry, None, None))[1]


class FusedProposalLossFunction(torch.autograd.Function):
    """ProposalLoss.forward and its gradient with respect to the fused head maps in one native pass (csrc/proposal_loss.hip):
    (maps, G_cls int8, M_cls, G_reg, M_reg) -> (cls_loss, reg_loss).  The gradient is computed with the forward; backward scales
    its two channel groups with the upstream gradients."""

    @staticmethod
    def forward(ctx, maps, g_cls, m_cls, g_reg, m_reg, n_cls, n_yaw, alpha, gamma):
        from .. import _lib as L
        b, _, h, w = maps.shape
        losses = torch.empty(3, dtype=torch.float32, device=maps.device)
        dmaps = torch.empty_like(maps)
        lib = L.lib()
        ws = L.workspace(lib.v3d_proposal_loss_workspace(), maps.device)
        with L.device_guard(maps.device):
            L.check(lib.v3d_proposal_loss_fwd_bwd(L.ptr(maps), L.ptr(g_cls), L.ptr(m_cls), L.ptr(g_reg), L.ptr(m_reg), b, n_cls, n_yaw, h, w,
                                                  float(alpha), float(gamma), L.ptr(losses), L.ptr(dmaps), L.ptr(ws), ws.numel(),
                                                  L.stream_ptr()), "proposal_loss_fwd_bwd")
        ctx.grad, ctx.geom = dmaps, (b, n_cls, n_yaw, h, w)
        return losses[0], losses[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_cls_loss, g_reg_loss):
        dmaps = take_gradient(ctx, "proposal")
        scale_gradient("proposal_loss_scale", dmaps, (dmaps, *ctx.geom), (g_cls_loss, g_reg_loss))
        return (dmaps,) + (None,) * 8


class FusedProposalDirLossFunction(torch.autograd.Function):
    """The same for a head with a direction classifier (cfg.DIRECTION; v3d_proposal_dir_loss_fwd_bwd): (maps [cls | reg | dir], G_cls,
    M_cls, G_reg, M_reg, G_dir int8) -> (cls_loss, reg_loss, dir_loss); backward scales the three channel groups with their upstream
    gradients."""

    @staticmethod
    def forward(ctx, maps, g_cls, m_cls, g_reg, m_reg, g_dir, sin_yaw, n_cls, n_yaw, alpha, gamma):
        from .. import _lib as L
        b, _, h, w = maps.shape
        losses = torch.empty(4, dtype=torch.float32, device=maps.device)
        dmaps = torch.empty_like(maps)
        lib = L.lib()
        ws = L.workspace(lib.v3d_proposal_dir_loss_workspace(), maps.device)
        with L.device_guard(maps.device):
            L.check(lib.v3d_proposal_dir_loss_fwd_bwd(L.ptr(maps), L.ptr(g_cls), L.ptr(m_cls), L.ptr(g_reg), L.ptr(m_reg), L.ptr(g_dir),
                                                      int(bool(sin_yaw)), b, n_cls, n_yaw, h, w, float(alpha), float(gamma), L.ptr(losses),
                                                      L.ptr(dmaps), L.ptr(ws), ws.numel(), L.stream_ptr()), "proposal_dir_loss_fwd_bwd")
        ctx.grad, ctx.geom = dmaps, (b, n_cls, n_yaw, h, w)
        return losses[0], losses[1], losses[2]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_cls_loss, g_reg_loss, g_dir_loss):
        dmaps = take_gradient(ctx, "proposal")
        # (the fourth scalar is the 1.0f the two-way scale kernel multiplies the other groups with: csrc/proposal_loss.hip)
        scale_gradient("proposal_dir_loss_scale", dmaps, (dmaps, *ctx.geom), (g_cls_loss, g_reg_loss, g_dir_loss, torch.ones_like(g_cls_loss)))
        return (dmaps,) + (None,) * 10


class FusedProposalIoULossFunction(torch.autograd.Function):
    """The same for a head with an IoU-aware confidence logit (cfg.IOU_HEAD; v3d_proposal_iou_loss_fwd_bwd): (maps [cls | reg | (dir) |
    iou], anchors, G_cls, M_cls, G_reg, M_reg, G_dir int8 or None) -> (cls_loss, reg_loss, dir_loss (0 without the group), iou_loss,
    iou_target or None).  The IoU target is computed inside the pass from the box channels and is a constant: no gradient reaches
    them through it.  backward scales the four (three) channel groups with their upstream gradients."""

    @staticmethod
    def forward(ctx, maps, anchors, g_cls, m_cls, g_reg, m_reg, g_dir, sin_yaw, n_cls, n_yaw, alpha, gamma, want_target=False):
        from .. import _lib as L
        b, _, h, w = maps.shape
        losses = torch.empty(5, dtype=torch.float32, device=maps.device)
        dmaps = torch.empty_like(maps)
        target = torch.empty((b, n_cls, n_yaw, h, w), dtype=torch.float32, device=maps.device) if want_target else None
        lib = L.lib()
        ws = L.workspace(lib.v3d_proposal_iou_loss_workspace(), maps.device)
        with L.device_guard(maps.device):
            L.check(lib.v3d_proposal_iou_loss_fwd_bwd(L.ptr(maps), L.ptr(anchors), L.ptr(g_cls), L.ptr(m_cls), L.ptr(g_reg), L.ptr(m_reg),
                                                      L.ptr(g_dir), int(bool(sin_yaw)), b, n_cls, n_yaw, h, w, float(alpha), float(gamma),
                                                      L.ptr(losses), L.ptr(dmaps), L.ptr(target), L.ptr(ws), ws.numel(), L.stream_ptr()),
                    "proposal_iou_loss_fwd_bwd")
        ctx.grad, ctx.geom, ctx.with_dir = dmaps, (b, n_cls, n_yaw, h, w), g_dir is not None
        if target is not None:
            ctx.mark_non_differentiable(target)
        return losses[0], losses[1], losses[2], losses[3], target

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_cls_loss, g_reg_loss, g_dir_loss, g_iou_loss, _g_target=None):
        from .. import _lib as L
        dmaps = take_gradient(ctx, "proposal")
        # (the last scalar is the 1.0f the two-way scale kernel multiplies the other groups with: csrc/proposal_loss.hip)
        up = [g.to(torch.float32).contiguous() for g in (g_cls_loss, g_reg_loss, g_dir_loss, g_iou_loss, torch.ones_like(g_cls_loss))]
        with L.device_guard(dmaps.device):
            L.check(L.lib().v3d_proposal_iou_loss_scale(L.ptr(dmaps), *ctx.geom, L.ptr(up[0]), L.ptr(up[1]), L.ptr(up[2]) if ctx.with_dir else 0,
                                                        L.ptr(up[3]), L.ptr(up[4]), L.stream_ptr()), "proposal_iou_loss_scale")
        return (dmaps,) + (None,) * 12


class ProposalLoss(nn.Module):
    """Focal classification + smooth-L1 box loss, both divided by max(#positives, 1)
    (proposal.py:100-141).  (P, G, M) = (predicted, ground truth, mask).  With cfg.DIRECTION.ENABLED: the yaw column's smooth-L1
    argument is sin(P_yaw - G_yaw) (SIN_YAW) and dir_loss = BCE-with-logits(P_dir, G_dir) over M_reg / max(#positives, 1) joins the
    sum times LOSS_WEIGHT.  With cfg.IOU_HEAD.ENABLED: iou_loss = soft-target BCE-with-logits(P_iou, iou_targets) over M_reg /
    max(#positives, 1) joins the sum times its LOSS_WEIGHT; the target is detached."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.direction = direction_config(cfg)
        self.iou_head = checked_iou_head(cfg)

    @staticmethod
    def masked_sum(loss, mask):
        return (loss * mask.type_as(loss)).sum()

    def reg_loss(self, P_reg, G_reg, M_reg):
        per = F.smooth_l1_loss(P_reg, G_reg, reduction="none")
        yaw = per[..., 6:7]
        if self.direction["ENABLED"] and self.direction["SIN_YAW"]:
            s = torch.sin(P_reg[..., 6:7] - G_reg[..., 6:7])
            yaw = F.smooth_l1_loss(s, torch.zeros_like(s), reduction="none")
        total = per[..., 0:3] + per[..., 3:6] + yaw / math.pi
        return self.masked_sum(total, M_reg)

    def dir_loss(self, P_dir, G_dir, M_reg):
        x, g = P_dir, G_dir.to(P_dir.dtype)
        bce = x.clamp(min=0) - x * g + torch.log1p(torch.exp(-x.abs()))
        return self.masked_sum(bce, M_reg[..., 0])

    def iou_targets(self, item, native=None):
        """The IoU target of cfg.IOU_HEAD in the shape of P_cls: at the M_reg positives t = clamp(IoU3D(P, G), 0, 1) of the boxes decoded
        from P_reg and G_reg relative to the anchor's centre (`relative_boxes`; the raw yaw, also with cfg.DIRECTION: IoU is
        pi-periodic), 0 elsewhere; detached.  The IoU is ops.box_iou3d_aligned on fp32 GPU tensors (native=None: where it applies) and
        its torch statement elsewhere, on the gathered positives."""
        from ..ops.iou_loss import box_iou3d_aligned, box_iou3d_aligned_torch
        P_reg, G_reg, M_reg = item["P_reg"].detach(), item["G_reg"], item["M_reg"]
        mask = M_reg[..., 0].ne(0) if M_reg.dim() == P_reg.dim() else M_reg.ne(0)
        anchors = item["anchors"].to(device=P_reg.device, dtype=P_reg.dtype).reshape((1,) + tuple(P_reg.shape[1:])).expand_as(P_reg)
        p = relative_boxes(P_reg[mask], anchors[mask])
        g = relative_boxes(G_reg.to(P_reg.dtype)[mask], anchors[mask])
        if native is None:
            native = p.is_cuda and p.dtype == torch.float32
        iou = box_iou3d_aligned(p.contiguous(), g.contiguous()) if native else box_iou3d_aligned_torch(p, g)
        target = torch.zeros(mask.shape, dtype=P_reg.dtype, device=P_reg.device)
        target[mask] = iou.clamp(0, 1)
        return target

    def iou_loss(self, P_iou, target, M_reg):
        z, t = P_iou, target.to(P_iou.dtype)
        bce = z.clamp(min=0) - z * t + torch.log1p(torch.exp(-z.abs()))
        return self.masked_sum(bce, M_reg[..., 0])

    def cls_loss(self, P_cls, G_cls, M_cls):
        # (float64 logits keep float64 targets: torch's BCE takes the dtype of its TARGET, so fp32 targets made the float64 statement fp32)
        target = G_cls.double() if P_cls.dtype == torch.float64 else G_cls.float()
        return self.masked_sum(sigmoid_focal_loss(P_cls, target, reduction="none"), M_cls)

    def _fused(self, item):
        """The native pass applies when the model left its FUSED head maps in the item (`_head_maps`: Second.forward on the native
        training path) and the targets have the assigner's layout; else None and the torch expressions below run."""
        maps = item.get("_head_maps")
        if isinstance(maps, tuple):
            # (maps, P_cls, P_reg) as Second.forward leaves them: the fused maps only speak for this item while its P_cls / P_reg
            # are still the views made from them -- outputs that were replaced or post-processed go through the torch expressions
            maps, p_cls, p_reg, *extra = maps
            keys = [k for k, on in (("P_dir", self.direction["ENABLED"]), ("P_iou", self.iou_head["ENABLED"])) if on]
            if item.get("P_cls") is not p_cls or item.get("P_reg") is not p_reg or len(extra) != len(keys) \
                    or any(item.get(k) is not m for k, m in zip(keys, extra)):
                return None
        cfg = self.cfg
        with_dir, with_iou = bool(self.direction["ENABLED"]), bool(self.iou_head["ENABLED"])
        if maps is None or not maps.is_cuda or maps.dtype != torch.float32 or not maps.is_contiguous() or cfg.BOX_DOF != 7:
            return None
        G_cls, M_cls, G_reg, M_reg = (item[k] for k in ("G_cls", "M_cls", "G_reg", "M_reg"))
        b, o, h, w = maps.shape
        n_cls, n_yaw = cfg.NUM_CLASSES, cfg.NUM_YAW
        shape = (b, n_cls, n_yaw, h, w)
        if o != n_cls * n_yaw * (8 + with_dir + with_iou) or tuple(G_cls.shape) != shape or tuple(M_cls.shape) != shape \
                or tuple(G_reg.shape) != shape + (7,) or tuple(M_reg.shape) != shape + (1,) or G_reg.dtype != torch.float32:
            return None
        if any(t.device != maps.device for t in (G_cls, M_cls, G_reg, M_reg)):
            return None
        g_cls = G_cls if G_cls.dtype == torch.int8 else G_cls.to(torch.int8)
        as_u8 = lambda m: (m if m.dtype in (torch.bool, torch.uint8) else m.ne(0)).contiguous().view(torch.uint8)
        g_dir = None
        if with_dir:
            G_dir = item["G_dir"]
            if tuple(G_dir.shape) != shape or G_dir.device != maps.device:
                return None
            g_dir = (G_dir if G_dir.dtype == torch.int8 else G_dir.to(torch.int8)).contiguous()
        if with_iou:
            anchors = item.get("anchors")
            if not torch.is_tensor(anchors) or anchors.device != maps.device or anchors.dtype != torch.float32 \
                    or anchors.numel() != n_cls * n_yaw * h * w * 7:
                return None
            cls_loss, reg_loss, dir_loss, iou_loss, _ = FusedProposalIoULossFunction.apply(
                maps, anchors.contiguous(), g_cls.contiguous(), as_u8(M_cls), G_reg.contiguous(), as_u8(M_reg), g_dir,
                bool(self.direction["SIN_YAW"]), n_cls, n_yaw, 0.25, 2.0)
            return self._total(cls_loss, reg_loss, dir_loss if with_dir else None, iou_loss)
        if with_dir:
            cls_loss, reg_loss, dir_loss = FusedProposalDirLossFunction.apply(
                maps, g_cls.contiguous(), as_u8(M_cls), G_reg.contiguous(), as_u8(M_reg), g_dir.contiguous(), bool(self.direction["SIN_YAW"]),
                n_cls, n_yaw, 0.25, 2.0)
            return self._total(cls_loss, reg_loss, dir_loss)
        cls_loss, reg_loss = FusedProposalLossFunction.apply(maps, g_cls.contiguous(), as_u8(M_cls), G_reg.contiguous(), as_u8(M_reg),
                                                             n_cls, n_yaw, 0.25, 2.0)
        return dict(cls_loss=cls_loss, reg_loss=reg_loss, loss=cls_loss + self.cfg.TRAIN.LAMBDA * reg_loss)

    def _total(self, cls_loss, reg_loss, dir_loss, iou_loss=None):
        out = dict(cls_loss=cls_loss, reg_loss=reg_loss)
        loss = cls_loss + self.cfg.TRAIN.LAMBDA * reg_loss
        if dir_loss is not None:
            out["dir_loss"] = dir_loss
            loss = loss + self.direction["LOSS_WEIGHT"] * dir_loss
        if iou_loss is not None:
            out["iou_loss"] = iou_loss
            loss = loss + self.iou_head["LOSS_WEIGHT"] * iou_loss
        out["loss"] = loss
        return out

    def forward(self, item):
        fused = self._fused(item)
        if fused is not None:
            return fused
        G_cls, M_cls, P_cls, G_reg, M_reg, P_reg = (item[k] for k in ("G_cls", "M_cls", "P_cls", "G_reg", "M_reg", "P_reg"))
        normalizer = M_reg.type_as(P_reg).sum().clamp_(min=1)
        cls_loss = self.cls_loss(P_cls, G_cls, M_cls) / normalizer
        reg_loss = self.reg_loss(P_reg, G_reg, M_reg) / normalizer
        if self.direction["ENABLED"] or self.iou_head["ENABLED"]:
            dir_loss = self.dir_loss(item["P_dir"], item["G_dir"], M_reg) / normalizer if self.direction["ENABLED"] else None
            iou_loss = self.iou_loss(item["P_iou"], self.iou_targets(item), M_reg) / normalizer if self.iou_head["ENABLED"] else None
            return self._total(cls_loss, reg_loss, dir_loss, iou_loss)
        return dict(cls_loss=cls_loss, reg_loss=reg_loss, loss=cls_loss + self.cfg.TRAIN.LAMBDA * reg_loss)

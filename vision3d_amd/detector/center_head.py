"""Anchor-free centre heatmap head for SECOND (CenterPoint, arXiv 2006.11275; stage 1 of PV-RCNN++), opt-in: cfg.CENTERHEAD.

No upstream counterpart; the definition is this repository's (restated in float64 by tests/center_head_ref.py).
CenterHead: two 1x1 convolutions over the RPN map -> fused maps (B, n_cls + 8, H, W): channels [0, n_cls) heat logits, n_cls + j for
j = 0..7 = dx, dy, z, log w, log l, log h, sin yaw, cos yaw, raw.  Inference = peaks of the heat logits (>= the up to eight in-map
neighbours), the PROPOSAL.TOPK highest per (frame, class), box decode, then the tail of ProposalLayer unchanged: rotated NMS per
(frame, class) at CENTERHEAD.NMS_IOU and the per-class score threshold of cfg.ANCHORS.  Targets: core/center_targets.py; CenterLoss
below.  The native calls live in csrc/center_head.hip; the torch statements beside them (decode_torch, the loss expression) are the
on-device cross-check and the path beyond the native limits or on CPU tensors.
"""
import math

import torch
import torch.nn.functional as F
from torch import nn

from .. import _lib as L
from ..ops import batched_nms_rotated_padded
from .fused_loss import scale_gradient, take_gradient
from .proposal import ProposalLayer, _raise_on_flag

CENTERHEAD_DEFAULTS = dict(ENABLED=False, MIN_OVERLAP=0.1, MIN_RADIUS=2, FOCAL_ALPHA=2.0, FOCAL_BETA=4.0, CODE_WEIGHTS=[1.0] * 8,
                           NMS_IOU=0.01)
MAX_OBJ = 128  # objects per frame of the target / loss tensors (csrc/center_head.hip CH_MAX_OBJ)
MAX_FRAMES, MAX_CLS, MAX_TOPK, MAX_CELLS = 64, 8, 1024, 1 << 24  # the native limits


def centerhead_config(cfg):
    """-> the keys of cfg.CENTERHEAD over their defaults (a config written before the key existed means "disabled")."""
    out = dict(CENTERHEAD_DEFAULTS)
    out.update(cfg.get("CENTERHEAD") or {})
    return out


def centerhead_enabled(cfg):
    return bool(centerhead_config(cfg)["ENABLED"])


def refuse_centerhead(cfg, what):
    """The entry points that do not know the centre head yet (follow-ups) say so instead of building an anchor head beside it."""
    if centerhead_enabled(cfg):
        raise ValueError(f"cfg.CENTERHEAD.ENABLED: {what} does not support the centre heatmap head yet (Second.inference / "
                         "inference_points / forward do)")


def center_geometry(cfg):
    """-> (px, py, x_lo, y_lo) as Python floats, (H, W): the map of AnchorGenerator.compute_grid_params."""
    import types
    from ..core.anchor_generator import AnchorGenerator
    stride = cfg.STRIDES[-1]
    px, py = float(cfg.VOXEL_SIZE[0] * stride), float(cfg.VOXEL_SIZE[1] * stride)
    _, _, (nx, ny) = AnchorGenerator.compute_grid_params(types.SimpleNamespace(cfg=cfg))  # (the method reads nothing but self.cfg)
    return (px, py, float(cfg.GRID_BOUNDS[0]), float(cfg.GRID_BOUNDS[1])), (int(ny), int(nx))


def _host_f64(values):
    import ctypes
    return (ctypes.c_double * len(values))(*[float(v) for v in values])


def center_decode(maps, n_cls, geom, topk):
    """v3d_center_decode: fused maps (B, n_cls + 8, H, W) fp32 cuda -> boxes (B, n_cls * topk, 7), scores (B, n_cls * topk); two
    launches, no host read (capturable)."""
    L.require_gpu("center_decode", maps)
    maps = L.as_f32("center_decode", maps)
    B, O, H, W = maps.shape
    if O != n_cls + 8:
        raise RuntimeError("center_decode: the maps do not have n_cls + 8 channels")
    boxes = torch.empty((B, n_cls * topk, 7), dtype=torch.float32, device=maps.device)
    scores = torch.empty((B, n_cls * topk), dtype=torch.float32, device=maps.device)
    lib = L.lib()
    ws = L.workspace(lib.v3d_center_decode_workspace(B, n_cls, H, W), maps.device)
    with L.device_guard(maps.device):
        L.check(lib.v3d_center_decode(L.ptr(maps), B, n_cls, H, W, _host_f64(geom), int(topk), L.ptr(boxes), L.ptr(scores), L.ptr(ws),
                                      ws.numel(), L.stream_ptr()), "center_decode")
    return boxes, scores


class CenterHead(nn.Module):

    def __init__(self, cfg):
        super().__init__()
        from .keypoint_weighting import pkw_config
        from .voxel_roi_pool import voxelpool_config
        if pkw_config(cfg)["ENABLED"] or voxelpool_config(cfg)["ENABLED"]:
            raise ValueError("cfg.CENTERHEAD.ENABLED with cfg.PKW.ENABLED or cfg.VOXELPOOL.ENABLED: both belong to PV_RCNN, which does "
                             "not take the centre head yet")
        from .proposal import refuse_direction
        refuse_direction(cfg, "the centre heatmap head (cfg.CENTERHEAD.ENABLED regresses sin / cos of the yaw itself)")
        from .proposal import refuse_iou_head
        refuse_iou_head(cfg, "the centre heatmap head (cfg.CENTERHEAD.ENABLED has no anchors to rate)")
        from .proposal import refuse_box_voting
        refuse_box_voting(cfg, "the centre heatmap head (cfg.CENTERHEAD.ENABLED decodes through its own fused NMS)")
        self.cfg = cfg
        self.opt = centerhead_config(cfg)
        if len(self.opt["CODE_WEIGHTS"]) != 8:
            raise ValueError("cfg.CENTERHEAD.CODE_WEIGHTS has one weight per regression channel: 8")
        self.n_cls, self.TOPK = int(cfg.NUM_CLASSES), int(cfg.PROPOSAL.TOPK)
        # the attribute names of ProposalLayer on purpose: runtime.DenseHeadPlan and ProposalLayer.native_head fuse conv_cls | conv_reg
        self.conv_cls = nn.Conv2d(cfg.PROPOSAL.C_IN, self.n_cls, 1)
        self.conv_reg = nn.Conv2d(cfg.PROPOSAL.C_IN, 8, 1)
        self.geom, self.map_shape = center_geometry(cfg)
        self._init_weights()

    def _init_weights(self):
        nn.init.constant_(self.conv_cls.bias, -math.log((1 - 0.1) / 0.1))
        nn.init.constant_(self.conv_reg.bias, 0)
        nn.init.normal_(self.conv_cls.weight, std=0.01)
        nn.init.normal_(self.conv_reg.weight, std=0.01)

    # ---- maps
    def maps_from_fused(self, maps):
        """(B, n_cls + 8, H, W) = [heat | reg] channels of the fused 1x1 head -> (heat logits (B, n_cls, H, W), reg (B, 8, H, W)): views."""
        return maps[:, :self.n_cls], maps[:, self.n_cls:]

    native_head = ProposalLayer.native_head  # the streaming 1x1 kernel on conv_cls | conv_reg, weight image cached per module

    def forward(self, feature_map):
        if not self.training and not torch.is_grad_enabled() and feature_map.is_cuda:
            return self.maps_from_fused(self.native_head(feature_map))  # inference on the GPU: csrc/dense_conv.hip, not MIOpen
        return self.conv_cls(feature_map), self.conv_reg(feature_map)

    @staticmethod
    def fuse(heat, reg):
        return torch.cat((heat, reg), 1)

    # ---- decode
    def native_supported(self, maps):
        B, _, H, W = maps.shape
        return (maps.is_cuda and maps.dtype == torch.float32 and B <= MAX_FRAMES and self.n_cls <= MAX_CLS and self.TOPK <= MAX_TOPK
                and H * W <= MAX_CELLS)

    def decode(self, maps):
        """Fused maps -> (boxes (B, n_cls * TOPK, 7), scores (B, n_cls * TOPK)) in the layout of ProposalLayer.native_topk: native
        (csrc/center_head.hip) on the GPU within its limits, else the torch statements."""
        if not self.native_supported(maps):
            return self.decode_torch(maps)
        return center_decode(maps, self.n_cls, self.geom, self.TOPK)

    def decode_torch(self, maps):
        """The same definition op by op (any device).  The top-k is a stable descending sort, so that ties go to the lower cell."""
        px, py, x_lo, y_lo = self.geom
        maps = maps.float()
        B, _, H, W = maps.shape
        logits, reg = maps[:, :self.n_cls], maps[:, self.n_cls:].reshape(B, 1, 8, H * W)
        peak = logits >= F.max_pool2d(logits, 3, 1, 1)
        masked = torch.where(peak, logits, logits.new_tensor(-math.inf)).reshape(B, self.n_cls, H * W)
        if H * W < self.TOPK:
            masked = F.pad(masked, (0, self.TOPK - H * W), value=-math.inf)
        top, cell = masked.sort(dim=-1, descending=True, stable=True)
        top, cell = top[..., :self.TOPK], cell[..., :self.TOPK]
        real = top > -math.inf
        cell = torch.where(real, cell, torch.zeros_like(cell))
        r = reg.expand(B, self.n_cls, 8, H * W).gather(3, cell[:, :, None, :].expand(-1, -1, 8, -1))
        ix, iy = (cell % W).to(r.dtype), (cell // W).to(r.dtype)
        boxes = torch.stack(((ix + r[:, :, 0]) * px + x_lo, (iy + r[:, :, 1]) * py + y_lo, r[:, :, 2], r[:, :, 3].exp(), r[:, :, 4].exp(),
                             r[:, :, 5].exp(), torch.atan2(r[:, :, 6], r[:, :, 7])), -1)
        boxes = torch.where(real[..., None], boxes, torch.zeros_like(boxes))
        scores = torch.where(real, top.sigmoid(), torch.zeros_like(top))
        return boxes.reshape(B, self.n_cls * self.TOPK, 7), scores.reshape(B, self.n_cls * self.TOPK)

    # ---- tail (that of ProposalLayer)
    _generate_group_idx = ProposalLayer._generate_group_idx
    _above_score_thresh = ProposalLayer._above_score_thresh
    finalize = ProposalLayer.finalize

    def proposals_padded(self, maps):
        """Decode + NMS with no host synchronisation (capturable): the B * n_cls * TOPK candidates (boxes, batch_idx, class_idx, scores)
        plus (keep padded, n_keep) on the device; `finalize` does the variable-length selection.  Pad slots (score 0) sort last in their
        group, so they suppress no real box, and fall to the strict score cut."""
        boxes, scores = self.decode(maps)
        B = boxes.shape[0]
        boxes, scores = boxes.reshape(-1, 7), scores.reshape(-1)
        batch_idx, class_idx, group_idx = self._generate_group_idx(B, self.n_cls, scores.device)
        bev = torch.stack((boxes[:, 0], boxes[:, 1], boxes[:, 3], boxes[:, 4], boxes[:, 6]), dim=1)
        keep, n_keep = batched_nms_rotated_padded(bev, scores, group_idx, float(self.opt["NMS_IOU"]))
        return boxes, batch_idx, class_idx, scores, keep, n_keep

    def inference_native(self, maps, anchors=None, overflow_flag=None):
        """Fused maps -> (boxes (K, 7), batch_idx, class_idx, scores).  One host read: the NMS count and, with it, the plan's flag word."""
        boxes, batch_idx, class_idx, scores, keep, n_keep = self.proposals_padded(maps)
        if overflow_flag is not None and n_keep.is_cuda:
            pair = torch.cat((n_keep.reshape(-1)[:1].to(torch.int32), overflow_flag.reshape(-1)[:1].to(torch.int32))).tolist()
            _raise_on_flag(pair[1])
            n = pair[0]
        else:
            if overflow_flag is not None:
                _raise_on_flag(int(overflow_flag.item()))
            n = int(n_keep.item())
        keep = keep[:n]
        boxes, batch_idx, class_idx, scores = (x[keep] for x in (boxes, batch_idx, class_idx, scores))
        mask = self._above_score_thresh(scores, class_idx)
        return [x[mask] for x in (boxes, batch_idx, class_idx, scores)]

    def inference(self, feature_map, anchors=None):
        heat, reg = self(feature_map)
        return self.inference_native(self.fuse(heat, reg))


class FusedCenterLossFunction(torch.autograd.Function):
    """CenterLoss and its gradient with respect to the fused maps in one native pass (csrc/center_head.hip): the gradient is computed
    with the forward; backward scales its two channel groups with the upstream gradients."""

    @staticmethod
    def forward(ctx, maps, heat, ind, mask, reg, n_cls, alpha, beta, code_weights):
        b, _, h, w = maps.shape
        losses = torch.empty(3, dtype=torch.float32, device=maps.device)
        dmaps = torch.empty_like(maps)
        lib = L.lib()
        ws = L.workspace(lib.v3d_center_loss_workspace(), maps.device)
        with L.device_guard(maps.device):
            L.check(lib.v3d_center_loss_fwd_bwd(L.ptr(maps), L.ptr(heat), L.ptr(ind), L.ptr(mask), L.ptr(reg), b, n_cls, h, w, float(alpha),
                                                float(beta), L.host_f32(code_weights), L.ptr(losses), L.ptr(dmaps), L.ptr(ws), ws.numel(),
                                                L.stream_ptr()), "center_loss_fwd_bwd")
        ctx.grad, ctx.geom = dmaps, (b, n_cls, h, w)
        return losses[0], losses[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_hm, g_reg):
        dmaps = take_gradient(ctx, "centre")
        scale_gradient("center_loss_scale", dmaps, (dmaps, *ctx.geom), (g_hm, g_reg))
        return (dmaps,) + (None,) * 8


def center_loss_fused(maps, heat, ind, mask, reg, n_cls, alpha=2.0, beta=4.0, code_weights=(1.0,) * 8):
    """-> (hm_loss, reg_loss); differentiable with respect to `maps` (cuda, fp32, contiguous)."""
    return FusedCenterLossFunction.apply(maps, heat, ind, mask, reg, int(n_cls), float(alpha), float(beta), tuple(code_weights))


class CenterLoss(nn.Module):
    """Penalty-reduced focal loss on the heat logits + weighted L1 on the eight regression channels at the objects' cells, both divided
    by max(#masked objects, 1).  Reads P_cls (B, n_cls, H, W), P_reg (B, 8, H, W) and G_heat, G_ind, G_mask, G_creg of the item."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.opt = centerhead_config(cfg)

    def _fused(self, item):
        """The native pass applies when the model left its FUSED head maps in the item and P_cls / P_reg are still the views made from
        them (the identity rule of ProposalLoss._fused); else None and the torch expression runs."""
        maps = item.get("_head_maps")
        if not isinstance(maps, tuple):
            return None
        maps, p_cls, p_reg = maps
        if item.get("P_cls") is not p_cls or item.get("P_reg") is not p_reg:
            return None
        n_cls = int(self.cfg.NUM_CLASSES)
        if not (maps.is_cuda and maps.dtype == torch.float32 and maps.is_contiguous() and maps.dim() == 4 and maps.shape[1] == n_cls + 8):
            return None
        heat, ind, mask, reg = (item[k] for k in ("G_heat", "G_ind", "G_mask", "G_creg"))
        b, _, h, w = maps.shape
        if (b > MAX_FRAMES or n_cls > MAX_CLS or h * w > MAX_CELLS or tuple(heat.shape) != (b, n_cls, h, w)
                or tuple(ind.shape) != (b, MAX_OBJ) or tuple(mask.shape) != (b, MAX_OBJ) or tuple(reg.shape) != (b, MAX_OBJ, 8)
                or heat.dtype != torch.float32 or reg.dtype != torch.float32 or ind.dtype != torch.int32
                or mask.dtype not in (torch.uint8, torch.bool) or any(t.device != maps.device for t in (heat, ind, mask, reg))):
            return None
        hm, rl = center_loss_fused(maps, heat.contiguous(), ind.contiguous(), mask.contiguous().view(torch.uint8), reg.contiguous(),
                                  n_cls, self.opt["FOCAL_ALPHA"], self.opt["FOCAL_BETA"], self.opt["CODE_WEIGHTS"])
        return dict(cls_loss=hm, reg_loss=rl, loss=hm + self.cfg.TRAIN.LAMBDA * rl)

    def forward_torch(self, P_cls, P_reg, heat, ind, mask, reg):
        """The definition as torch statements (autograd gives the gradient; any device)."""
        alpha, beta = float(self.opt["FOCAL_ALPHA"]), float(self.opt["FOCAL_BETA"])
        n = mask.to(P_cls.dtype).sum().clamp(min=1)
        x = P_cls
        log_p, log_q = -F.softplus(-x), -F.softplus(x)  # log p, log(1 - p)
        p, q = torch.sigmoid(x), torch.sigmoid(-x)
        heat = heat.to(x.dtype)
        pos = heat == 1
        terms = torch.where(pos, -q.pow(alpha) * log_p, -(1 - heat).pow(beta) * p.pow(alpha) * log_q)
        hm = terms.sum() / n
        B = P_reg.shape[0]
        m = mask.bool()
        cell = torch.where(m, ind.long(), torch.zeros_like(ind, dtype=torch.long))
        pred = P_reg.reshape(B, 8, -1).gather(2, cell[:, None, :].expand(-1, 8, -1)).transpose(1, 2)  # (B, MAX_OBJ, 8)
        cw = pred.new_tensor([float(v) for v in self.opt["CODE_WEIGHTS"]])
        rl = ((pred - reg.to(pred.dtype)).abs() * cw * m[..., None].to(pred.dtype)).sum() / n
        return dict(cls_loss=hm, reg_loss=rl, loss=hm + self.cfg.TRAIN.LAMBDA * rl)

    def forward(self, item):
        fused = self._fused(item)
        if fused is not None:
            return fused
        return self.forward_torch(item["P_cls"], item["P_reg"], item["G_heat"], item["G_ind"], item["G_mask"], item["G_creg"])

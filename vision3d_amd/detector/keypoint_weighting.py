"""Predicted Keypoint Weighting of PV-RCNN (arXiv 1912.13192, section 3.3), opt-in through `cfg.PKW.ENABLED`.  Upstream hands every
keypoint to RoI-grid pooling with weight 1 (model.py:72-74) and has no statement of the module; the definition is this repository's,
restated in numpy in tests/keypoint_weighting_ref.py:

  KeypointWeighting   a foreground head `MLP([C, *PKW.MLPS, 1])` scores every keypoint; its feature row is multiplied with
                      sigmoid(logit) before RoI-grid pooling.
  KeypointSegLoss     the head's supervision.  Label 1: the keypoint lies inside a ground-truth box (class index >= 0) of its own
                      frame -- the test of `core.geometry.points_in_boxes_mask` with use_z; label 255 (ignored): not 1, but inside
                      such a box with `wlh + PKW.GT_EXTRA_WIDTH` (summed in float32); else 0.
                      keypoint_seg_loss = sum over labels != 255 of sigmoid_focal_loss(logit, label, FOCAL_ALPHA, FOCAL_GAMMA)
                      / max(#label 1, 1); loss = PKW.LOSS_WEIGHT * keypoint_seg_loss.

Inference runs the head's tail and the scaling as one native pass over the point-major keypoint feature matrix, the loss and its
gradient as one native pass (csrc/keypoint_weight.hip); the torch statements are kept beside them as the training path, the
fallback and the cross-check."""
import torch
from torch import nn

from ..ops.focal_loss import sigmoid_focal_loss
from .fused_loss import scale_gradient, take_gradient
from .layers import MLP

PKW_DEFAULTS = dict(ENABLED=False, MLPS=[256], GT_EXTRA_WIDTH=[0.2, 0.2, 0.2], FOCAL_ALPHA=0.25, FOCAL_GAMMA=2.0, LOSS_WEIGHT=1.0)
IGNORE = 255


def pkw_config(cfg):
    """-> the keys of cfg.PKW over their defaults (a config written before the key existed means "disabled")."""
    out = dict(PKW_DEFAULTS)
    out.update(cfg.get("PKW") or {})
    return out


def keypoint_weight(hidden, w2, b2, feats_pm):
    """The native tail of the head (v3d_keypoint_weight): hidden (R, H) float32 rows (unit column stride), w2 (H,), b2 (1,) or None,
    feats_pm (R, C) rows with unit column stride, SCALED IN PLACE by sigmoid(hidden @ w2 + b2).  -> logits (R,)."""
    from .. import _lib as L
    L.require_gpu("keypoint_weight", hidden, w2, b2, feats_pm)
    if any(t.dtype != torch.float32 for t in (hidden, w2, feats_pm)) or hidden.dim() != 2 or feats_pm.dim() != 2 \
            or hidden.stride(1) != 1 or feats_pm.stride(1) != 1 or hidden.shape[0] != feats_pm.shape[0] or w2.numel() != hidden.shape[1]:
        raise RuntimeError("keypoint_weight: float32 (R, H) and (R, C) matrices with contiguous columns and H weights")
    rows, h = hidden.shape
    c = feats_pm.shape[1]
    w2 = w2.contiguous()
    logits = torch.empty(rows, dtype=torch.float32, device=feats_pm.device)
    with L.device_guard(feats_pm.device):
        L.check(L.lib().v3d_keypoint_weight(L.ptr(hidden), hidden.stride(0) if rows > 1 else max(hidden.stride(0), h), h, L.ptr(w2),
                                            L.ptr(b2), L.ptr(feats_pm), feats_pm.stride(0) if rows > 1 else max(feats_pm.stride(0), c),
                                            c, rows, L.ptr(logits), L.stream_ptr()), "keypoint_weight")
    return logits


class KeypointWeighting(nn.Module):

    native = True  # False: the torch statements everywhere (the cross-check of the tests)

    def __init__(self, cfg, c_in):
        super().__init__()
        self.cfg = cfg
        hidden = [int(v) for v in pkw_config(cfg)["MLPS"]]
        self.mlp = MLP([int(c_in), *hidden, 1], bias=True, bn=False, relu=[True] * len(hidden) + [False])

    def forward_torch(self, features):
        """features (B, C, K) -> (weighted (B, C, K), logits (B, K)), op by op (any device / dtype, under autograd)."""
        logits = nn.Sequential.forward(self.mlp, features.transpose(1, 2)).squeeze(-1)  # (the torch modules, not MLP's native route)
        return features * torch.sigmoid(logits)[:, None, :], logits

    def native_ok(self, feats_pm):
        """The native pass takes a float32 (B, K, C) view on the GPU with unit channel stride and frames back to back, in eval mode
        without autograd, for a head with ONE hidden layer."""
        lins = [m for m in self.mlp if isinstance(m, nn.Linear)]
        return (self.native and not self.training and not torch.is_grad_enabled() and len(lins) == 2 and feats_pm.is_cuda
                and feats_pm.dtype == torch.float32 and feats_pm.dim() == 3 and feats_pm.numel() > 0 and feats_pm.stride(2) == 1
                and feats_pm.stride(0) == feats_pm.shape[1] * feats_pm.stride(1) and feats_pm.shape[2] % 4 == 0
                and feats_pm.stride(1) % 4 == 0 and feats_pm.data_ptr() % 16 == 0 and lins[0].weight.dtype == torch.float32)

    def _tail(self):
        """(W1^T, b1) as v3d_linear_rows takes them and the last layer as a vector (w2 (H padded), b2 (1,)), cached with MLP._packed."""
        packed = self.mlp._packed()
        cached = self.__dict__.get("_tail_cache")
        if cached is None or cached[0] is not packed:
            (w1, b1, _, _), (w2, b2, _, _) = packed
            cached = self.__dict__["_tail_cache"] = (packed, w1, b1, w2[:, 0].contiguous(), None if b2 is None else b2[:1].contiguous())
        return cached[1:]

    def weight_point_major(self, feats_pm):
        """feats_pm (B, K, C) point-major view (`native_ok`): the hidden layer on v3d_linear_rows, then ONE launch for the last
        layer, the sigmoid and the scaling of the rows IN PLACE.  -> logits (B, K)."""
        from ..pointnet2.pointnet2_utils import linear_rows
        b, k, c = feats_pm.shape
        rows = feats_pm.reshape(b * k, c)  # (a view: the frames are back to back)
        if rows.data_ptr() != feats_pm.data_ptr():
            raise RuntimeError("weight_point_major: feats_pm must be a (B, K, C) view with unit channel stride and frames back to back")
        w1, b1, w2, b2 = self._tail()
        hidden = linear_rows(rows, w1, b1, relu=True)
        return keypoint_weight(hidden, w2, b2, rows).view(b, k)

    def forward(self, features):
        """features (B, C, K) -> (weighted (B, C, K), logits (B, K)); `features` itself is left as it is."""
        pm = features.transpose(1, 2)
        if self.native and not self.training and not torch.is_grad_enabled() and features.is_cuda and features.dtype == torch.float32:
            pm = pm.clone(memory_format=torch.contiguous_format)
            if self.native_ok(pm):
                logits = self.weight_point_major(pm)
                return pm.transpose(1, 2), logits
        return self.forward_torch(features)


# ---- labels
def _frame_lists(boxes, class_idx):
    if torch.is_tensor(boxes):  # one frame handed over without its list
        boxes, class_idx = [boxes], [class_idx]
    return list(boxes), list(class_idx)


def _inside_torch(points, boxes):
    """points (N, 3), boxes (G, 7), float32 -> (N, G) bool: the statements of csrc/pib_device.h (vision3d/core/geometry.py:4-45 in
    numpy's promotions): cos / sin of the float32 yaw, corners and edge tests in float64, the z limits in float32."""
    c, s = boxes[:, 6].cos().double(), boxes[:, 6].sin().double()
    bd = boxes.double()
    ux = torch.tensor([-0.5, 0.5, 0.5, -0.5], dtype=torch.float64, device=boxes.device)
    uy = torch.tensor([-0.5, -0.5, 0.5, 0.5], dtype=torch.float64, device=boxes.device)
    lx, ly = bd[:, 3:4] * ux, bd[:, 4:5] * uy
    cx = (c[:, None] * lx + (-s)[:, None] * ly) + bd[:, 0:1]  # (G, 4)
    cy = (s[:, None] * lx + c[:, None] * ly) + bd[:, 1:2]
    half = boxes[:, 5] / 2
    pz = points[:, 2:3]
    inside = (pz > (boxes[:, 2] - half)[None]) & (pz < (boxes[:, 2] + half)[None])
    px, py = points[:, 0:1].double(), points[:, 1:2].double()
    for v in range(4):
        pv = (v + 3) & 3
        sx, sy = -(cx[:, v] - cx[:, pv]), -(cy[:, v] - cy[:, pv])
        inside = inside & (sx[None] * (cy[None, :, v] - py) - sy[None] * (cx[None, :, v] - px) > 0)
    return inside


def keypoint_labels_torch(keypoints, boxes, class_idx, extra):
    """keypoints (B, K, 3), per-frame boxes (g, 7) / class_idx (g,) -> (B, K) uint8 labels (1 / 255 / 0), op by op on any device.
    Positions and boxes are taken as float32 (the labels are defined on float32 values)."""
    boxes, class_idx = _frame_lists(boxes, class_idx)
    kp = keypoints.detach().to(torch.float32)
    dev = kp.device
    grow = torch.tensor([0.0, 0.0, 0.0, *[float(e) for e in extra], 0.0], dtype=torch.float32, device=dev)
    labels = torch.zeros(kp.shape[:2], dtype=torch.uint8, device=dev)
    for b, (bx, ci) in enumerate(zip(boxes, class_idx)):
        bx = torch.as_tensor(bx).detach().to(dev, torch.float32).reshape(-1, 7)
        bx = bx[torch.as_tensor(ci).to(dev).reshape(-1) >= 0]
        if bx.shape[0] == 0:
            continue
        fg = _inside_torch(kp[b], bx).any(1)
        near = _inside_torch(kp[b], bx + grow).any(1)
        labels[b] = torch.where(fg, 1, torch.where(near, IGNORE, 0)).to(torch.uint8)
    return labels


def _flat_ground_truth(boxes, class_idx, dev):
    """per-frame lists -> (gt (n_gt, 7) f32, gt_class (n_gt) i64, offsets (B + 1) i32) on `dev`, no host synchronisation."""
    boxes, class_idx = _frame_lists(boxes, class_idx)
    offsets = [0]
    for bx in boxes:
        offsets.append(offsets[-1] + int(bx.shape[0]))
    gt = torch.cat([torch.as_tensor(bx).detach().to(dev, torch.float32).reshape(-1, 7) for bx in boxes]).contiguous()
    gt_class = torch.cat([torch.as_tensor(ci).to(dev, torch.int64).reshape(-1) for ci in class_idx]).contiguous()
    if gt_class.numel() != gt.shape[0]:
        raise RuntimeError("keypoint labels: boxes and class_idx disagree")
    return gt, gt_class, torch.tensor(offsets, dtype=torch.int32).to(dev, non_blocking=True)


def _seg_loss_call(keypoints, logits, boxes, class_idx, extra, alpha, gamma):
    """One launch of v3d_keypoint_seg_loss_fwd_bwd.  -> (labels (B, K) u8, losses (3,), d_logits (B, K) or None when logits is None)."""
    from .. import _lib as L
    kp = keypoints.detach().contiguous()
    dev, (b, k) = kp.device, kp.shape[:2]
    if len(_frame_lists(boxes, class_idx)[0]) != b:
        raise RuntimeError("keypoint labels: one ground-truth list entry per frame")
    gt, gt_class, offsets = _flat_ground_truth(boxes, class_idx, dev)
    labels = torch.empty((b, k), dtype=torch.uint8, device=dev)
    losses = torch.empty(3, dtype=torch.float32, device=dev)
    d_logits = None if logits is None else torch.empty((b, k), dtype=torch.float32, device=dev)
    with L.device_guard(dev):
        L.check(L.lib().v3d_keypoint_seg_loss_fwd_bwd(L.ptr(kp), L.ptr(logits), b, k, L.ptr(gt), L.ptr(gt_class), L.ptr(offsets),
                                                      gt.shape[0], L.host_f32(extra), float(alpha), float(gamma), L.ptr(labels),
                                                      L.ptr(losses), L.ptr(d_logits), L.stream_ptr()), "keypoint_seg_loss_fwd_bwd")
    return labels, losses, d_logits


def keypoint_labels(keypoints, boxes, class_idx, extra):
    """(B, K) uint8 labels: one native launch for float32 keypoints on the GPU, else `keypoint_labels_torch`."""
    if keypoints.is_cuda and keypoints.dtype == torch.float32 and keypoints.dim() == 3 and keypoints.shape[-1] == 3:
        return _seg_loss_call(keypoints, None, boxes, class_idx, extra, 0.0, 0.0)[0]
    return keypoint_labels_torch(keypoints, boxes, class_idx, extra)


class FusedKeypointSegLossFunction(torch.autograd.Function):
    """KeypointSegLoss.forward_torch and its gradient in one native pass (csrc/keypoint_weight.hip): logits (B, K) -> the loss; the
    labels and the kernel's (#1, #255) stay on the node as `loss.grad_fn.labels` / `.counts`.  The gradient is computed with the
    forward; backward scales it with the upstream gradient."""

    @staticmethod
    def forward(ctx, logits, keypoints, boxes, class_idx, extra, alpha, gamma):
        labels, losses, d_logits = _seg_loss_call(keypoints, logits.detach().contiguous(), boxes, class_idx, extra, alpha, gamma)
        ctx.grad, ctx.rows = d_logits, logits.numel()
        ctx.labels, ctx.counts = labels, losses[1:3]
        ctx.mark_non_differentiable(labels)
        return losses[0], labels

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_labels):
        grad = take_gradient(ctx, "keypoint segmentation")
        scale_gradient("keypoint_seg_loss_scale", grad, (grad, ctx.rows), (g_loss,))
        return grad, None, None, None, None, None, None


class KeypointSegLoss(nn.Module):
    """The supervision of KeypointWeighting over `K_cls` (B, K) logits, `keypoints` (B, K, 3) and the per-frame `boxes` /
    `class_idx` lists of the item (see the module docstring).  -> dict(loss, keypoint_seg_loss); leaves `K_label` (B, K) uint8."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        pkw = pkw_config(cfg)
        self.extra = tuple(float(v) for v in pkw["GT_EXTRA_WIDTH"])
        self.alpha, self.gamma, self.weight = float(pkw["FOCAL_ALPHA"]), float(pkw["FOCAL_GAMMA"]), float(pkw["LOSS_WEIGHT"])
        if len(self.extra) != 3:
            raise ValueError("PKW.GT_EXTRA_WIDTH must be [dw, dl, dh]")

    def _result(self, seg):
        return dict(loss=self.weight * seg, keypoint_seg_loss=seg)

    def _fused(self, item):
        """The native pass applies to float32 logits and keypoints on one GPU; else None."""
        logits, kp = item["K_cls"], item["keypoints"]
        if not logits.is_cuda or logits.dtype != torch.float32 or kp.dtype != torch.float32 or kp.device != logits.device \
                or kp.dim() != 3 or kp.shape[-1] != 3 or tuple(logits.shape) != tuple(kp.shape[:2]):
            return None
        seg, labels = FusedKeypointSegLossFunction.apply(logits, kp, item["boxes"], item["class_idx"], self.extra, self.alpha, self.gamma)
        item["K_label"] = labels
        return self._result(seg)

    def forward_torch(self, item):
        """The same loss op by op in torch (any device / dtype): the fallback and the cross-check of the native pass."""
        logits = item["K_cls"]
        labels = keypoint_labels_torch(item["keypoints"], item["boxes"], item["class_idx"], self.extra).to(logits.device)
        item["K_label"] = labels
        zero = logits.new_zeros(())
        focal = sigmoid_focal_loss(logits, (labels == 1).type_as(logits), self.alpha, self.gamma)
        seg = torch.where(labels != IGNORE, focal, zero).sum() / (labels == 1).sum().clamp(min=1).type_as(logits)
        return self._result(seg)

    def forward(self, item):
        fused = self._fused(item)
        return fused if fused is not None else self.forward_torch(item)

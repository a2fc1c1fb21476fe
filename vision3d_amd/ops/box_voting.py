"""IoU-weighted box voting behind rotated NMS (cfg.BOX_VOTING; box voting / weighted NMS / the DI-NMS of CIA-SSD; not in the
reference, whose tails stop at greedy NMS).  Definition: DESIGN.md section 7, csrc/box_vote_device.h, tests/box_voting_ref.py.

A group is one (frame, class): boxes (G, T, 7) = (x, y, z, w, l, h, yaw), scores (G, T).  Every candidate k is voted as a centre by the
candidates j of its own group:

    u_j = box_iou_rotated(b_k[0,1,3,4,6], b_j[0,1,3,4,6])       centre first; that operator's bits and angle convention
    j votes iff s_j > 0, b_j finite in all seven components, u_j >= iou_threshold (a NaN is not a member)
    w_j = s_j * u_j,  W = sum of w_j
    out[c] = b_k[c] + sum w_j (b_j[c] - b_k[c]) / W,  c = 0 .. 5  (offsets: a plain weighted mean at 70 m loses three digits in fp32)
    out[6] = yaw_k + sum w_j wrap(yaw_j - yaw_k) / W,  wrap(d) = d - pi * rint(d / pi), pi = float32(pi), round half even
    W not finite or not > 0: out = b_k with its own bits

`box_voting_rotated` is the native op (csrc/box_voting.hip, one launch, no host synchronisation); `box_voting_statement` states the
same op by op in torch, in any dtype, on the IoU matrix of `box_iou_rotated` -- so both make the same membership decisions."""
import numpy as np
import torch

from .. import _lib as L
from .iou_nms import box_iou_rotated

PI32 = float(np.float32(np.pi))  # the pi of the yaw wrap in every statement: the fp32 constant the kernel divides by


def _check(name, boxes, scores):
    if boxes.dim() != 3 or boxes.shape[-1] != 7 or tuple(scores.shape) != tuple(boxes.shape[:2]):
        raise RuntimeError(f"{name}: expected boxes (G, T, 7) and scores (G, T), got {tuple(boxes.shape)} and {tuple(scores.shape)}")


def box_voting_rotated(boxes, scores, iou_threshold):
    """boxes (G, T, 7), scores (G, T) float32 on the GPU -> voted boxes (G, T, 7): every candidate as a centre (module docstring)."""
    L.require_gpu("box_voting_rotated", boxes, scores)
    b, s = L.as_f32("box_voting_rotated", boxes), L.as_f32("box_voting_rotated", scores)
    _check("box_voting_rotated", b, s)
    out = torch.empty_like(b)
    with L.device_guard(b.device):
        L.check(L.lib().v3d_box_voting(L.ptr(b), L.ptr(s), b.shape[0], b.shape[1], float(np.float32(iou_threshold)), L.ptr(out),
                                       L.stream_ptr()), "box_voting_rotated")
    return out


def group_iou(boxes):
    """(G, T, 7) float32 on the GPU -> (G, T, T) float32: u[g, k, j] = box_iou_rotated(centre k, candidate j) inside group g, on the
    unshifted boxes.  One operator call per group; no host-built index tensor (an H2D copy is illegal during graph capture)."""
    b = boxes.float()
    bev = torch.stack((b[..., 0], b[..., 1], b[..., 3], b[..., 4], b[..., 6]), dim=-1)
    if bev.shape[0] == 0:
        return b.new_zeros((0, bev.shape[1], bev.shape[1]))
    return torch.stack([box_iou_rotated(bev[g], bev[g]) for g in range(bev.shape[0])])


def box_voting_statement(boxes, scores, iou_threshold, dtype=None, iou=None):
    """The definition op by op: boxes (G, T, 7), scores (G, T) -> (G, T, 7) in `dtype` (default: the boxes'), every candidate as a
    centre.  iou (G, T, T): u[g, k, j]; None = `group_iou` of the boxes as fp32 (GPU only, like every native op), cast to `dtype`.  The
    threshold is compared as the fp32 number the kernel receives.  No host synchronisation."""
    _check("box_voting_statement", boxes, scores)
    dtype = boxes.dtype if dtype is None else dtype
    u = (group_iou(boxes) if iou is None else iou).to(dtype)
    b, s = boxes.to(dtype), scores.to(dtype)
    member = (s > 0)[:, None, :] & torch.isfinite(b).all(-1)[:, None, :] & (u >= float(np.float32(iou_threshold)))
    w = torch.where(member, s[:, None, :] * u, torch.zeros_like(u))                       # (G, k, j)
    W = w.sum(-1)                                                                         # (G, k)
    off = b[:, None, :, :] - b[:, :, None, :]                                             # (G, k, j, 7): b_j - b_k
    d = off[..., 6]
    off = torch.cat((off[..., :6], (d - PI32 * torch.round(d / PI32))[..., None]), -1)  # (a Python scalar: no H2D copy under capture)
    # (a non-member's offset may be NaN or inf: it is taken out, not multiplied by a zero weight)
    terms = torch.where(member[..., None], w[..., None] * off, torch.zeros_like(off))
    voted = b + terms.sum(2) / W[..., None]
    vote = torch.isfinite(W) & (W > 0)
    return torch.where(vote[..., None], voted, b)

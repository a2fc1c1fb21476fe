"""Targets of the centre heatmap head (cfg.CENTERHEAD; detector/center_head.py): a Gaussian splat per ground-truth box on its class's
heat map and one regression row per box.  The definition is this repository's (tests/center_head_ref.py).

CenterTargetAssigner(cfg)(item) reads the collated item's per-frame lists `boxes` [(n_b, 7) = (x, y, z, w, l, h, yaw)] and `class_idx`
[(n_b,)] and adds G_heat (B, n_cls, H, W) f32, G_ind (B, 128) i32, G_mask (B, 128) u8, G_cls (B, 128) i32, G_creg (B, 128, 8) f32.
On the GPU with at most 128 boxes per frame: one launch of csrc/center_head.hip (v3d_center_targets); `forward_torch` states the
same definition with torch operators -- the on-device cross-check, and the path for CPU tensors and larger frames (where the
per-object tensors grow to the largest frame).
"""
import torch
from torch import nn

from .. import _lib as L

MAX_OBJ = 128


def center_targets(boxes, classes, n_cls, H, W, geom, min_overlap=0.1, min_radius=2):
    """v3d_center_targets: per-frame lists boxes[b] (n_b <= 128, 7) f32 / classes[b] (n_b,) i32 on one GPU, geom = (px, py, x_lo, y_lo)
    -> (heat (B, n_cls, H, W) f32, ind (B, 128) i32, mask (B, 128) u8, cls (B, 128) i32, reg (B, 128, 8) f32).  One launch, no host read."""
    import ctypes
    L.require_gpu("center_targets", *boxes, *classes)
    dev = boxes[0].device
    B = len(boxes)
    offsets = [0]
    for b in boxes:
        offsets.append(offsets[-1] + int(b.shape[0]))
    if offsets[-1]:
        flat = L.as_f32("center_targets", torch.cat([b.reshape(-1, 7) for b in boxes]))
        cls_in = L.as_i32("center_targets", torch.cat([c.reshape(-1) for c in classes]))
    else:
        flat = cls_in = None
    heat = torch.empty((B, n_cls, H, W), dtype=torch.float32, device=dev)
    ind = torch.empty((B, MAX_OBJ), dtype=torch.int32, device=dev)
    mask = torch.empty((B, MAX_OBJ), dtype=torch.uint8, device=dev)
    cls = torch.empty((B, MAX_OBJ), dtype=torch.int32, device=dev)
    reg = torch.empty((B, MAX_OBJ, 8), dtype=torch.float32, device=dev)
    with L.device_guard(dev):
        L.check(L.lib().v3d_center_targets(L.ptr(flat), L.ptr(cls_in), L.host_i32(offsets), B, int(n_cls), int(H), int(W),
                                           (ctypes.c_double * 4)(*[float(v) for v in geom]), float(min_overlap), int(min_radius),
                                           L.ptr(heat), L.ptr(ind), L.ptr(mask), L.ptr(cls), L.ptr(reg), L.stream_ptr()), "center_targets")
    return heat, ind, mask, cls, reg


class CenterTargetAssigner(nn.Module):

    def __init__(self, cfg):
        super().__init__()
        from ..detector.center_head import center_geometry, centerhead_config
        self.cfg = cfg
        self.opt = centerhead_config(cfg)
        self.n_cls = int(cfg.NUM_CLASSES)
        self.geom, (self.H, self.W) = center_geometry(cfg)

    @staticmethod
    def _frames(item):
        boxes = [torch.as_tensor(b, dtype=torch.float32).reshape(-1, 7) for b in item["boxes"]]
        classes = [torch.as_tensor(c).reshape(-1).to(device=b.device, dtype=torch.int32) for b, c in zip(boxes, item["class_idx"])]
        return boxes, classes

    def native_supported(self, boxes):
        return (len(boxes) <= 64 and self.n_cls <= 8 and self.H * self.W <= 1 << 24 and all(b.is_cuda for b in boxes)
                and all(b.shape[0] <= MAX_OBJ for b in boxes) and len(boxes) > 0)

    def forward(self, item):
        boxes, classes = self._frames(item)
        out = self.forward_native(boxes, classes) if self.native_supported(boxes) else self.forward_torch(boxes, classes)
        item.update(dict(zip(("G_heat", "G_ind", "G_mask", "G_cls", "G_creg"), out)))
        return item

    def forward_native(self, boxes, classes):
        """-> (heat, ind, mask, cls, reg): v3d_center_targets, one launch, no host read."""
        return center_targets(boxes, classes, self.n_cls, self.H, self.W, self.geom, self.opt["MIN_OVERLAP"], self.opt["MIN_RADIUS"])

    def forward_torch(self, boxes, classes):
        """The same definition with torch operators on the boxes' device: fp32 where the kernel is fp32, the radius in float64."""
        px, py, x_lo, y_lo = self.geom
        o, H, W, n_cls = float(self.opt["MIN_OVERLAP"]), self.H, self.W, self.n_cls
        B = len(boxes)
        dev = boxes[0].device if B else torch.device("cpu")
        rows = max([MAX_OBJ] + [int(b.shape[0]) for b in boxes])
        heat = torch.zeros((B, n_cls, H, W), dtype=torch.float32, device=dev)
        ind = torch.full((B, rows), -1, dtype=torch.int32, device=dev)
        mask = torch.zeros((B, rows), dtype=torch.uint8, device=dev)
        cls = torch.zeros((B, rows), dtype=torch.int32, device=dev)
        reg = torch.zeros((B, rows, 8), dtype=torch.float32, device=dev)
        vv = torch.arange(H, device=dev).view(1, H, 1)
        uu = torch.arange(W, device=dev).view(1, 1, W)
        for b, (bx, c) in enumerate(zip(boxes, classes)):
            n = bx.shape[0]
            if n == 0:
                continue
            cls[b, :n] = c
            fx, fy = (bx[:, 0] - x_lo) / px, (bx[:, 1] - y_lo) / py
            size_ok = (torch.isfinite(bx[:, 3:6]) & (bx[:, 3:6] > 0)).all(1)
            live = (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H) & (c >= 0) & (c < n_cls) & size_ok
            safe = lambda t: torch.where(live, t, torch.ones_like(t))
            ix, iy = torch.floor(safe(fx)), torch.floor(safe(fy))
            w, l = safe(bx[:, 3]).double(), safe(bx[:, 4]).double()
            a, bb = w / px, l / py
            s = a + bb
            r1 = (s + torch.sqrt(s * s - 4 * a * bb * (1 - o) / (1 + o))) / 2
            r2 = (2 * s + torch.sqrt(4 * s * s - 16 * (1 - o) * a * bb)) / 2
            r3 = (-2 * o * s + torch.sqrt(4 * o * o * s * s + 16 * o * (1 - o) * a * bb)) / 2
            r = torch.minimum(torch.minimum(r1, r2), r3).clamp(max=1048576.0).long().clamp(min=int(self.opt["MIN_RADIUS"]))
            k = (-1.0 / (2 * ((2 * r.double() + 1) / 6) ** 2)).float()
            ixl, iyl = ix.long(), iy.long()
            du, dv = uu - ixl.view(n, 1, 1), vv - iyl.view(n, 1, 1)
            g = torch.exp((du * du + dv * dv).float() * k.view(n, 1, 1))
            inside = (du.abs() <= r.view(n, 1, 1)) & (dv.abs() <= r.view(n, 1, 1)) & live.view(n, 1, 1)
            g = torch.where(inside, g, torch.zeros_like(g))
            for k_cls in range(n_cls):
                sel = live & (c == k_cls)
                if bool(sel.any()):
                    heat[b, k_cls] = g[sel].amax(0)
            ind[b, :n] = torch.where(live, iyl * W + ixl, torch.full_like(ixl, -1)).to(torch.int32)
            mask[b, :n] = live.to(torch.uint8)
            row = torch.stack((fx - ix, fy - iy, bx[:, 2], safe(bx[:, 3]).log(), safe(bx[:, 4]).log(), safe(bx[:, 5]).log(),
                               torch.sin(bx[:, 6]), torch.cos(bx[:, 6])), 1)
            reg[b, :n] = torch.where(live[:, None], row, torch.zeros_like(row))
        return heat, ind, mask, cls, reg

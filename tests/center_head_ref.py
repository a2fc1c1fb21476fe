"""The centre heatmap head (cfg.CENTERHEAD) restated in numpy float64: targets, loss with its gradient, peak decode.  The yardstick of
tests/test_host_center_head.py and tests/test_gpu_center_head.py; written from the definition, with loops where
they are clearer than array expressions -- no torch, no call into the package.

Maps are (B, n_cls + 8, H, W): channels [0, n_cls) heat logits, n_cls + j for j = 0..7 = dx, dy, z, log w, log l, log h, sin yaw, cos yaw.
geom = (px, py, x_lo, y_lo): metres per cell and the grid origin."""
import math

import numpy as np

MAX_OBJ = 128


def radius_roots(w, l, px, py, min_overlap):
    """The three CornerNet roots of an object of w x l metres, in cells."""
    a, b, o = float(w) / px, float(l) / py, float(min_overlap)
    s = a + b
    r1 = (s + math.sqrt(s * s - 4 * a * b * (1 - o) / (1 + o))) / 2
    r2 = (2 * s + math.sqrt(4 * s * s - 16 * (1 - o) * a * b)) / 2
    r3 = (-2 * o * s + math.sqrt(4 * o * o * s * s + 16 * o * (1 - o) * a * b)) / 2
    return r1, r2, r3


def targets(boxes, class_idx, n_cls, H, W, geom, min_overlap=0.1, min_radius=2):
    """boxes[b] (n_b, 7) float32, class_idx[b] (n_b,) -> dict(heat (B, n_cls, H, W), ind / mask / cls (B, 128), reg (B, 128, 8),
    window (B, n_cls, H, W) bool: reached by some window, fmargin: the smallest distance of a live fx / fy from an integer,
    rmargin: the smallest distance of min(r1, r2, r3) from an integer)."""
    px, py, x_lo, y_lo = (float(v) for v in geom)
    B = len(boxes)
    heat = np.zeros((B, n_cls, H, W))
    window = np.zeros((B, n_cls, H, W), bool)
    ind = np.full((B, MAX_OBJ), -1, np.int32)
    mask = np.zeros((B, MAX_OBJ), np.uint8)
    cls = np.zeros((B, MAX_OBJ), np.int32)
    reg = np.zeros((B, MAX_OBJ, 8))
    fmargin = rmargin = np.inf
    for b in range(B):
        bx = np.asarray(boxes[b], np.float32).reshape(-1, 7).astype(np.float64)
        assert len(bx) <= MAX_OBJ
        for i, (x, y, z, w, l, h, yaw) in enumerate(bx):
            c = int(class_idx[b][i])
            cls[b, i] = c
            fx, fy = (x - x_lo) / px, (y - y_lo) / py
            if not (np.isfinite(fx) and np.isfinite(fy)):
                continue
            ix, iy = math.floor(fx), math.floor(fy)
            live = 0 <= ix < W and 0 <= iy < H and 0 <= c < n_cls and all(np.isfinite(v) and v > 0 for v in (w, l, h))
            if not live:
                continue
            rmin = min(radius_roots(w, l, px, py, min_overlap))
            r = max(int(min_radius), int(rmin))
            fmargin = min(fmargin, abs(fx - round(fx)), abs(fy - round(fy)))
            rmargin = min(rmargin, abs(rmin - round(rmin)))
            sigma = (2 * r + 1) / 6
            for v in range(max(iy - r, 0), min(iy + r, H - 1) + 1):
                for u in range(max(ix - r, 0), min(ix + r, W - 1) + 1):
                    g = math.exp(-((u - ix) ** 2 + (v - iy) ** 2) / (2 * sigma * sigma))
                    heat[b, c, v, u] = max(heat[b, c, v, u], g)
                    window[b, c, v, u] = True
            ind[b, i], mask[b, i] = iy * W + ix, 1
            reg[b, i] = [fx - ix, fy - iy, z, math.log(w), math.log(l), math.log(h), math.sin(yaw), math.cos(yaw)]
    return dict(heat=heat, ind=ind, mask=mask, cls=cls, reg=reg, window=window, fmargin=fmargin, rmargin=rmargin)


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def loss(maps, heat, ind, mask, reg, n_cls, alpha=2.0, beta=4.0, code_weights=(1.0,) * 8, lam=1.0):
    """-> dict(hm, reg, n, loss, d_hm, d_reg: gradients of hm / reg with respect to the maps, dmaps: of loss, reg_margin: the smallest
    |pred - target| over the masked components)."""
    maps, heat, reg = np.asarray(maps, np.float64), np.asarray(heat, np.float64), np.asarray(reg, np.float64)
    B, O, H, W = maps.shape
    n = max(int(np.asarray(mask).sum()), 1)
    x = maps[:, :n_cls]
    p = np.where(x >= 0, 1 / (1 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1 + np.exp(-np.abs(x))))
    q = np.where(x >= 0, np.exp(-np.abs(x)) / (1 + np.exp(-np.abs(x))), 1 / (1 + np.exp(-np.abs(x))))
    lp, lq = -softplus(-x), -softplus(x)
    pos = heat == 1
    w = (1 - heat) ** beta
    terms = np.where(pos, -(q ** alpha) * lp, -w * (p ** alpha) * lq)
    grad = np.where(pos, q ** alpha * (alpha * p * lp - q), w * p ** alpha * (p - alpha * q * lq))
    d_hm, d_reg = np.zeros_like(maps), np.zeros_like(maps)
    d_hm[:, :n_cls] = grad / n
    total, margin = 0.0, np.inf
    flat = d_reg.reshape(B, O, H * W)
    pred_flat = maps.reshape(B, O, H * W)
    for b in range(B):
        for i in range(MAX_OBJ):
            if not mask[b, i]:
                continue
            for j in range(8):
                d = pred_flat[b, n_cls + j, ind[b, i]] - reg[b, i, j]
                total += code_weights[j] * abs(d)
                margin = min(margin, abs(d))
                flat[b, n_cls + j, ind[b, i]] += code_weights[j] * np.sign(d) / n
    hm, rl = terms.sum() / n, total / n
    return dict(hm=hm, reg=rl, n=n, loss=hm + lam * rl, d_hm=d_hm, d_reg=d_reg, dmaps=d_hm + lam * d_reg, reg_margin=margin)


def peaks(logits):
    """(H, W) -> bool (H, W): >= each of the up to eight in-map neighbours."""
    H, W = logits.shape
    out = np.ones((H, W), bool)
    for dv in (-1, 0, 1):
        for du in (-1, 0, 1):
            if dv == 0 and du == 0:
                continue
            v0, v1, u0, u1 = max(0, -dv), min(H, H - dv), max(0, -du), min(W, W - du)
            out[v0:v1, u0:u1] &= logits[v0:v1, u0:u1] >= logits[v0 + dv:v1 + dv, u0 + du:u1 + du]
    return out


def decode(maps, n_cls, geom, topk):
    """-> dict(boxes (B, n_cls * topk, 7), scores (B, n_cls * topk), cells (B, n_cls, topk) int64: the selected cell, -1 = pad slot)."""
    px, py, x_lo, y_lo = (float(v) for v in geom)
    maps = np.asarray(maps, np.float64)
    B, O, H, W = maps.shape
    boxes, scores = np.zeros((B, n_cls, topk, 7)), np.zeros((B, n_cls, topk))
    cells = np.full((B, n_cls, topk), -1, np.int64)
    for b in range(B):
        r = maps[b, n_cls:].reshape(8, -1)
        for c in range(n_cls):
            x = maps[b, c]
            idx = np.flatnonzero(peaks(x).reshape(-1))
            order = idx[np.lexsort((idx, -x.reshape(-1)[idx]))][:topk]  # logit descending, ties: cell ascending
            k = len(order)
            cells[b, c, :k] = order
            iy, ix = order // W, order % W
            boxes[b, c, :k] = np.stack([(ix + r[0, order]) * px + x_lo, (iy + r[1, order]) * py + y_lo, r[2, order], np.exp(r[3, order]),
                                        np.exp(r[4, order]), np.exp(r[5, order]), np.arctan2(r[6, order], r[7, order])], 1)
            scores[b, c, :k] = 1 / (1 + np.exp(-x.reshape(-1)[order]))
    return dict(boxes=boxes.reshape(B, n_cls * topk, 7), scores=scores.reshape(B, n_cls * topk), cells=cells)

"""The direction classifier and sine yaw loss of the anchor head (cfg.DIRECTION) restated in plain numpy, float64: the direction bit,
the targets, the decode rule, and the loss with its gradient with respect to the fused [cls | reg | dir] head maps.  No torch, no GPU.

Layouts (those of the C ABI): maps (B, n_anchor * 9, H, W), n_anchor = n_cls * n_yaw -- class channel c * n_yaw + yaw, box channel
n_anchor + (c * 7 + d) * n_yaw + yaw, direction channel n_anchor * 8 + c * n_yaw + yaw; targets (B, n_cls, n_yaw, H, W[, 7 | 1]).
"""
import math

import numpy as np

PI = math.pi
OFFSET = 0.7853981634  # cfg.DIRECTION.OFFSET


def bit(t, offset=OFFSET):
    """floor(remainder(t - offset, 2 pi) / pi) in {0, 1}"""
    return np.floor(np.remainder(np.asarray(t, np.float64) - offset, 2 * PI) / PI).astype(np.int64)


def bin_edge_distance(t, offset=OFFSET):
    """distance of a yaw from the nearest edge of its direction bin (the edges lie at offset + k pi)"""
    r = np.remainder(np.asarray(t, np.float64) - offset, PI)
    return np.minimum(r, PI - r)


def targets(gt_yaw, matches, m_reg, offset=OFFSET):
    """G_dir int8 in the shape of `matches`: bit(yaw of the matched ground truth) where m_reg, else 0"""
    matches, m_reg = np.asarray(matches), np.asarray(m_reg).reshape(np.shape(matches)).astype(bool)
    out = np.zeros(matches.shape, np.int8)
    if m_reg.any():
        out[m_reg] = bit(np.asarray(gt_yaw, np.float64)[matches[m_reg]], offset)
    return out


def decode_yaw(raw, dir_logit, offset=OFFSET):
    """remainder(raw - offset, pi) + offset + pi * [dir_logit > 0]; the comparison is strict (+-0 and NaN give 0)"""
    with np.errstate(invalid="ignore"):
        up = np.asarray(dir_logit) > 0
    return np.remainder(np.asarray(raw, np.float64) - offset, PI) + offset + PI * up


def wrap_argument_distance(raw, offset=OFFSET):
    """distance of the decode rule's wrap argument raw - offset from the nearest multiple of pi"""
    return bin_edge_distance(raw, offset)


def split_maps(maps, n_cls, n_yaw):
    """fused maps -> (P_cls (B, n_cls, n_yaw, H, W), P_reg (..., 7), P_dir like P_cls)"""
    maps = np.asarray(maps)
    B, _, H, W = maps.shape
    na = n_cls * n_yaw
    p_cls = maps[:, :na].reshape(B, n_cls, n_yaw, H, W)
    p_reg = maps[:, na:8 * na].reshape(B, n_cls, 7, n_yaw, H, W).transpose(0, 1, 3, 4, 5, 2)
    p_dir = maps[:, 8 * na:9 * na].reshape(B, n_cls, n_yaw, H, W)
    return p_cls, p_reg, p_dir


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _bce(x, g):
    """max(x, 0) - x g + log1p(exp(-|x|)); gradient sigmoid(x) - g"""
    return np.maximum(x, 0.0) - x * g + np.log1p(np.exp(-np.abs(x)))


def _smooth_l1(d):
    a = np.abs(d)
    return np.where(a < 1.0, 0.5 * d * d, a - 0.5), np.clip(d, -1.0, 1.0)


def loss(maps, G_cls, M_cls, G_reg, M_reg, G_dir, n_cls, n_yaw, sin_yaw=True, lam=1.0, weight=0.2, alpha=0.25, gamma=2.0):
    """-> dict(cls_loss, reg_loss, dir_loss, loss, normalizer, grads=(d cls_loss, d reg_loss, d dir_loss) each in the maps' shape)."""
    maps = np.asarray(maps, np.float64)
    B, _, H, W = maps.shape
    na = n_cls * n_yaw
    p_cls, p_reg, p_dir = split_maps(maps, n_cls, n_yaw)
    m_cls = np.asarray(M_cls).astype(bool)
    pos = np.asarray(M_reg).astype(bool).reshape(m_cls.shape)
    n = max(int(pos.sum()), 1)
    # focal (ops/focal_loss.py)
    t = (np.asarray(G_cls) > 0).astype(np.float64)
    prob = _sigmoid(p_cls)
    bce = _bce(p_cls, t)
    q = 1.0 - (prob * t + (1.0 - prob) * (1.0 - t))
    w = alpha * t + (1.0 - alpha) * (1.0 - t)
    focal = w * bce * q ** gamma
    d_focal = w * ((prob - t) * q ** gamma - bce * gamma * q ** (gamma - 1.0) * prob * (1.0 - prob) * (2.0 * t - 1.0))
    cls_loss = float((focal * m_cls).sum()) / n
    # box terms: smooth-L1, the yaw column / pi counted three times; with sin_yaw its argument is sin(P - G)
    diff = p_reg - np.asarray(G_reg, np.float64)
    val, grad = _smooth_l1(diff)
    if sin_yaw:
        v6, g6 = _smooth_l1(np.sin(diff[..., 6]))
        val[..., 6], grad[..., 6] = v6, g6 * np.cos(diff[..., 6])
    wd = np.array([1.0] * 6 + [3.0 / PI])
    reg_loss = float((val * wd * pos[..., None]).sum()) / n
    # direction
    g = (np.asarray(G_dir) > 0).astype(np.float64)
    dir_loss = float((_bce(p_dir, g) * pos).sum()) / n
    grads = []
    for which in range(3):
        d = np.zeros_like(maps)
        if which == 0:
            d[:, :na] = (d_focal * m_cls / n).reshape(B, na, H, W)
        elif which == 1:
            d[:, na:8 * na] = (grad * wd * pos[..., None] / n).transpose(0, 1, 5, 2, 3, 4).reshape(B, 7 * na, H, W)
        else:
            d[:, 8 * na:] = ((_sigmoid(p_dir) - g) * pos / n).reshape(B, na, H, W)
        grads.append(d)
    return dict(cls_loss=cls_loss, reg_loss=reg_loss, dir_loss=dir_loss, loss=cls_loss + lam * reg_loss + weight * dir_loss,
                normalizer=n, grads=tuple(grads))

"""Deterministic input builders of tests/test_gpu_direction.py, shared with tests/test_host_direction.py, which proves on the CPU --
on the reference alone -- that every case is well-posed.  Every builder is cached: a case is computed once per process and must not
be modified by a test."""
import functools
import zlib

import numpy as np

import direction_ref as D
import proposal_cases as C
import proposal_ref as R

WRAP_MARGIN = 1e-2  # every wrap argument of a decode case stays this far (rad) from a multiple of pi
BIN_MARGIN = 1e-3   # every ground-truth yaw of a target case stays this far from a direction bin edge


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------------------------------ config
def make_cfg(n_cls, n_yaw=2, topk=None, enabled=True, sin_yaw=True, bounds=None, thresh=None):
    """1 class: the shipped car config (anchor yaws 0 and 1.501); 3 classes: the defaults (0 and pi / 2)."""
    from vision3d_amd.core.config import _defaults, second_car_cfg
    cfg = second_car_cfg() if n_cls == 1 else _defaults()
    assert cfg.NUM_CLASSES == n_cls
    cfg.NUM_YAW = n_yaw
    cfg.DIRECTION.ENABLED, cfg.DIRECTION.SIN_YAW = enabled, sin_yaw
    if topk is not None:
        cfg.PROPOSAL.TOPK = topk
    if bounds is not None:
        cfg.GRID_BOUNDS = list(bounds)
    if thresh is not None:
        for a, t in zip(cfg.ANCHORS, thresh):
            a["score_thresh"] = float(t)
    return cfg


# ----------------------------------------------------------------------------------------------------------------------- targets
TARGET_BOUNDS = [0, -1.1, -3, 2.9, 1.1, 1]  # a 5 x 7 anchor grid: 35 cells, 70 anchors per class -- no multiple of 64
TARGET_CASES = [(n_gt, n_cls) for n_cls in (1, 3) for n_gt in (0, 1, 3)]
# (cell iy, ix; anchor yaw index; half turns; offset from the anchor's yaw): the ground truth sits on an anchor, turned by m * pi + eps
_TARGET_GT = [(2, 3, 0, 0, 0.05), (1, 5, 1, 0, 0.04), (3, 1, 1, -1, -0.03)]  # direction bits 1, 0, 1


@functools.lru_cache(maxsize=None)
def target_case(n_gt, n_cls):
    """-> dict(cfg, boxes (n_gt, 7) float32, class_idx (n_gt) int64): ground truth i has class i % n_cls, the size of that class's
    anchor, a centre 5 cm off an anchor's and a yaw a few hundredths off the anchor's modulo pi -- a clear positive."""
    from vision3d_amd.core.anchor_generator import AnchorGenerator
    cfg = make_cfg(n_cls, bounds=TARGET_BOUNDS)
    anchors = AnchorGenerator(cfg).anchors.numpy()
    assert anchors.shape[:4] == (n_cls, 2, 5, 7)
    boxes, classes = [], []
    for i, (iy, ix, yi, m, eps) in enumerate(_TARGET_GT[:n_gt]):
        c = i % n_cls
        b = anchors[c, yi, iy, ix].astype(np.float64)
        b[0] += 0.05
        b[1] -= 0.05
        b[6] += m * np.pi + eps
        boxes.append(b)
        classes.append(c)
    return dict(cfg=cfg, boxes=np.asarray(boxes, np.float32).reshape(-1, 7), class_idx=np.asarray(classes, np.int64))


# -------------------------------------------------------------------------------------------------------------------------- loss
# (B, H, W, n_cls, variant, sin_yaw).  5 x 7: two groups of 35 cells, nothing a multiple of a wave
LOSS_CASES = [(2, 5, 7, 1, "plain", True), (2, 5, 7, 3, "plain", True), (2, 20, 24, 1, "plain", True), (2, 20, 24, 3, "plain", False),
              (2, 20, 24, 1, "no_positives", True), (2, 5, 7, 3, "no_positives", False), (2, 20, 24, 1, "large_logits", True),
              (2, 5, 7, 1, "large_logits", False), (2, 20, 24, 3, "wide_yaw", True), (2, 5, 7, 1, "wide_yaw", False)]


@functools.lru_cache(maxsize=None)
def loss_case(B, H, W, n_cls, variant, sin_yaw):
    """-> dict(maps float32 (B, n_anchor * 9, H, W), G_cls int8, M_cls bool, G_reg float32, M_reg bool (..., 1), G_dir int8, geometry).
    large_logits: every map value times 12 (saturated sigmoids in the class AND direction channels); wide_yaw: predicted yaw residuals
    uniform in [-7, 7], so that P_yaw - G_yaw passes +-pi and +-2 pi."""
    n_yaw = 2
    rng = _rng("loss", B, H, W, n_cls, variant, sin_yaw)
    na = n_cls * n_yaw
    shape = (B, n_cls, n_yaw, H, W)
    maps = (rng.standard_normal((B, na * 9, H, W)) * (12.0 if variant == "large_logits" else 1.5)).astype(np.float32)
    G_cls = (rng.random(shape) > 0.85).astype(np.int8)
    if variant == "no_positives":
        G_cls[:] = 0
    M_cls = rng.random(shape) > 0.2
    G_reg = (rng.standard_normal(shape + (7,)) * 1.2).astype(np.float32)
    G_reg[..., 6] = rng.uniform(0.0, np.pi, shape).astype(np.float32)  # an encoded yaw residual lies in [0, pi)
    if variant == "wide_yaw":
        yaw_ch = na + (np.arange(n_cls)[:, None] * 7 + 6) * n_yaw + np.arange(n_yaw)[None]
        maps[:, yaw_ch.reshape(-1)] = rng.uniform(-7.0, 7.0, (B, na, H, W)).astype(np.float32)
    M_reg = (G_cls == 1)[..., None]
    G_dir = ((rng.random(shape) > 0.5) & M_reg[..., 0]).astype(np.int8)
    return dict(maps=maps, G_cls=G_cls, M_cls=M_cls, G_reg=G_reg, M_reg=M_reg, G_dir=G_dir, n_cls=n_cls, n_yaw=n_yaw, sin_yaw=sin_yaw,
                variant=variant)


def torch_statement(case, dtype, device="cpu"):
    """ProposalLoss's torch expressions (no `_head_maps` in the item) on a loss case -> (leaf maps with requires_grad, losses)"""
    import torch
    from vision3d_amd.detector import ProposalLoss
    cfg = make_cfg(case["n_cls"], case["n_yaw"], sin_yaw=case["sin_yaw"])
    maps = torch.from_numpy(case["maps"]).to(device=device, dtype=dtype).requires_grad_(True)
    B, _, H, W = maps.shape
    n_cls, n_yaw = case["n_cls"], case["n_yaw"]
    na = n_cls * n_yaw
    item = {k: torch.from_numpy(case[k]).to(device) for k in ("G_cls", "M_cls", "M_reg", "G_dir")}
    item["G_reg"] = torch.from_numpy(case["G_reg"]).to(device=device, dtype=dtype)
    item["P_cls"] = maps[:, :na].reshape(B, n_cls, n_yaw, H, W)
    item["P_reg"] = maps[:, na:8 * na].reshape(B, n_cls, 7, n_yaw, H, W).permute(0, 1, 3, 4, 5, 2)
    item["P_dir"] = maps[:, 8 * na:].reshape(B, n_cls, n_yaw, H, W)
    return maps, ProposalLoss(cfg)(item)


# ------------------------------------------------------------------------------------------------------------------------ decode
# SELECT_ROWS[1] at (2, 3): the separate merge and decode launches; [6] and [7] at (1, 1): the fused launch, rank and bitonic sort
DECODE_CASES = [(C.SELECT_ROWS[1], 2, 3), (C.SELECT_ROWS[6], 1, 1), (C.SELECT_ROWS[7], 1, 1)]
HAND_LOGITS = np.array([0.0, -0.0, np.nan, -1e-30, 1e-30], np.float32)  # bits 0, 0, 0, 0, 1
HAND_BITS = np.array([0, 0, 0, 0, 1])


def _with_direction(maps8, anchors, rng, B, n_cls, n_yaw, H, W):
    """maps (B, n_anchor * 8, H, W) -> (B, n_anchor * 9, H, W): the yaw residual of every anchor rebuilt as u + k pi + OFFSET - anchor
    yaw with u in [0.01, pi - 0.01] and k in -2 .. 2 -- the decode rule's wrap argument is u + k pi, at least WRAP_MARGIN from an
    edge -- and random direction logits (none of them zero) behind the box channels."""
    na, n = n_cls * n_yaw, n_yaw * H * W
    u = rng.uniform(WRAP_MARGIN, np.pi - WRAP_MARGIN, (B, n_cls, n_yaw, H, W))
    k = rng.integers(-2, 3, (B, n_cls, n_yaw, H, W))
    d_yaw = (u + k * np.pi + D.OFFSET - anchors[None, ..., 6].astype(np.float64)).astype(np.float32)
    maps = np.zeros((B, na * 9, H, W), np.float32)
    maps[:, :na * 8] = maps8
    yaw_ch = na + (np.arange(n_cls)[:, None] * 7 + 6) * n_yaw + np.arange(n_yaw)[None]  # channel n_anchor + (c * 7 + 6) * n_yaw + yaw
    maps[:, yaw_ch.reshape(-1)] = d_yaw.reshape(B, na, H, W)
    logits = rng.standard_normal((B, na, H, W)).astype(np.float32)
    logits[logits == 0] = 0.5
    maps[:, na * 8:] = logits
    return maps


def _expected(maps, anchors, geom):
    """reference candidates of the first n_anchor * 8 channels + the decode rule on their yaw"""
    B, n_cls, n_yaw, H, W, topk = geom
    na, n = n_cls * n_yaw, n_yaw * H * W
    idx, sc, boxes = R.candidates(maps[:, :na * 8], anchors, B, n_cls, n_yaw, H, W, topk)
    logit = np.take_along_axis(maps[:, na * 8:].reshape(B, n_cls, n), idx, 2)
    return idx, sc, boxes, logit, D.decode_yaw(boxes[..., 6], logit)


@functools.lru_cache(maxsize=None)
def decode_case(row, B, n_cls):
    """proposal_cases.decode_case with the yaw channel rebuilt and direction channels appended; at (1, 1) the direction logits of the
    first five selected anchors are HAND_LOGITS.  -> dict(maps, anchors, logits, geom, idx, scores, boxes (float64, RAW yaw), dir_logit,
    yaw (float64, the decode rule))"""
    base = C.decode_case(row, B, n_cls)
    n_yaw, H, W, topk = row
    geom = (B, n_cls, n_yaw, H, W, topk)
    maps = _with_direction(base["maps"], base["anchors"], _rng("direction-decode", row, B, n_cls), B, n_cls, n_yaw, H, W)
    hand = None
    if (B, n_cls) == (1, 1):
        hand = base["idx"][0, 0, :len(HAND_LOGITS)]  # selection reads the class channels only: the same anchors are selected
        maps[0, n_cls * n_yaw * 8:].reshape(-1)[hand] = HAND_LOGITS
    idx, sc, boxes, logit, yaw = _expected(maps, base["anchors"], geom)
    assert np.array_equal(idx, base["idx"])
    return dict(maps=maps, anchors=base["anchors"], logits=base["logits"], geom=geom, idx=idx, scores=sc, boxes=boxes, dir_logit=logit,
                yaw=yaw, hand=hand)


# ------------------------------------------------------------------------------------------------------------------- whole stage
STAGE_ROW = C.SELECT_ROWS[2]  # three classes: 48 candidates
STAGE_SEED = 0                # chosen on the CPU: test_host_direction.py asserts the margin


@functools.lru_cache(maxsize=None)
def stage_case():
    """proposal_cases.stage_case's scene with the yaw channel rebuilt and direction channels appended.  ref = the plain stage
    (proposal_ref.stage) on the class / box channels: a rectangle turned by pi is the same rectangle, so the direction stage keeps the
    same candidates; yaw (flat candidate order) = the decode rule."""
    n_yaw, H, W, topk = STAGE_ROW
    B, n_cls = 1, 3
    base = C.stage_case(STAGE_ROW)
    geom = (B, n_cls, n_yaw, H, W, topk)
    maps = _with_direction(base["maps"], base["anchors"], _rng("direction-stage", STAGE_SEED), B, n_cls, n_yaw, H, W)
    ref = R.stage(maps[:, :n_cls * n_yaw * 8], base["anchors"], B, n_cls, n_yaw, H, W, topk, C.STAGE_THRESH, C.STAGE_IOU)
    _, _, boxes, logit, yaw = _expected(maps, base["anchors"], geom)
    return dict(maps=maps, anchors=base["anchors"], logits=base["logits"], geom=geom, ref=ref, raw=boxes[..., 6].reshape(-1),
                yaw=yaw.reshape(-1), thresh=C.STAGE_THRESH, iou=C.STAGE_IOU)

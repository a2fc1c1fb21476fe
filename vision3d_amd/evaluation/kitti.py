"""KITTI 2-D bbox, BEV and 3-D average precision and average orientation similarity (AOS), evaluated on the device
(csrc/kitti_eval.hip).  The upstream project has no evaluator.

The protocol is the KITTI devkit's as its widely used Python port states it, in the rectified camera frame, so the numbers
compare with published ones.  It is NOT the loader's `Labels.level` (dataset/kitti.py `_difficulty`, the upstream loader's
`+1`, `>=` rule); this module never reads `level`.

Overlaps, for every (detection, ground truth) pair of a frame, from ONE polygon clip (rotated_iou.h, fp32):
  BEV  IoU of (x, z, l, w, ry) in the camera's (x, z) plane.  l lies along the heading; rotation by ry about the camera's y
       axis (pointing down) turns the local x axis to (cos ry, -sin ry).  (The core takes degrees: -ry * 180 / pi.)
  3-D  BEV intersection * y-overlap / union of the volumes; y-overlap = min(y1, y2) - max(y1 - h1, y2 - h2) clamped at 0,
       y the box bottom.
  bbox IoU of the image boxes (x1, y1, x2, y2), no +1: iw = min(x2) - max(x1), ih = min(y2) - max(y1); 0 unless both > 0, else
       iw * ih / (area_dt + area_gt - iw * ih).  (Separate pass over the pairs, double precision, stored as float32.)

Per class c, difficulty d (easy, moderate, hard), metric and minimum overlap t_min:
  MIN_HEIGHT = [40, 25, 25], MAX_OCCLUSION = [0, 1, 2], MAX_TRUNCATION = [0.15, 0.3, 0.5];
  t_min "strict": Car 0.7, Pedestrian 0.5, Cyclist 0.5; "loose": 0.5 / 0.25 / 0.25 (BEV and 3-D alike).  bbox and aos use
    0.7 / 0.5 / 0.5 in both sets (the loose set loosens BEV and 3-D only).
  Ground truth (height = y2 - y1 of the 2-D box, no +1):
    valid = 1 if its name is c, 0 if it is c's neighbour (Van for Car, Person_sitting for Pedestrian), else -1 (DontCare and
    every other name included); ignore = occ > MAX_OCCLUSION[d] or trunc > MAX_TRUNCATION[d] or height <= MIN_HEIGHT[d];
    ignored_gt = 0 if valid == 1 and not ignore (these are n_valid_gt), 1 if valid == 0 or (valid == 1 and ignore), else -1.
  Detection (height = |y2 - y1|): ignored_dt = 1 if height < MIN_HEIGHT[d] (first, whatever the class), else 0 if its class
    is c, else -1.
  assign(frame, thresh, compute_fp): ground truths in file order, skipping ignored_gt == -1; over the detections, skip
    ignored_dt == -1, already assigned ones and (compute_fp) those with score < thresh; only pairs with overlap > t_min.
    Without compute_fp the highest score wins (ties: the earlier detection).  With compute_fp an ignored_dt == 0 detection
    wins if its overlap is larger than the best so far or the current pick is an ignored detection; an ignored_dt == 1
    detection is taken only while nothing is picked.  Then: no pick and ignored_gt == 0 -> FN; a pick with ignored_gt == 1 or
    ignored_dt == 1 -> assigned, neither TP nor FP; any other pick -> TP, assigned, (pass 1) its score recorded.  With
    compute_fp, FP = detections not assigned, with ignored_dt == 0 and not under thresh.  DontCare regions play no part in
    BEV and 3-D.
  Pass 1: assign(., 0, False) over all frames -> TP scores.
  Thresholds: TP scores in descending order, current = 0; score i (0-based): l = (i+1)/n_valid_gt, r = (i+2)/n_valid_gt
    (r = l for the last); skip it if (r - current) < (current - l) and it is not the last, else take it and current += 1/40.
    Double precision, in this order; at most 41 thresholds.
  Pass 2: per threshold, (tp, fp, fn) = sum over frames of assign(., thresh, True).
  Pass 2, bbox only: after the FP count, every detection still unassigned, with ignored_dt == 0 and not under thresh, whose
    inter / area_dt (not IoU) with any ground truth named DontCare is > t_min is absorbed: fp -= 1, assigned.  (DontCare ground
    truths stay ignored_gt == -1 for the matching; pass 1 has no DontCare step.)
  precision[k] = tp / (tp + fp) (0 when tp + fp == 0 and for k >= the number of thresholds) on 41 entries, then
    precision[k] = max(precision[k:]); AP_R11 = sum(precision[0, 4, ..., 40]) / 11 * 100, AP_R40 = sum(precision[1..40]) / 40
    * 100, summed in index order.  A class without valid ground truth gets AP 0.
  AOS (on the bbox combos' own thresholds and counts): every true positive of pass 2 adds (1 + cos(alpha_gt - alpha_dt)) / 2,
    in double; similarity[k] = that sum over all frames at threshold k (a frame with tp == fp == 0 adds nothing);
    aos[k] = similarity[k] / (tp + fp) with fp after absorption (0 when tp + fp == 0 and for k >= the number of thresholds),
    then the running maximum and the R11 / R40 sums of AP.  Each frame's sum is added as 32.32 fixed point (integer atomics),
    so the total is deterministic whatever the frame order.
  Alpha is taken as given: ground truth and file detections field 3 of the line, model detections
    -atan2(-y_lidar, x_lidar) + ry (what write_kitti_results writes).  The devkit's -10 ("unknown") is not special-cased: a
    detection with alpha -10 simply scores its cosine.

COCO-style AP (overlap set "coco"; the port's get_coco_eval_result / do_coco_style_eval): the same AP averaged over ten
minimum overlaps.
  Levels per class: Car np.linspace(0.5, 0.95, 10); Pedestrian and Cyclist np.linspace(0.25, 0.70, 10).  Computed in double,
    each stored as the nearest float32 in v3d_kitti_combo.min_overlap and compared exactly as above (overlap > level).  The
    same levels apply to bbox, BEV and 3-D; the strict / loose split does not apply to the sweep.
  Per level: each (class, metric, difficulty, level) is an ordinary combo run through the protocol above unchanged -- pass 1,
    the thresholds, pass 2, the R11 / R40 sums; for bbox the DontCare absorption at inter / area_dt > level; AOS from the bbox
    combos' counts.
  COCO value: the mean over the ten levels of AP_R11, AP_R40, AOS_R11 and AOS_R40, each summed in double in level order, then
    divided by 10.
  Summary: one line per class and AP kind, `Car coco AP_R40@0.50:0.05:0.95: bev: ...  3d: ...`.

Limits: 1 024 detections and 256 ground truths per frame (RuntimeError beyond them).  No CPU fallback.
"""
import math

import numpy as np
import torch

from .. import _lib as L
from ..dataset import kitti as K

MIN_HEIGHT = (40.0, 25.0, 25.0)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
DIFFICULTIES = ("easy", "moderate", "hard")
MIN_OVERLAP = {"strict": {"Car": 0.7, "Pedestrian": 0.5, "Cyclist": 0.5},
               "loose": {"Car": 0.5, "Pedestrian": 0.25, "Cyclist": 0.25}}  # BEV and 3-D
MIN_OVERLAP_IMAGE = {"Car": 0.7, "Pedestrian": 0.5, "Cyclist": 0.5}  # bbox and aos, in both overlap sets
COCO_RANGE = {"Car": (0.5, 0.95), "Pedestrian": (0.25, 0.70), "Cyclist": (0.25, 0.70)}  # first and last level
COCO_LEVELS = {c: np.linspace(lo, hi, 10).astype(np.float32) for c, (lo, hi) in COCO_RANGE.items()}  # every metric
OVERLAP_SETS = ("strict", "loose", "coco")
METRICS = ("bbox", "bev", "3d", "aos")
METRIC_BEV, METRIC_3D, METRIC_BBOX = 0, 1, 2  # v3d_kitti_combo.metric (V3D_KITTI_METRIC_*): the overlap plane a combo reads
METRIC_CODE = {"bev": METRIC_BEV, "3d": METRIC_3D, "bbox": METRIC_BBOX}
DONTCARE_BIT = 3  # gt_meta[1] bit: the ground truth is a DontCare region (V3D_KITTI_DONTCARE_BIT)
NEIGHBOUR = {"Car": "Van", "Pedestrian": "Person_sitting", "Cyclist": None}
CLASS_CODE = {"Car": 0, "Pedestrian": 1, "Cyclist": 2, "Van": 3, "Person_sitting": 4}  # every other name: OTHER
CODE_OTHER = 5
MAX_DT, MAX_GT, SAMPLE_PTS = 1024, 256, 41


def class_code(name):
    return CLASS_CODE.get(name, CODE_OTHER)


def min_overlap(overlap_set, cls, metric):
    """t_min of one (overlap set, class, metric): MIN_OVERLAP for BEV / 3-D, MIN_OVERLAP_IMAGE for bbox / aos."""
    return MIN_OVERLAP_IMAGE[cls] if metric in ("bbox", "aos") else MIN_OVERLAP[overlap_set][cls]


def coco_header(cls, kind="R40"):
    """`coco AP_R40@0.50:0.05:0.95`: the summary's name of the COCO-style AP of a class (first level, step, last level)."""
    lo, hi = COCO_RANGE[cls]
    return f"coco AP_{kind}@{lo:.2f}:{(hi - lo) / 9:.2f}:{hi:.2f}"


def calib_rows(calib):
    """(26,) float32: R0 . V2C (3, 4), P2 (3, 4), image (W, H) -- what the camera conversion reads of one frame's calibration."""
    m = (np.asarray(calib.R0, np.float32) @ np.asarray(calib.V2C, np.float32)).astype(np.float32)
    return np.concatenate([m.ravel(), np.asarray(calib.P2, np.float32).ravel(), np.asarray(calib.WH, np.float32).ravel()])


def lidar_to_camera(boxes, calib):
    """Lidar-frame boxes (K, 7) = (x, y, z, w, l, h, yaw) -> (cam (K, 7) = rectified-camera (x, y_bottom, z, h, w, l, ry),
    box2d (K, 4) = (x1, y1, x2, y2)), float32, on the tensors' device, elementwise torch ops (no host loop over boxes).
    `calib` is (K, 26) rows of `calib_rows`, one per box (a gather of per-frame rows).  Centre through R0 . V2C, bottom
    y = y_c + h / 2, (h, w, l) from columns (5, 3, 4), ry = -yaw; the 2-D box is the min / max of the 8 corners projected through
    P2, clipped to [0, 0, W, H]."""
    x, y, z, w, l, h = (boxes[:, k] for k in range(6))
    ry = -boxes[:, 6]
    m = [[calib[:, 4 * r + c] for c in range(4)] for r in range(3)]
    cx, cy, cz = (m[r][0] * x + m[r][1] * y + m[r][2] * z + m[r][3] for r in range(3))
    yb = cy + h / 2
    cam = torch.stack((cx, yb, cz, h, w, l, ry), 1)
    half_l, half_w = (l / 2)[:, None], (w / 2)[:, None]
    sx = torch.tensor([1, 1, -1, -1, 1, 1, -1, -1], dtype=boxes.dtype, device=boxes.device)
    sz = torch.tensor([1, -1, -1, 1, 1, -1, -1, 1], dtype=boxes.dtype, device=boxes.device)
    top = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1], dtype=boxes.dtype, device=boxes.device)
    lx, lz = half_l * sx, half_w * sz
    c, s = torch.cos(ry)[:, None], torch.sin(ry)[:, None]
    X = c * lx + s * lz + cx[:, None]
    Y = yb[:, None] - h[:, None] * top
    Z = c * lz - s * lx + cz[:, None]
    p = [[calib[:, 12 + 4 * r + k][:, None] for k in range(4)] for r in range(3)]
    u, v, q = (p[r][0] * X + p[r][1] * Y + p[r][2] * Z + p[r][3] for r in range(3))
    u, v = u / q, v / q
    zero = torch.zeros_like(x)
    W, H = calib[:, 24], calib[:, 25]
    box2d = torch.stack((torch.minimum(torch.maximum(u.amin(1), zero), W), torch.minimum(torch.maximum(v.amin(1), zero), H),
                         torch.minimum(torch.maximum(u.amax(1), zero), W), torch.minimum(torch.maximum(v.amax(1), zero), H)), 1)
    return cam, box2d


def write_kitti_results(path, boxes, class_idx, scores, calib, names):
    """One frame of lidar-frame detections (boxes (K, 7), class_idx (K,), scores (K,); tensors on any device, or arrays) as a
    KITTI result file: `name -1 -1 alpha x1 y1 x2 y2 h w l x y z ry score`, alpha = -atan2(-y_lidar, x_lidar) + ry.  Numbers are
    written with %.9g, so `dataset.kitti.read_labels` reads back the float32 values computed here."""
    b = torch.as_tensor(boxes).float().reshape(-1, 7)
    rows = torch.from_numpy(calib_rows(calib)).to(b.device)[None].expand(b.shape[0], 26)
    cam, box2d = lidar_to_camera(b, rows)
    b, cam, box2d = (t.cpu().numpy() for t in (b, cam, box2d))
    cls = np.asarray(torch.as_tensor(class_idx).cpu()).reshape(-1)
    sc = np.asarray(torch.as_tensor(scores).float().cpu()).reshape(-1)
    with open(path, "w") as f:
        for k in range(len(b)):
            alpha = np.float32(-math.atan2(-float(b[k, 1]), float(b[k, 0])) + float(cam[k, 6]))
            vals = [alpha, *box2d[k], *cam[k, 3:6], *cam[k, 0:3], cam[k, 6], sc[k]]
            f.write(f"{names[int(cls[k])]} -1 -1 " + " ".join(f"{float(v):.9g}" for v in vals) + "\n")


def _height_flags(height, short):
    """Bit d = the 2-D height test of difficulty d: `height < MIN_HEIGHT[d]` (detections, short=True) or `<=` (ground truth)."""
    flags = np.zeros(len(height), np.int32)
    for d, mh in enumerate(MIN_HEIGHT):
        flags |= ((height < mh) if short else (height <= mh)).astype(np.int32) << d
    return flags


def _camera_rows(labels):
    """(n, 7) float32 (x, y_bottom, z, h, w, l, ry) of a Labels (its `location` is the centre: the bottom is y + h / 2)."""
    h = labels.hwl[:, 0]
    return np.stack((labels.location[:, 0], labels.location[:, 1] + h / 2, labels.location[:, 2], h, labels.hwl[:, 1],
                     labels.hwl[:, 2], labels.ry), 1).astype(np.float32).reshape(-1, 7)


def _gt_arrays(labels):
    box2d = np.asarray(labels.box2d, np.float64).reshape(-1, 4)
    height = box2d[:, 3] - box2d[:, 1]
    flags = _height_flags(height, short=False)
    for d in range(3):
        flags |= ((labels.occlusion > MAX_OCCLUSION[d]) | (labels.truncation > MAX_TRUNCATION[d])).astype(np.int32) << d
    flags |= np.array([n.lower() == "dontcare" for n in labels.names], np.int32).reshape(-1) << DONTCARE_BIT
    codes = np.array([class_code(n) for n in labels.names], np.int32)
    return _camera_rows(labels), np.stack((codes, flags), 1).astype(np.int32).reshape(-1, 2)


def _image_rows(labels):
    """(n, 5) float32 (x1, y1, x2, y2, alpha) of a Labels."""
    return np.concatenate([np.asarray(labels.box2d, np.float64).reshape(-1, 4), np.asarray(labels.alpha, np.float64).reshape(-1, 1)],
                          1).astype(np.float32)


def _dt_arrays(labels):
    box2d = np.asarray(labels.box2d, np.float64).reshape(-1, 4)
    flags = _height_flags(np.abs(box2d[:, 3] - box2d[:, 1]), short=True)
    codes = np.array([class_code(n) for n in labels.names], np.int32)
    rows = np.concatenate([_camera_rows(labels), np.asarray(labels.score, np.float32).reshape(-1, 1)], 1)
    return rows.astype(np.float32), np.stack((codes, flags), 1).astype(np.int32).reshape(-1, 2)


def _check(code, what, max_dt, max_gt):
    if code == -3:  # V3D_EUNSUPPORTED
        raise RuntimeError(f"{what}: a frame holds {max_dt} detections / {max_gt} ground truths; the device evaluation supports at "
                           f"most {MAX_DT} / {MAX_GT} per frame")
    L.check(code, what)


def camera_box_overlaps(dt_boxes, gt_boxes):
    """(BEV, 3-D) IoU matrices (K, N) float32 of rectified-camera boxes (K, 7) x (N, 7) = (x, y_bottom, z, h, w, l, ry), on the
    GPU: the overlaps stage of the evaluator for a single frame."""
    L.require_gpu("camera_box_overlaps", dt_boxes, gt_boxes)
    dt = L.as_f32("camera_box_overlaps", dt_boxes)
    gt = L.as_f32("camera_box_overlaps", gt_boxes)
    if dt.dim() != 2 or gt.dim() != 2 or dt.shape[1] != 7 or gt.shape[1] != 7:
        raise RuntimeError("camera_box_overlaps: expected (K,7) and (N,7)")
    k, n = dt.shape[0], gt.shape[0]
    dev = dt.device
    dt8 = torch.cat([dt, torch.zeros((k, 1), dtype=torch.float32, device=dev)], 1).contiguous()
    offs = torch.tensor([0, n, 0, k], dtype=torch.int32, device=dev)
    ov_off = torch.tensor([0, k * n], dtype=torch.int64, device=dev)
    ov = torch.zeros((2, max(k * n, 1)), dtype=torch.float32, device=dev)
    with L.device_guard(dev):
        _check(L.lib().v3d_kitti_eval_overlaps(L.ptr(gt), L.ptr(offs), L.ptr(dt8), L.ptr(offs[2:]), L.ptr(ov_off), 1, k, n,
                                               L.ptr(ov[0]), L.ptr(ov[1]), L.stream_ptr()), "camera_box_overlaps", k, n)
    return ov[0, :k * n].view(k, n), ov[1, :k * n].view(k, n)


class KittiEvaluator:
    """Accumulates frames (`add_frame`) and evaluates them all at once on the GPU (`compute`): a fixed number of launches and one
    host read, whatever the frame count.  `metrics` is any of "bbox", "bev", "3d", "aos" (default BEV and 3-D); "aos" is computed
    from the bbox combos, which run whenever "bbox" or "aos" is asked for.  `overlaps` is any of "strict", "loose" (default both)
    and "coco", the COCO-style AP over ten minimum overlaps per class (COCO_LEVELS).  `det_names[class_idx]` names model
    detections added as tensors (default: the KITTI class order of dataset/kitti.py)."""

    def __init__(self, classes=("Car", "Pedestrian", "Cyclist"), metrics=("bev", "3d"), overlaps=("strict", "loose"),
                 det_names=("Car", "Pedestrian", "Cyclist"), device=None):
        for c in classes:
            if c not in NEIGHBOUR:
                raise ValueError(f"KittiEvaluator: unknown class {c!r} (Car, Pedestrian, Cyclist)")
        for m in metrics:
            if m not in METRICS:
                raise ValueError(f"KittiEvaluator: unknown metric {m!r} (bbox, bev, 3d, aos)")
        for o in overlaps:
            if o not in OVERLAP_SETS:
                raise ValueError(f"KittiEvaluator: unknown overlap set {o!r} (strict, loose, coco)")
        self.classes, self.metrics, self.overlaps = tuple(classes), tuple(metrics), tuple(overlaps)
        self.det_names = tuple(det_names)
        self.device = torch.device(device) if device is not None else None
        # device combos (overlap set, class, metric, difficulty, level: the sweep's index, None in strict / loose): BEV / 3-D
        # first, then the bbox combos (which also carry aos)
        levels = {o: range(len(COCO_LEVELS["Car"])) if o == "coco" else (None,) for o in self.overlaps}
        self.combos = [(o, c, m, d, k) for o in self.overlaps for c in self.classes for m in self.metrics if m in ("bev", "3d")
                       for d in range(3) for k in levels[o]]
        self.image = "bbox" in self.metrics or "aos" in self.metrics
        if self.image:
            self.combos += [(o, c, "bbox", d, k) for o in self.overlaps for c in self.classes for d in range(3) for k in levels[o]]
        self.frames = []
        self.details = {}
        self.result = None

    def __len__(self):
        return len(self.frames)

    def add_frame(self, labels, detections):
        """labels: ground truth, a `dataset.kitti.Labels`.  detections: a `Labels` read from a KITTI result file, or model output
        in the lidar frame `(boxes (K, 7), class_idx (K,), scores (K,), calib)` (tensors may stay on the GPU)."""
        gt = _gt_arrays(labels) + (_image_rows(labels),)
        if isinstance(detections, K.Labels):
            self.frames.append((gt, ("labels",) + _dt_arrays(detections) + (_image_rows(detections),)))
            return
        boxes, class_idx, scores, calib = detections
        L.require_gpu("KittiEvaluator.add_frame", boxes, class_idx, scores)
        boxes = L.as_f32("KittiEvaluator.add_frame", boxes).reshape(-1, 7)
        if class_idx.shape[0] != boxes.shape[0] or scores.shape[0] != boxes.shape[0]:
            raise RuntimeError("KittiEvaluator.add_frame: boxes, class_idx and scores differ in length")
        codes = np.array([class_code(n) for n in self.det_names] + [CODE_OTHER], np.int32)
        self.frames.append((gt, ("model", boxes, class_idx, scores.float(), calib_rows(calib), codes)))

    # ---- the ragged batch --------------------------------------------------------------------------------------------------
    def _device(self):
        if self.device is not None:
            return self.device
        for _, d in self.frames:
            if d[0] == "model":
                return d[1].device
        return torch.device("cuda", torch.cuda.current_device())

    def _detections(self, dev):
        """(dt (D, 8) f32, dt_meta (D, 2) i32, dt_img (D, 5) f32 or None) on `dev`, frame-major: file detections in one upload,
        model detections converted to the camera frame in one batch (per-frame calibration rows gathered per detection).
        dt_img (image box, alpha) is filled only when a bbox / aos metric is asked for."""
        file_pos, file_rows, file_meta, file_img, model_pos, model, calibs, counts = [], [], [], [], [], [], [], []
        at = 0
        for _, d in self.frames:
            if d[0] == "labels":
                n = len(d[1])
                file_pos.append(np.arange(at, at + n))
                file_rows.append(d[1])
                file_meta.append(d[2])
                file_img.append(d[3])
            else:
                n = d[1].shape[0]
                model_pos.append(np.arange(at, at + n))
                model.append(d)
                calibs.append(d[4])
                counts.append(n)
            at += n
        dt = torch.empty((max(at, 1), 8), dtype=torch.float32, device=dev)
        meta = torch.empty((max(at, 1), 2), dtype=torch.int32, device=dev)
        img = torch.zeros((max(at, 1), 5), dtype=torch.float32, device=dev) if self.image else None
        if file_rows:
            pos = torch.from_numpy(np.concatenate(file_pos)).to(dev)
            dt[pos] = torch.from_numpy(np.concatenate(file_rows)).to(dev)
            meta[pos] = torch.from_numpy(np.concatenate(file_meta)).to(dev)
            if self.image:
                img[pos] = torch.from_numpy(np.concatenate(file_img)).to(dev)
        if model:
            pos = torch.from_numpy(np.concatenate(model_pos)).to(dev)
            boxes = torch.cat([d[1] for d in model]).to(dev)
            cls = torch.cat([d[2].to(dev).long() for d in model])
            scores = torch.cat([d[3] for d in model]).to(dev)
            frame = torch.from_numpy(np.repeat(np.arange(len(model)), counts)).to(dev)
            rows = torch.from_numpy(np.stack(calibs)).to(dev)[frame]
            codes = torch.from_numpy(np.stack([d[5] for d in model])).to(dev)
            cam, box2d = lidar_to_camera(boxes, rows)
            height = (box2d[:, 3] - box2d[:, 1]).abs()
            flags = sum((height < mh).int() << d for d, mh in enumerate(MIN_HEIGHT))
            n_names = codes.shape[1] - 1
            code = codes[frame, torch.where((cls >= 0) & (cls < n_names), cls, torch.full_like(cls, n_names))]
            dt[pos] = torch.cat([cam, scores[:, None]], 1)
            meta[pos] = torch.stack((code, flags.int()), 1)
            if self.image:  # alpha as write_kitti_results computes it: in double, rounded to float32
                alpha = -torch.atan2(-boxes[:, 1].double(), boxes[:, 0].double()) + cam[:, 6].double()
                img[pos] = torch.cat([box2d, alpha.float()[:, None]], 1)
        return dt, meta, img

    def _layout(self):
        """(name, shape) of every per-combo output, in the order of compute()'s one host read; aos and similarity (its 32.32
        sums scaled to float) only with bbox combos, one row per combo."""
        n = len(self.combos)
        out = [("ap", (n, 2)), ("n_valid", (n,)), ("n_thr", (n,)), ("thr", (n, SAMPLE_PTS)), ("counts", (n, SAMPLE_PTS, 3))]
        return out + ([("aos", (n, 2)), ("similarity", (n, SAMPLE_PTS))] if self.image else [])

    def compute(self):
        """Evaluates every frame added so far -> result[overlap_set][class][metric]["R11" | "R40"] = [easy, moderate, hard] in
        percent.  Per-combo detail (n_valid_gt, thresholds, (tp, fp, fn) per threshold; bbox combos also the similarity sum
        per threshold) lands in `self.details`, keyed (overlap_set, class, "bev" | "3d" | "bbox", difficulty).  A "coco" key
        holds `levels` (10,) float32, `ap` (10, 2) per-level (R11, R40), for bbox also `aos` (10, 2), and `per_level`, the ten
        per-combo detail dicts."""
        n_gt = np.array([len(g[0]) for g, _ in self.frames], np.int64)
        n_dt = np.array([len(d[1]) if d[0] == "labels" else d[1].shape[0] for _, d in self.frames], np.int64)
        if self.frames:
            packed = self._run(n_gt, n_dt)
        else:
            packed = np.zeros(sum(int(np.prod(shape)) for _, shape in self._layout()))
        self._unpack(packed)
        return self.result

    def _run(self, n_gt, n_dt):
        dev = self._device()
        n_frames, n_combos = len(self.frames), len(self.combos)
        max_dt, max_gt = int(n_dt.max()), int(n_gt.max())
        G = int(n_gt.sum())
        with L.device_guard(dev):
            gt = torch.from_numpy(np.concatenate([g[0] for g, _ in self.frames] + [np.zeros((1, 7), np.float32)])).to(dev)
            gt_meta = torch.from_numpy(np.concatenate([g[1] for g, _ in self.frames] + [np.zeros((1, 2), np.int32)])).to(dev)
            gt_img = None
            if self.image:
                gt_img = torch.from_numpy(np.concatenate([g[2] for g, _ in self.frames] + [np.zeros((1, 5), np.float32)])).to(dev)
            dt, dt_meta, dt_img = self._detections(dev)
            off = torch.from_numpy(np.concatenate([np.r_[0, np.cumsum(n_gt)], np.r_[0, np.cumsum(n_dt)]]).astype(np.int32)).to(dev)
            gt_off, dt_off = off[: n_frames + 1], off[n_frames + 1:]
            pairs = (dt_off[1:] - dt_off[:-1]).long() * (gt_off[1:] - gt_off[:-1]).long()
            ov_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(pairs, 0)])
            n_pairs = int((n_dt * n_gt).sum())
            # one plane per metric code (BEV, 3-D, bbox); a combo reads plane `metric`
            ov = torch.empty((3 if self.image else 2, max(n_pairs, 1)), dtype=torch.float32, device=dev)
            combos = (L.KittiCombo * n_combos)(*[
                L.KittiCombo(CLASS_CODE[c], CLASS_CODE.get(NEIGHBOUR[c]) if NEIGHBOUR[c] else -1, d, METRIC_CODE[m],
                             min_overlap(o, c, m) if k is None else COCO_LEVELS[c][k]) for o, c, m, d, k in self.combos])
            cap = max(G, 1)
            ints = torch.zeros(2 * n_combos + n_combos * SAMPLE_PTS * 3, dtype=torch.int32, device=dev)
            tp_count, n_valid, counts = ints[:n_combos], ints[n_combos:2 * n_combos], ints[2 * n_combos:]
            tp_scores = torch.full((n_combos, cap), -math.inf, dtype=torch.float32, device=dev)
            thr = torch.zeros((n_combos, SAMPLE_PTS), dtype=torch.float32, device=dev)
            n_thr = torch.zeros(n_combos, dtype=torch.int32, device=dev)
            ap = torch.zeros((n_combos, 2), dtype=torch.float64, device=dev)
            sim = torch.zeros((n_combos, SAMPLE_PTS), dtype=torch.int64, device=dev) if self.image else None
            aos = torch.zeros((n_combos, 2), dtype=torch.float64, device=dev) if self.image else None
            lib, st, what = L.lib(), L.stream_ptr(), "KittiEvaluator.compute"
            if {"bev", "3d"} & set(self.metrics):
                _check(lib.v3d_kitti_eval_overlaps(L.ptr(gt), L.ptr(gt_off), L.ptr(dt), L.ptr(dt_off), L.ptr(ov_off), n_frames,
                                                   max_dt, max_gt, L.ptr(ov[METRIC_BEV]), L.ptr(ov[METRIC_3D]), st),
                       what, max_dt, max_gt)
            if self.image:
                _check(lib.v3d_kitti_eval_overlaps_image(L.ptr(gt_img), L.ptr(gt_off), L.ptr(dt_img), L.ptr(dt_off),
                                                         L.ptr(ov_off), n_frames, max_dt, max_gt, L.ptr(ov[METRIC_BBOX]), st),
                       what, max_dt, max_gt)
            batch = (n_frames, max_dt, max_gt, combos, n_combos)
            _check(lib.v3d_kitti_eval_pass1(L.ptr(gt_meta), L.ptr(gt_off), L.ptr(dt), L.ptr(dt_meta), L.ptr(dt_off),
                                            L.ptr(ov_off), L.ptr(ov), ov.stride(0), *batch, cap, L.ptr(tp_count),
                                            L.ptr(tp_scores), L.ptr(n_valid), st), what, max_dt, max_gt)
            sorted_scores = torch.sort(tp_scores, dim=1, descending=True).values.contiguous()
            L.check(lib.v3d_kitti_eval_thresholds(L.ptr(sorted_scores), cap, L.ptr(tp_count), L.ptr(n_valid), n_combos, L.ptr(thr),
                                                  L.ptr(n_thr), st), what)
            _check(lib.v3d_kitti_eval_pass2(L.ptr(gt_meta), L.ptr(gt_off), L.ptr(gt_img), L.ptr(dt), L.ptr(dt_meta),
                                            L.ptr(dt_off), L.ptr(dt_img), L.ptr(ov_off), L.ptr(ov), ov.stride(0), *batch,
                                            L.ptr(thr), L.ptr(n_thr), L.ptr(counts), L.ptr(sim), st), what, max_dt, max_gt)
            L.check(lib.v3d_kitti_eval_ap(L.ptr(counts), L.ptr(sim), L.ptr(n_thr), n_combos, L.ptr(ap), L.ptr(aos), st), what)
            parts = dict(ap=ap, n_valid=n_valid, n_thr=n_thr, thr=thr, counts=counts)
            if self.image:
                parts.update(aos=aos, similarity=sim.double() * 2.0 ** -32)
            out = torch.cat([parts[name].double().flatten() for name, _ in self._layout()])
            return out.cpu().numpy()  # the one host read

    def _unpack(self, packed):
        out, at = {}, 0
        for name, shape in self._layout():
            size = int(np.prod(shape))
            out[name] = packed[at: at + size].reshape(shape)
            at += size
        n_valid, n_thr, counts = out["n_valid"].astype(np.int64), out["n_thr"].astype(np.int64), out["counts"].astype(np.int64)
        result = {o: {c: {m: {"R11": [0.0] * 3, "R40": [0.0] * 3} for m in self.metrics} for c in self.classes}
                  for o in self.overlaps}
        self.details = {}
        for k, (o, c, m, d, lvl) in enumerate(self.combos):
            det = dict(n_valid_gt=int(n_valid[k]), thresholds=out["thr"][k, : n_thr[k]].copy(), counts=counts[k, : n_thr[k]].copy())
            if m == "bbox":
                det["similarity"] = out["similarity"][k, : n_thr[k]].copy()
            if lvl is not None:  # a sweep level: gathered below
                sweep = self.details.setdefault((o, c, m, d), dict(levels=COCO_LEVELS[c].copy(), ap=np.zeros((len(COCO_LEVELS[c]), 2)),
                                                                    per_level=[None] * len(COCO_LEVELS[c])))
                sweep["ap"][lvl] = out["ap"][k]
                sweep["per_level"][lvl] = det
                if m == "bbox":
                    sweep.setdefault("aos", np.zeros((len(COCO_LEVELS[c]), 2)))[lvl] = out["aos"][k]
                continue
            if m in self.metrics:
                result[o][c][m]["R11"][d] = float(out["ap"][k, 0])
                result[o][c][m]["R40"][d] = float(out["ap"][k, 1])
            self.details[(o, c, m, d)] = det
            if m == "bbox" and "aos" in self.metrics:
                result[o][c]["aos"]["R11"][d] = float(out["aos"][k, 0])
                result[o][c]["aos"]["R40"][d] = float(out["aos"][k, 1])
        if "coco" in self.overlaps:  # the mean over the levels, summed in double in level order
            for c in self.classes:
                for m in self.metrics:
                    key, src = ("bbox", "aos") if m == "aos" else (m, "ap")
                    for d in range(3):
                        vals = self.details[("coco", c, key, d)][src]
                        for col, kind in enumerate(("R11", "R40")):
                            total = 0.0
                            for v in vals[:, col]:
                                total += float(v)
                            result["coco"][c][m][kind][d] = total / len(vals)
        self.result = result

    def summary(self, r11=False):
        """The usual text block, one line per (overlap set, class, AP kind), the metrics in the order asked for:
        `Car AP_R40@0.70, 0.70: bev: 89.1000, 85.2000, 80.3000  3d: ...` (R40 only unless r11); the header holds one minimum
        overlap per metric other than aos (aos's own when it is the only one)."""
        if self.result is None:
            self.compute()
        lines = []
        for o in self.overlaps:
            for c in self.classes:
                for kind in (("R11", "R40") if r11 else ("R40",)):
                    parts = "  ".join(f"{m}: " + ", ".join(f"{v:.4f}" for v in self.result[o][c][m][kind]) for m in self.metrics)
                    if o == "coco":
                        lines.append(f"{c} {coco_header(c, kind)}: {parts}")
                        continue
                    t = ", ".join(f"{min_overlap(o, c, m):.2f}" for m in ([m for m in self.metrics if m != "aos"] or ["aos"]))
                    lines.append(f"{c} AP_{kind}@{t}: {parts}")
        return "\n".join(lines)

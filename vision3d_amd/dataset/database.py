"""The GT-sampling database built on the device (reference: vision3d/dataset/augmentation.py:201-243 `DatabaseBuilder`, with
the `create_annotations` / `numpify_objects` part of vision3d/dataset/kitti_dataset.py:64-87).

    annotations = build_annotations("KITTI/training", ids)          # {idx: dict(velo_path, calib, idx, boxes, class_idx)}
    DatabaseBuilder(cfg, annotations)                               # writes cfg.DATA.CACHEDIR/database.pkl unless it exists
    db = SampleDatabase.from_frames(frames, cfg.NUM_CLASSES, 8)     # or straight to the device form, no pickle in between

What runs where.  The reference tests every frame's points against its boxes in numpy (an (N, G) mask, G boolean gathers, G
subtractions: "~10 ms for each scene").  Here a BATCH of frames goes through `v3d_database_extract` (csrc/database.hip): three
launches per batch, the kept boxes' points written in point order, de-meaned, in the concatenated layout `SampleDatabase` keeps.
One host read per batch (the ragged sizes).

What stays on the host, and why.  The inside test is the reference's float64 test on corners built from cos / sin of the yaw;
annotation boxes are float64 (`boxes_in_lidar_frame`), and the device's double cos / sin need not equal the libm's that numpy
calls -- a corner one ulp off flips a point that lies on an edge.  `box_prep` therefore evaluates, in numpy with the reference's
expressions in the dtype of the boxes, one row per box (cos yaw, sin yaw, x, y, w, l, z - h / 2, z + h / 2); the kernel builds the
corners from it as (c lx + (-s) ly) + x.  That multiply-add form equals the reference's `einsum` corners in every coordinate
(tests/test_host_database.py compares it with corners recorded from the reference), so the rows carry cos / sin and not corners.
The pickle keeps the reference's dtypes (float64 rows for float64 boxes): the host forms them from the device's `src_index`
with the reference's own subtraction, so only indices cross the bus.
"""
import os
import pickle
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import _lib as L
from . import kitti as K

MAX_BOXES_PER_FRAME = 256  # V3D_DATABASE_MAX_BOXES
FLAG_OVERFLOW, FLAG_LIMIT = 1, 2


def box_prep(boxes):
    """(n, 7) boxes (x, y, z, w, l, h, yaw), float64 or float32 -> (n, 8) float64 rows (cos yaw, sin yaw, x, y, w, l, zlo, zhi),
    every value computed in the dtype of `boxes` (geometry.py:18-19, :36-37) and then widened."""
    boxes = np.asarray(boxes)
    if boxes.dtype not in (np.float32, np.float64):
        boxes = boxes.astype(np.float64)
    boxes = boxes.reshape(-1, 7)
    yaw, z, h = boxes[:, 6], boxes[:, 2], boxes[:, 5]
    cols = (np.cos(yaw), np.sin(yaw), boxes[:, 0], boxes[:, 1], boxes[:, 3], boxes[:, 4], z - h / 2, z + h / 2)
    return np.stack([np.asarray(c, np.float64) for c in cols], 1) if len(boxes) else np.zeros((0, 8), np.float64)


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def extract_objects(frames, min_pts, cap=None):
    """The objects of a list of frames, each `dict(points (N, C) float32, boxes (G, 7), class_idx (G,))` of numpy arrays or cuda
    tensors (what `load_frame` returns): every box holding more than `min_pts` points, frames in list order, boxes in annotation
    order.  -> device tensors (points (sum P, C) float32 de-meaned in xy, sizes (K,) int32, boxes (K, 7) in the dtype of the
    annotation boxes with xy zeroed, class_idx (K,) int64, frame (K,) int64, box_row (K,) int64 = row inside its frame,
    src_index (sum P,) int64 = row inside its frame's points).  `cap`: rows to provide for at first (default: a quarter of the
    points); a result that does not fit is extracted once more at its exact size."""
    frames = list(frames)
    F = len(frames)
    points = [f["points"] for f in frames]
    L.require_gpu("database_extract", *[p for p in points if isinstance(p, torch.Tensor)])
    dev = next((p.device for p in points if isinstance(p, torch.Tensor)), torch.device("cuda", torch.cuda.current_device()))
    C = int(points[0].shape[1]) if F else 4
    n_pts = [int(p.shape[0]) for p in points]
    boxes_host = [_host(f["boxes"]).reshape(-1, 7) for f in frames]
    n_box = [len(b) for b in boxes_host]
    if any(int(p.shape[1]) != C for p in points) or any(len(_host(f["class_idx"])) != g for f, g in zip(frames, n_box)):
        raise RuntimeError("database_extract: frames differ in point columns, or class_idx does not match boxes")
    if max(n_box, default=0) > MAX_BOXES_PER_FRAME:
        raise RuntimeError(f"database_extract: a frame holds {max(n_box)} boxes, at most {MAX_BOXES_PER_FRAME} per frame are supported")
    f32 = all(b.dtype == np.float32 for b in boxes_host)
    boxes_all = np.concatenate([b.astype(np.float32 if f32 else np.float64, copy=False) for b in boxes_host]) if F else np.zeros((0, 7))
    prep = np.concatenate([box_prep(b) for b in boxes_host]) if F else np.zeros((0, 8))
    cls_all = np.concatenate([_host(f["class_idx"]).astype(np.int64).reshape(-1) for f in frames]) if F else np.zeros(0, np.int64)
    p_off = np.concatenate([[0], np.cumsum(n_pts)]).astype(np.int32)
    b_off = np.concatenate([[0], np.cumsum(n_box)]).astype(np.int32)
    N, G = int(p_off[-1]), int(b_off[-1])
    with L.device_guard(dev):
        if all(isinstance(p, np.ndarray) for p in points):
            pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(points), np.float32) if F else np.zeros((0, C), np.float32)).to(dev)
        else:
            pts = torch.cat([torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(dev) if isinstance(p, np.ndarray)
                             else L.as_f32("database_extract", p) for p in points])
        small = torch.from_numpy(np.concatenate([p_off, b_off])).to(dev)
        p_off_d, b_off_d = small[:F + 1], small[F + 1:]
        prep_d = torch.from_numpy(prep).to(dev)
        counts = torch.empty(G, dtype=torch.int32, device=dev)
        starts = torch.empty(G, dtype=torch.int32, device=dev)
        totals = torch.empty(3, dtype=torch.int32, device=dev)
        work_bytes = int(L.lib().v3d_database_work_bytes(N, G, F))
        work = torch.empty((work_bytes + 3) // 4, dtype=torch.int32, device=dev)
        cap = max(4096, N // 4) if cap is None else int(cap)
        for attempt in range(2):
            out = torch.empty((cap, C), dtype=torch.float32, device=dev)
            src = torch.empty(cap, dtype=torch.int32, device=dev)
            L.check(L.lib().v3d_database_extract(L.ptr(pts), N, C, L.ptr(p_off_d), L.ptr(prep_d), G, L.ptr(b_off_d), F, int(min_pts),
                                                 L.ptr(counts), L.ptr(starts), L.ptr(src), L.ptr(out), cap, L.ptr(totals), L.ptr(work),
                                                 work_bytes, L.stream_ptr()), "database_extract")
            kept, rows, flags = (int(v) for v in totals.cpu().numpy())  # the one host read of the batch
            if flags & FLAG_LIMIT:
                raise RuntimeError(f"database_extract: a frame holds more than {MAX_BOXES_PER_FRAME} boxes")
            if not flags & FLAG_OVERFLOW:
                break
            cap = rows
        box_row_all = torch.nonzero(starts >= 0).reshape(-1)
        frame_of_box = torch.from_numpy(np.repeat(np.arange(F, dtype=np.int64), n_box)).to(dev)
        sizes = counts[box_row_all]
        boxes = torch.from_numpy(boxes_all).to(dev)[box_row_all]
        boxes[:, :2] *= 0  # `0 * center` (augmentation.py:226)
        frame = frame_of_box[box_row_all]
        src_index = src[:rows].long() - p_off_d.long()[frame].repeat_interleave(sizes.long(), output_size=rows)
        return (out[:rows], sizes, boxes, torch.from_numpy(cls_all).to(dev)[box_row_all], frame,
                box_row_all - b_off_d.long()[frame], src_index)


def sample_database_from_frames(cls, frames, num_classes, min_pts):
    """`SampleDatabase.from_frames`: the device form of the database straight from annotated frames (grouped by class on the
    device; objects of class -1 -- Tram, Truck, Misc -- are dropped: `draw_samples` never draws them)."""
    points, sizes, boxes, class_idx, _, _, _ = extract_objects(frames, min_pts)
    starts = torch.cumsum(sizes.long(), 0) - sizes.long()
    db = cls.__new__(cls)
    db.points, db.offsets, db.sizes, db.boxes = [], [], [], []
    for c in range(num_classes):
        sel = torch.nonzero(class_idx == c).reshape(-1)
        n = sizes[sel].long()
        total = int(n.sum())
        first = torch.cumsum(n, 0) - n
        rows = torch.arange(total, device=points.device) + (starts[sel] - first).repeat_interleave(n, output_size=total)
        n_host = n.cpu().numpy().astype(np.int64)
        db.sizes.append(n_host)
        db.offsets.append(np.concatenate([[0], np.cumsum(n_host)]))
        db.points.append(points[rows])
        db.boxes.append(boxes[sel].float())
    return db


def build_annotations(root, ids, reduced=True):
    """{idx: dict(velo_path, calib, idx, boxes (n, 7) float64 in the lidar frame, class_idx (n,))} for the frames `ids` of a KITTI
    `training` directory: label_2 + calib through this package's readers (kitti_dataset.py:64-87; the field names are the
    reference's, so its cached train.pkl is accepted by `DatabaseBuilder` as well)."""
    annotations = {}
    for idx in ids:
        idx = int(idx)
        name = f"{idx:06d}"
        calib = K.read_calib(os.path.join(root, "calib", name + ".txt"))
        labels = K.read_labels(os.path.join(root, "label_2", name + ".txt"))
        annotations[idx] = dict(velo_path=os.path.join(root, "velodyne_reduced" if reduced else "velodyne", name + ".bin"),
                                calib=calib, idx=idx, boxes=K.boxes_in_lidar_frame(labels, calib), class_idx=labels.class_idx)
    return annotations


class DatabaseBuilder:
    """Builds the cached database for SampleAugmentation (augmentation.py:201-243): `DatabaseBuilder(cfg, annotations)` returns
    at once if cfg.DATA.CACHEDIR/database.pkl exists, else writes {class_idx: [dict(points (n, 4), box (7,)), ...]} -- items in
    frame-then-box order, key -1 included, dtypes as numpy's promotions give them upstream."""

    def __init__(self, cfg, annotations, batch_frames=64, workers=8):
        self.cfg = cfg
        self.batch_frames, self.workers = int(batch_frames), max(1, min(int(workers), 16))
        self.fpath = os.path.join(cfg.DATA.CACHEDIR, "database.pkl")
        if os.path.isfile(self.fpath):
            print(f"Found cached database: {self.fpath}")
            return
        self._build(annotations)

    def _build(self, annotations):
        database = {}
        items = list(annotations.values())
        with ThreadPoolExecutor(self.workers) as pool:
            for b0 in range(0, len(items), self.batch_frames):
                batch = items[b0:b0 + self.batch_frames]
                clouds = list(pool.map(lambda it: K.read_points(it["velo_path"]), batch))
                for key, val in self._process_batch(batch, clouds):
                    database.setdefault(key, []).append(val)
        with open(self.fpath, "wb") as f:
            pickle.dump(database, f)

    def _process_batch(self, batch, clouds):
        """-> [(class_idx, dict(points, box))] of the batch's kept objects.  The device decides which rows belong to which box;
        the rows themselves are taken from the host's copy of the cloud with the reference's subtraction (:219-227)."""
        frames = [dict(points=p, boxes=it["boxes"], class_idx=it["class_idx"]) for it, p in zip(batch, clouds)]
        _, sizes, _, class_idx, frame, box_row, src_index = extract_objects(frames, self.cfg.AUG.MIN_NUM_SAMPLE_PTS)
        sizes, class_idx, frame, box_row, src_index = (t.cpu().numpy() for t in (sizes, class_idx, frame, box_row, src_index))
        out, first = [], 0
        for n, c, f, g in zip(sizes, class_idx, frame, box_row):
            p = clouds[f][src_index[first:first + n]]
            box = np.asarray(batch[f]["boxes"])[g]
            first += n
            out.append((int(c), dict(points=np.concatenate((p[:, :2] - box[:2], p[:, 2:]), 1), box=np.concatenate((0 * box[:2], box[2:])))))
        return out

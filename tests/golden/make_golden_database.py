"""Golden vectors for the GT-sampling database builder, captured from the REFERENCE itself: vision3d/dataset/augmentation.py
`DatabaseBuilder` (:201-243) with core/geometry.py `PointsInCuboids`, and -- for the `kitti` case -- the annotation part of
vision3d/dataset/kitti_dataset.py `AnnotationLoader` (:15-87).  Run in the build container only; the reference files are
imported by path through make_golden.py's loader (tqdm stubbed as in make_golden_aug.py).  This part of the reference is pure
numpy: neither a GPU nor its compiled extension is needed, so the extension is not built here.

    python tests/golden/make_golden_database.py      ->  tests/golden/database.npz      (only DATA is written; < 1 MiB)

Every case is a list of frames written as a small KITTI tree into a temporary directory and handed to the reference's builder;
stored are the inputs the reference saw ({tag}_n frames; {tag}_f{i}_points float32, _boxes, _class_idx, _corners = the
reference's `box3d_to_bev_corners`), the unpickled database per class key ({tag}_db_keys in the pickle's key order;
{tag}_db{c}_points / _sizes / _boxes, dtypes as pickled) and the class of every kept object in the builder's own order, frame
then box ({tag}_kept_class, {tag}_kept_frame: from the reference's `_process_item`, called once more per frame), plus min_pts.

Cases, chosen so that the reference alone exercises every rule:
  synth    4 frames make_cloud(seed, 16384) / make_gt_boxes(seed), seeds 0-3, float64 boxes with 0.123456789012345 added to every
           yaw (float64 cos / sin matter), class indices 0, 1, 2, -1 in turn.  Asserted: >= 8 boxes kept, >= 3 non-empty boxes
           dropped, a box with exactly min_pts points (dropped: the comparison is strict) and one with min_pts + 1 (kept), an object
           of class -1 kept.
  kitti    the three frames of tests/golden/kitti.npz (label text, calib text, points) through the reference's AnnotationLoader
           ('train' split: annotations -> float64 lidar boxes -> database).  Those clouds were made for the file readers --
           uniform noise, a few points per box -- so eleven points are placed inside each of the first two boxes of frames 0
           and 2 (seeded, appended behind the cloud); asserted: >= 2 objects kept.
  overlap  a frame with two overlapping boxes (a point inside both goes to both: asserted), a frame without boxes, a frame
           without points.
  f32      one synth frame with float32 boxes (what the augmentation's own callers pass).
Size: a cloud is thinned BEFORE the reference runs on it, order kept: every point within 4 m (BEV) of a box centre, and every
16th of the others.  What is stored is what the reference saw."""
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402

from vision3d_amd import synth  # noqa: E402

MIN_PTS = 8
YAW_OFFSET = 0.123456789012345


def thin(points, boxes):
    near = np.zeros(len(points), bool)
    for b in np.asarray(boxes, np.float64).reshape(-1, 7):
        near |= np.hypot(points[:, 0] - b[0], points[:, 1] - b[1]) < 4.0
    keep = near.copy()
    keep[np.flatnonzero(~near)[::16]] = True
    return np.ascontiguousarray(points[keep])


def points_inside(rng, box, n):
    """n points well inside a (x, y, z, w, l, h, yaw) box."""
    local = rng.uniform(-0.4, 0.4, (n, 3)) * box[3:6]
    c, s = np.cos(box[6]), np.sin(box[6])
    xy = local[:, :2] @ np.array([[c, s], [-s, c]]) + box[:2]
    return np.concatenate([xy, local[:, 2:3] + box[2], rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)


def load_reference():
    G.install_stubs(None)
    pkg = types.ModuleType("vision3d.dataset")
    pkg.__path__ = [G.REF + "/vision3d/dataset"]
    sys.modules["vision3d.dataset"] = pkg
    sys.modules.setdefault("tqdm", types.ModuleType("tqdm")).tqdm = lambda x, **k: x
    sys.modules["vision3d.ops"].box_iou_rotated = None  # imported by augmentation.py, used by the collision filter only
    sys.modules["vision3d.core"].ProposalTargetAssigner = None  # imported by kitti_dataset.py, used by the train dataset only
    geo = G.load_file("vision3d.core.geometry")
    aug = G.load_file("vision3d.dataset.augmentation")
    kd = G.load_file("vision3d.dataset.kitti_dataset")
    return geo, aug, kd


def make_cfg(root, cache):
    ns = types.SimpleNamespace
    return ns(DATA=ns(ROOTDIR=root, CACHEDIR=cache), AUG=ns(MIN_NUM_SAMPLE_PTS=MIN_PTS))


def write_cloud(root, idx, points):
    os.makedirs(os.path.join(root, "velodyne_reduced"), exist_ok=True)
    path = os.path.join(root, "velodyne_reduced", f"{idx:06d}.bin")
    np.asarray(points, np.float32).tofile(path)
    return path


def record(out, tag, geo, aug, cfg, annotations):
    """Runs the reference's builder on `annotations` and stores inputs + result; -> per-box counts per frame, kept classes."""
    builder = aug.DatabaseBuilder(cfg, annotations)
    with open(builder.fpath, "rb") as f:
        db = pickle.load(f)
    kept_class, kept_frame, counts = [], [], []
    out[f"{tag}_n"] = np.array(len(annotations))
    for i, item in enumerate(annotations.values()):
        points = np.fromfile(item["velo_path"], np.float32).reshape(-1, 4)
        out[f"{tag}_f{i}_points"], out[f"{tag}_f{i}_boxes"] = points, np.asarray(item["boxes"])
        out[f"{tag}_f{i}_class_idx"] = np.asarray(item["class_idx"], np.int64)
        out[f"{tag}_f{i}_corners"] = geo.box3d_to_bev_corners(item["boxes"])
        counts.append(np.array([len(p) for p in geo.PointsInCuboids(points)(item["boxes"])], np.int64))
        cls, samples = builder._process_item(item)
        cls = [int(c) for c in cls]
        kept_class += cls
        kept_frame += [i] * len(cls)
    out[f"{tag}_kept_class"], out[f"{tag}_kept_frame"] = np.array(kept_class, np.int64), np.array(kept_frame, np.int64)
    out[f"{tag}_db_keys"] = np.array([int(k) for k in db], np.int64)
    for k, items in db.items():
        out[f"{tag}_db{int(k)}_points"] = np.concatenate([it["points"] for it in items])
        out[f"{tag}_db{int(k)}_sizes"] = np.array([len(it["points"]) for it in items], np.int64)
        out[f"{tag}_db{int(k)}_boxes"] = np.stack([it["box"] for it in items])
    assert sum(len(v) for v in db.values()) == len(kept_class) == sum(int((c > MIN_PTS).sum()) for c in counts)
    print(tag, "frames", len(annotations), "kept", len(kept_class), "classes", sorted(int(k) for k in db),
          "points", {int(k): int(sum(len(it["points"]) for it in v)) for k, v in db.items()})
    return counts, kept_class


def synth_frame(seed, dtype):
    boxes = synth.make_gt_boxes(seed).astype(np.float64)
    boxes[:, 6] += YAW_OFFSET
    boxes = boxes.astype(dtype)
    return thin(synth.make_cloud(seed, 16384), boxes), boxes


def main():
    geo, aug, kd = load_reference()
    out = {"min_pts": np.array(MIN_PTS)}

    # ---- synth
    root = tempfile.mkdtemp(prefix="v3d_db_synth_")
    annotations = {}
    for seed in range(4):
        points, boxes = synth_frame(seed, np.float64)
        cls = np.array([(0, 1, 2, -1)[(g + seed) % 4] for g in range(len(boxes))], np.int64)
        annotations[seed] = dict(velo_path=write_cloud(root, seed, points), boxes=boxes, class_idx=cls, idx=seed)
    counts, kept_class = record(out, "synth", geo, aug, make_cfg(root, root), annotations)
    counts = np.concatenate(counts)
    assert (counts > MIN_PTS).sum() >= 8 and ((counts > 0) & (counts <= MIN_PTS)).sum() >= 3, counts
    assert (counts == MIN_PTS).any() and (counts == MIN_PTS + 1).any(), counts
    assert -1 in kept_class and {0, 1, 2} <= set(kept_class), kept_class
    for seed in range(4):  # the thinning kept every point that lies inside a box
        full = np.array([len(p) for p in geo.PointsInCuboids(synth.make_cloud(seed, 16384))(annotations[seed]["boxes"])])
        assert np.array_equal(full, counts[sum(len(annotations[s]["boxes"]) for s in range(seed)):][:len(full)])

    # ---- kitti: label / calib text -> the reference's AnnotationLoader -> DatabaseBuilder
    k = np.load(os.path.join(HERE, "kitti.npz"))
    root = tempfile.mkdtemp(prefix="v3d_db_kitti_")
    for d in ("label_2", "calib", "velodyne_reduced"):
        os.makedirs(os.path.join(root, d))
    rng = np.random.default_rng(2024)
    for i in range(3):
        boxes = k[f"c{i}_boxes"]
        points = thin(k[f"c{i}_points"], boxes)
        if i != 1:
            points = np.concatenate([points] + [points_inside(rng, boxes[g], 11) for g in range(2)])
        open(os.path.join(root, "label_2", f"{i:06d}.txt"), "w").write(str(k[f"c{i}_label_txt"]))
        open(os.path.join(root, "calib", f"{i:06d}.txt"), "w").write(str(k[f"c{i}_calib_txt"]))
        write_cloud(root, i, points)
    cache = os.path.join(root, "cache")
    loader = kd.AnnotationLoader(make_cfg(root, cache), [0, 1, 2], "train")  # (builds database.pkl: `record` finds it cached)
    for i in range(3):
        np.testing.assert_array_equal(loader.annotations[i]["boxes"], k[f"c{i}_boxes"])
    counts, kept_class = record(out, "kitti", geo, aug, make_cfg(root, cache), loader.annotations)
    assert len(kept_class) >= 2

    # ---- overlap / no boxes / no points
    root = tempfile.mkdtemp(prefix="v3d_db_overlap_")
    cloud = synth.make_cloud(7, 16384)
    counts7 = [len(p) for p in geo.PointsInCuboids(cloud)(synth.make_gt_boxes(7).astype(np.float64)[:12])]
    car = synth.make_gt_boxes(7).astype(np.float64)[int(np.argmax(counts7))][None]
    two = np.concatenate([car, car + np.array([0.6, 0.3, 0.0, 0.2, 0.1, 0.0, 0.35])])
    other = synth.make_gt_boxes(8).astype(np.float64)[:2]
    annotations = {
        0: dict(velo_path=write_cloud(root, 0, thin(cloud, two)), boxes=two, class_idx=np.array([0, 2]), idx=0),
        1: dict(velo_path=write_cloud(root, 1, thin(synth.make_cloud(8, 16384), other)[::4]), boxes=np.zeros((0, 7)),
                class_idx=np.zeros(0, np.int64), idx=1),
        2: dict(velo_path=write_cloud(root, 2, np.zeros((0, 4), np.float32)), boxes=other, class_idx=np.array([1, 0]), idx=2),
    }
    counts, kept_class = record(out, "overlap", geo, aug, make_cfg(root, root), annotations)
    mask = geo.PointsInCuboids(out["overlap_f0_points"])._get_mask(two)
    assert len(kept_class) == 2 and mask.all(1).any(), (kept_class, mask.sum(0))

    # ---- float32 boxes
    root = tempfile.mkdtemp(prefix="v3d_db_f32_")
    points, boxes = synth_frame(4, np.float32)
    annotations = {0: dict(velo_path=write_cloud(root, 0, points), boxes=boxes, class_idx=np.zeros(len(boxes), np.int64), idx=0)}
    counts, kept_class = record(out, "f32", geo, aug, make_cfg(root, root), annotations)
    assert len(kept_class) >= 3 and out["f32_db0_points"].dtype == np.float32 and out["synth_db0_points"].dtype == np.float64

    path = os.path.join(HERE, "database.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{path}: {size} bytes")
    assert size < (1 << 20), size


if __name__ == "__main__":
    main()

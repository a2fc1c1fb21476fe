"""GPU: the GT-sampling database built on the device (csrc/database.hip, vision3d_amd/dataset/database.py) against vectors
recorded from the reference's own DatabaseBuilder (tests/golden/make_golden_database.py -> tests/golden/database.npz).
Comparisons are EXACT: the inside test is the reference's float64 test on corners built from the same host-evaluated cos / sin,
and a de-meaned coordinate is one correctly rounded float64 subtraction -- a row that differs is a defect, not noise."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host_database import CASES, case_frames, write_kitti_tree  # noqa: E402

from vision3d_amd import _lib as L  # noqa: E402
from vision3d_amd import synth  # noqa: E402
from vision3d_amd.core.config import _defaults, second_car_cfg  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("points", "sizes", "boxes", "class_idx", "frame", "box_row", "src_index")


@pytest.fixture(scope="module")
def golden_db():
    return np.load(os.path.join(HERE, "golden", "database.npz"))


def golden_dict(g, tag):
    """{class: [dict(points, box), ...]} as the reference pickled it, keys in the pickle's order."""
    db = {}
    for c in g[f"{tag}_db_keys"].tolist():
        sizes = g[f"{tag}_db{c}_sizes"]
        pts = np.split(g[f"{tag}_db{c}_points"], np.cumsum(sizes)[:-1])
        db[c] = [dict(points=p, box=b) for p, b in zip(pts, g[f"{tag}_db{c}_boxes"])]
    return db


def golden_objects(g, tag):
    """The kept objects in the builder's order (frame, then box): [(class, points, box)]."""
    db, taken, out = golden_dict(g, tag), {}, []
    for c in g[f"{tag}_kept_class"].tolist():
        i = taken.get(c, 0)
        taken[c] = i + 1
        out.append((c, db[c][i]["points"], db[c][i]["box"]))
    assert all(taken[c] == len(db[c]) for c in db)
    return out


def extract(frames, min_pts, **kw):
    from vision3d_amd.dataset import extract_objects
    res = extract_objects(frames, min_pts, **kw)
    assert all(t.is_cuda for t in res)
    return {n: t.cpu().numpy() for n, t in zip(NAMES, res)}


def per_frame(res, n_frames):
    """The result of a batch cut into its frames: [(points, sizes, boxes, class_idx, box_row, src_index)]."""
    first = np.concatenate([[0], np.cumsum(res["sizes"])])
    out = []
    for f in range(n_frames):
        sel = np.flatnonzero(res["frame"] == f)
        rows = np.concatenate([np.arange(first[k], first[k + 1]) for k in sel]) if len(sel) else np.zeros(0, np.int64)
        out.append((res["points"][rows], res["sizes"][sel], res["boxes"][sel], res["class_idx"][sel], res["box_row"][sel],
                    res["src_index"][rows]))
    return out


def assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, (x.dtype, y.dtype, x.shape, y.shape)
        np.testing.assert_array_equal(x, y)


def case_cfg(cachedir, min_pts, base=_defaults):
    cfg = base().clone()
    cfg.merge_from_dict(dict(DATA=dict(CACHEDIR=str(cachedir)), AUG=dict(MIN_NUM_SAMPLE_PTS=int(min_pts))))
    return cfg


# ---- 1
@pytest.mark.parametrize("tag", CASES)
def test_extract_objects_equals_the_reference(golden_db, tag):
    g = golden_db
    frames, objs = case_frames(g, tag), golden_objects(g, tag)
    res = extract(frames, int(g["min_pts"]))
    np.testing.assert_array_equal(res["sizes"], [len(p) for _, p, _ in objs])
    np.testing.assert_array_equal(res["class_idx"], [c for c, _, _ in objs])
    np.testing.assert_array_equal(res["frame"], g[f"{tag}_kept_frame"])
    want_boxes = np.stack([b for _, _, b in objs])
    assert res["boxes"].dtype == want_boxes.dtype
    np.testing.assert_array_equal(res["boxes"], want_boxes)
    assert res["points"].dtype == np.float32
    np.testing.assert_array_equal(res["points"], np.concatenate([p for _, p, _ in objs]).astype(np.float32))
    # kept-box order: the box of every object is its frame's annotation box with the centre taken out
    first = 0
    for k, (f, r, n) in enumerate(zip(res["frame"], res["box_row"], res["sizes"])):
        np.testing.assert_array_equal(frames[f]["boxes"][r][2:], want_boxes[k][2:])
        src = res["src_index"][first:first + n]
        assert (np.diff(src) > 0).all()  # point order
        np.testing.assert_array_equal(frames[f]["points"][src][:, 2:], res["points"][first:first + n][:, 2:])
        first += n
    # device tensors in -> the same
    dev_frames = [{k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in fr.items()} for fr in frames]
    res2 = extract(dev_frames, int(g["min_pts"]))
    assert_same([res[n] for n in NAMES], [res2[n] for n in NAMES])


# ---- 2
@pytest.mark.parametrize("batch_frames", [64, 2])
@pytest.mark.parametrize("tag", CASES)
def test_database_builder_writes_the_reference_pickle(golden_db, tmp_path, tag, batch_frames):
    from vision3d_amd.dataset import DatabaseBuilder
    g = golden_db
    annotations = {}
    for i, fr in enumerate(case_frames(g, tag)):
        path = str(tmp_path / f"{i:06d}.bin")
        fr["points"].tofile(path)
        annotations[10 + i] = dict(velo_path=path, boxes=fr["boxes"], class_idx=fr["class_idx"], idx=10 + i)
    cfg = case_cfg(tmp_path, g["min_pts"])
    builder = DatabaseBuilder(cfg, annotations, batch_frames=batch_frames)
    assert builder.fpath == str(tmp_path / "database.pkl")
    with open(builder.fpath, "rb") as f:
        db = pickle.load(f)
    want = golden_dict(g, tag)
    assert list(db) == list(want), "keys in first-appearance order, -1 included"
    if tag in ("synth", "kitti"):
        assert -1 in db
    for c in want:
        assert len(db[c]) == len(want[c])
        for a, b in zip(db[c], want[c]):
            assert set(a) == {"points", "box"}
            assert_same([a["points"], a["box"]], [b["points"], b["box"]])
    stamp = os.stat(builder.fpath).st_mtime_ns
    DatabaseBuilder(cfg, {0: dict(velo_path="/nonexistent", boxes=None, class_idx=None)})  # cached: nothing is read or written
    assert os.stat(builder.fpath).st_mtime_ns == stamp


# ---- 3
def test_sample_database_from_frames_and_augmentation(golden_db):
    from vision3d_amd.dataset import ChainedAugmentation, SampleDatabase
    g, tag = golden_db, "synth"
    frames = case_frames(g, tag)
    cfg = _defaults().clone()
    got = SampleDatabase.from_frames(frames, cfg.NUM_CLASSES, int(g["min_pts"]))
    want = SampleDatabase(golden_dict(g, tag), cfg.NUM_CLASSES)
    assert len(got) == len(want) == 3
    for c in range(3):
        assert got.count(c) == want.count(c) > 0
        np.testing.assert_array_equal(got.sizes[c], want.sizes[c])
        np.testing.assert_array_equal(got.offsets[c], want.offsets[c])
        for a, b in ((got.points[c], want.points[c]), (got.boxes[c], want.boxes[c])):
            assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape and a.is_cuda
            assert torch.equal(a, b), c
    scene = g["f32_f0_points"], g["f32_f0_boxes"][:9], np.zeros(9, np.int64)
    outs = []
    for db in (got, golden_dict(g, tag)):
        np.random.seed(123)
        outs.append(ChainedAugmentation(cfg, database=db)(*(a.copy() for a in scene)))
    assert outs[0][1].shape[0] > 9, "the case must paste at least one object"
    assert_same(outs[0], outs[1])


# ---- 4
def test_float32_boxes_agree_with_points_in_boxes(golden_db):
    from vision3d_amd.core.geometry import points_in_boxes_mask
    g = golden_db
    fr = case_frames(g, "f32")[0]
    assert fr["boxes"].dtype == np.float32
    res = extract([fr], 0)
    mask = points_in_boxes_mask(torch.from_numpy(fr["points"]).cuda(), torch.from_numpy(fr["boxes"]).cuda()).cpu().numpy()
    np.testing.assert_array_equal(res["box_row"], np.flatnonzero(mask.sum(0) > 0))
    first = 0
    for r, n in zip(res["box_row"], res["sizes"]):
        np.testing.assert_array_equal(res["src_index"][first:first + n], np.flatnonzero(mask[:, r]))
        first += n
    assert first == len(res["src_index"]) > 0


# ---- 5
def test_batches_are_independent_and_runs_identical(golden_db):
    g = golden_db
    frames, m = case_frames(g, "synth"), int(g["min_pts"])
    together = extract(frames, m)
    again = extract(frames, m)
    assert_same([together[n] for n in NAMES], [again[n] for n in NAMES])
    batch = per_frame(together, 4)
    backwards = per_frame(extract(frames[::-1], m), 4)[::-1]
    for f in range(4):
        alone = per_frame(extract([frames[f]], m), 1)[0]
        assert len(alone[1]) > 0
        assert_same(batch[f], alone)
        assert_same(batch[f], backwards[f])


# ---- 6
def raw_extract(frames, min_pts, cap, guard=0, fill=-7.0):
    """v3d_database_extract itself on `frames` with `guard` rows behind the `cap` rows of the two row buffers."""
    from vision3d_amd.dataset import box_prep
    n_pts, n_box = [len(f["points"]) for f in frames], [len(f["boxes"]) for f in frames]
    F, N, G = len(frames), sum(n_pts), sum(n_box)
    pts = torch.from_numpy(np.concatenate([f["points"] for f in frames])).cuda()
    prep = torch.from_numpy(np.concatenate([box_prep(f["boxes"]) for f in frames])).cuda()
    p_off = torch.from_numpy(np.concatenate([[0], np.cumsum(n_pts)]).astype(np.int32)).cuda()
    b_off = torch.from_numpy(np.concatenate([[0], np.cumsum(n_box)]).astype(np.int32)).cuda()
    counts, starts = (torch.full((G,), -99, dtype=torch.int32, device="cuda") for _ in range(2))
    out = torch.full((cap + guard, 4), fill, dtype=torch.float32, device="cuda")
    src = torch.full((cap + guard,), int(fill), dtype=torch.int32, device="cuda")
    totals = torch.full((3,), -99, dtype=torch.int32, device="cuda")
    wb = int(L.lib().v3d_database_work_bytes(N, G, F))
    work = torch.empty((wb + 3) // 4, dtype=torch.int32, device="cuda")
    code = L.lib().v3d_database_extract(L.ptr(pts), N, 4, L.ptr(p_off), L.ptr(prep), G, L.ptr(b_off), F, min_pts, L.ptr(counts),
                                        L.ptr(starts), L.ptr(src), L.ptr(out), cap, L.ptr(totals), L.ptr(work), wb, L.stream_ptr())
    torch.cuda.synchronize()
    return code, tuple(t.cpu().numpy() for t in (counts, starts, src, out, totals))


def test_capacity_overflow_is_reported_and_nothing_written_behind_cap(golden_db):
    g = golden_db
    frames, m = case_frames(g, "synth"), int(g["min_pts"])
    full = extract(frames, m)
    rows = len(full["points"])
    code, (counts, starts, src, out, totals) = raw_extract(frames, m, rows, guard=64)
    assert code == 0 and totals.tolist() == [len(full["sizes"]), rows, 0]
    np.testing.assert_array_equal(out[:rows], full["points"])
    assert (out[rows:] == -7.0).all() and (src[rows:] == -7).all()
    cap = rows // 2
    code, (counts2, starts2, src2, out2, totals2) = raw_extract(frames, m, cap, guard=rows)
    assert code == 0 and totals2.tolist() == [len(full["sizes"]), rows, 1], "overflow word set, the needed rows reported"
    np.testing.assert_array_equal(counts2, counts)
    np.testing.assert_array_equal(starts2, starts)
    assert (counts >= 0).all() and ((starts >= 0) == (counts > m)).all()
    np.testing.assert_array_equal(counts[starts >= 0], full["sizes"])
    np.testing.assert_array_equal(out2[:cap], full["points"][:cap])
    np.testing.assert_array_equal(src2[:cap], src[:cap])
    assert (out2[cap:] == -7.0).all() and (src2[cap:] == -7).all(), "rows behind cap keep their fill value"
    retried = extract(frames, m, cap=cap)  # the wrapper sizes exactly and repeats
    assert_same([full[n] for n in NAMES], [retried[n] for n in NAMES])


# ---- 7
def inside_float64(points, boxes):
    """(N, G) mask: strictly between the z limits and strictly left of all four edges of the counter-clockwise BEV rectangle,
    evaluated in float64 on the float32 points (cos / sin in the dtype of the boxes)."""
    b = np.asarray(boxes)
    c, s = np.cos(b[:, 6]).astype(np.float64), np.sin(b[:, 6]).astype(np.float64)
    b = b.astype(np.float64)
    ux, uy = np.array([-0.5, 0.5, 0.5, -0.5]), np.array([-0.5, -0.5, 0.5, 0.5])
    lx, ly = b[:, 3:4] * ux, b[:, 4:5] * uy
    cx = (c[:, None] * lx + (-s)[:, None] * ly) + b[:, 0:1]  # (G, 4)
    cy = (s[:, None] * lx + c[:, None] * ly) + b[:, 1:2]
    px, py, pz = (points[:, j:j + 1].astype(np.float64) for j in range(3))
    inside = (pz > (b[:, 2] - b[:, 5] / 2)[None]) & (pz < (b[:, 2] + b[:, 5] / 2)[None])
    for v in range(4):
        ex, ey = -(cx[:, v] - cx[:, v - 1]), -(cy[:, v] - cy[:, v - 1])
        inside &= ex[None] * (cy[None, :, v] - py) - ey[None] * (cx[None, :, v] - px) > 0
    return inside


def expected_objects(frames, min_pts):
    pts, sizes, frame, box_row, src = [], [], [], [], []
    for f, fr in enumerate(frames):
        mask = inside_float64(fr["points"], fr["boxes"])
        for gi in np.flatnonzero(mask.sum(0) > min_pts):
            idx = np.flatnonzero(mask[:, gi])
            rows = fr["points"][idx].copy()
            rows[:, :2] = (rows[:, :2].astype(np.float64) - np.asarray(fr["boxes"], np.float64)[gi, :2]).astype(np.float32)
            pts.append(rows), sizes.append(len(idx)), frame.append(f), box_row.append(gi), src.append(idx)
    return np.concatenate(pts), np.array(sizes), np.array(frame), np.array(box_row), np.concatenate(src)


def check_against_restatement(frames, min_pts, min_rows):
    res = extract(frames, min_pts)
    pts, sizes, frame, box_row, src = expected_objects(frames, min_pts)
    print(f"{len(frames)} frames, {sum(len(f['points']) for f in frames)} points, {sum(len(f['boxes']) for f in frames)} boxes -> "
          f"{len(sizes)} objects, {len(pts)} rows")
    assert len(pts) >= min_rows
    np.testing.assert_array_equal(res["sizes"], sizes)
    np.testing.assert_array_equal(res["frame"], frame)
    np.testing.assert_array_equal(res["box_row"], box_row)
    np.testing.assert_array_equal(res["src_index"], src)
    np.testing.assert_array_equal(res["points"], pts)


def test_one_large_frame():
    """120 000 points, 40 boxes: 59 chunks of one frame -- the per-box running sum over (chunk, wave) segments at length."""
    cloud, boxes = synth.make_cloud(3, 120000, synth.WAYMO_BOUNDS, fov_deg=180.0, az_steps=3000, n_cars=40, return_boxes=True)
    boxes = boxes.astype(np.float64)
    boxes[:, 6] += 0.123456789012345
    boxes[:, 3:6] *= 1.5  # (more points per box, the neighbours' ground included)
    check_against_restatement([dict(points=cloud, boxes=boxes, class_idx=np.zeros(len(boxes), np.int64))], 8, 2000)


def test_batch_of_64_kitti_size_frames():
    """64 x 16 384 points (about a million), 27 boxes each; a short frame and a frame without boxes in between."""
    frames, scenes = [], [(synth.make_cloud(s, 16384), synth.make_gt_boxes(s).astype(np.float64)) for s in range(8)]
    for seed in range(64):
        cloud, boxes = scenes[seed % 8][0], scenes[seed % 8][1].copy()
        boxes[:, 6] += 0.01 * seed
        if seed % 8:  # the same eight scenes, shifted: different coordinates, same density
            cloud = cloud + np.array([0.001 * seed, -0.002 * seed, 0, 0], np.float32)
            boxes[:, :2] += [0.001 * seed, -0.002 * seed]
        frames.append(dict(points=np.ascontiguousarray(cloud), boxes=boxes, class_idx=np.arange(len(boxes)) % 3))
    frames[5]["points"] = frames[5]["points"][:2049]
    frames[9] = dict(points=frames[9]["points"], boxes=np.zeros((0, 7)), class_idx=np.zeros(0, np.int64))
    check_against_restatement(frames, 8, 20000)


def boxes_on_a_grid(n, points_of, seed):
    """n boxes of 2 x 2 x 2 m, 4 m apart, any yaw; box g holds points_of(g) points (within 0.6 m of its centre: inside at every yaw)
    -> one frame."""
    rng = np.random.default_rng(seed)
    g = np.arange(n)
    boxes = np.stack([4.0 * (g % 16), 4.0 * (g // 16), np.zeros(n), *np.full((3, n), 2.0), rng.uniform(-3.0, 3.0, n)], 1)
    owner = np.repeat(g, [points_of(i) for i in g])
    pts = np.concatenate([boxes[owner, :3] + rng.uniform(-0.6, 0.6, (len(owner), 3)), rng.random((len(owner), 1))], 1)
    pts = pts[rng.permutation(len(pts))].astype(np.float32)
    return dict(points=pts, boxes=boxes, class_idx=np.zeros(n, np.int64))


def test_256_boxes_every_third_kept():
    """The scan over a frame's boxes (one thread per box, 256 = the limit): every third box holds 12 points and is kept, the others 3
    and are dropped, so the kept boxes' first rows (rel_start) carry the sums across all three wave edges."""
    frame = boxes_on_a_grid(256, lambda g: 12 if g % 3 == 0 else 3, 0)
    check_against_restatement([frame], 8, 86 * 12)


def test_batch_of_257_tiny_frames():
    """257 frames of one box each, 8 points (5 of 7 frames) or 3 (dropped): the sums over the frames (db_locate, the rows before a
    frame) take a second trip of 256 with a carry."""
    frames = [boxes_on_a_grid(1, lambda g, f=f: 3 if f % 7 in (2, 5) else 8, f) for f in range(257)]
    kept = sum(f % 7 not in (2, 5) for f in range(257))
    check_against_restatement(frames, 4, kept * 8)


# ---- 8
def test_limits_and_cpu_tensors_are_refused(golden_db):
    from vision3d_amd.dataset import extract_objects
    fr = case_frames(golden_db, "f32")[0]
    many = dict(points=fr["points"], boxes=np.tile(fr["boxes"][:1], (257, 1)), class_idx=np.zeros(257, np.int64))
    with pytest.raises(RuntimeError, match="at most 256"):
        extract_objects([many], 8)
    code, _ = raw_extract([many], 8, 16)
    assert code == -3 and b"unsupported" in L.lib().v3d_error_string(code)
    empty = dict(points=fr["points"][:0], boxes=fr["boxes"][:0], class_idx=np.zeros(0, np.int64))
    code, (counts, starts, _, out, totals) = raw_extract([many, empty], 8, 16)  # the entry point cannot see the per-frame count
    assert code == 0 and totals.tolist() == [0, 0, 2] and (counts == 0).all() and (starts == -1).all() and (out == -7.0).all()
    ok = dict(points=fr["points"], boxes=np.tile(fr["boxes"][:1], (256, 1)), class_idx=np.zeros(256, np.int64))
    res = extract([ok], 0)
    assert len(res["sizes"]) in (0, 256) and len(set(res["sizes"].tolist())) <= 1
    with pytest.raises(RuntimeError, match="GPU"):
        extract_objects([dict(points=torch.zeros(8, 4), boxes=fr["boxes"], class_idx=fr["class_idx"])], 8)
    wb = L.lib().v3d_database_work_bytes(100, 4, 1)
    assert wb > 0 and L.lib().v3d_database_work_bytes(-1, 4, 1) == 0
    assert L.lib().v3d_database_extract(0, 100, 4, 0, 0, 4, 0, 1, 8, 0, 0, 0, 0, ctypes.c_int64(0), 0, 0, 0, 0) == -1


# ---- the command line, end to end
def test_command_line_builds_a_database_the_augmentation_loads(golden_db, tmp_path, capsys):
    from vision3d_amd.dataset import ChainedAugmentation
    from vision3d_amd.dataset.__main__ import main
    g = golden_db
    root, cache = tmp_path / "training", tmp_path / "cache"
    write_kitti_tree(str(root), g)
    (tmp_path / "train.txt").write_text("000000\n000001\n000002\n")
    assert main(["--root", str(root), "--ids", str(tmp_path / "train.txt"), "--cachedir", str(cache), "--min-pts", str(int(g["min_pts"]))]) == 0
    lines = capsys.readouterr().out.splitlines()
    want = golden_dict(g, "kitti")
    assert f"Car: {len(want[0])} objects, {sum(len(it['points']) for it in want[0])} points" in lines
    with open(cache / "database.pkl", "rb") as f:
        db = pickle.load(f)
    assert list(db) == list(want)
    for c in want:
        for a, b in zip(db[c], want[c]):
            assert_same([a["points"], a["box"]], [b["points"], b["box"]])
    cfg = case_cfg(cache, g["min_pts"], second_car_cfg)
    aug = ChainedAugmentation(cfg)  # loads CACHEDIR/database.pkl
    assert aug.sample.database.count(0) == len(want[0])
    np.random.seed(5)
    boxes = g["f32_f0_boxes"][:4]
    p, b, c = aug(g["f32_f0_points"].copy(), boxes.copy(), np.zeros(4, np.int64))
    assert b.shape[0] > 4 and p.shape[1] == 4 and len(c) == b.shape[0]

"""GPU: KITTI BEV / 3-D AP on the device (csrc/kitti_eval.hip via vision3d_amd.evaluation) against the float64 restatement of
tests/kitti_eval_ref.py: overlaps, and per combo n_valid_gt, thresholds, (tp, fp, fn) and AP exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_eval_ref as R  # noqa: E402

from vision3d_amd.dataset import kitti as K  # noqa: E402
from vision3d_amd.evaluation import KittiEvaluator, camera_box_overlaps, write_kitti_results  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_eval(pairs, **kw):
    ev = KittiEvaluator(**kw)
    for g, d in pairs:
        ev.add_frame(g, d)
    return ev.compute(), ev.details, ev


def _assert_same(pairs, dev_res, dev_det, **kw):
    want_res, want_det = R.evaluate([R.make_frame(g, d) for g, d in pairs], **kw)
    for key, w in want_det.items():
        got = dev_det[key]
        assert got["n_valid_gt"] == w["n_valid_gt"], key
        assert np.array_equal(got["thresholds"], w["thresholds"]), key
        assert np.array_equal(got["counts"], w["counts"]), key
    assert dev_res == want_res


def test_overlaps_match_float64_clip():
    rng = np.random.default_rng(0)
    n_dt, n_gt = 160, 80
    gt = np.zeros((n_gt, 7))
    gt[:, 0], gt[:, 2] = rng.uniform(-3, 3, n_gt), rng.uniform(7, 13, n_gt)
    gt[:, 1], gt[:, 3] = rng.uniform(1, 2, n_gt), rng.uniform(0.5, 2, n_gt)
    gt[:, 4], gt[:, 5] = rng.uniform(0.4, 2.5, n_gt), rng.uniform(0.5, 5, n_gt)
    gt[:, 6] = rng.uniform(-2 * np.pi, 2 * np.pi, n_gt)
    dt = gt[rng.integers(0, n_gt, n_dt)].copy()
    dt[:, [0, 2]] += rng.normal(0, 0.8, (n_dt, 2))
    dt[:, 1] += rng.normal(0, 0.3, n_dt)
    dt[:, 3:6] *= rng.uniform(0.7, 1.3, (n_dt, 3))
    dt[:, 6] = rng.uniform(-2 * np.pi, 2 * np.pi, n_dt)
    dt[:8] = gt[:8]  # identical boxes
    dt[8, 4] = 0.0  # degenerate: zero width
    dt[9, 3] = 0.0  # zero height
    gt[10, 5] = 0.0  # zero length
    gt, dt = gt.astype(np.float32), dt.astype(np.float32)
    bev, d3 = camera_box_overlaps(torch.from_numpy(dt).cuda(), torch.from_numpy(gt).cuda())
    wb, w3 = R.overlaps(dt.astype(np.float64), gt.astype(np.float64))
    assert n_dt * n_gt >= 10000 and (wb > 0).sum() > 2000
    assert np.abs(bev.cpu().numpy() - wb).max() <= 1e-5
    assert np.abs(d3.cpu().numpy() - w3).max() <= 1e-5
    assert np.abs(np.diag(bev.cpu().numpy()[:8, :8]) - 1).max() <= 1e-5
    assert (bev.cpu().numpy()[8] == 0).all() and (d3.cpu().numpy()[9] == 0).all() and (bev.cpu().numpy()[:, 10] == 0).all()


@pytest.mark.parametrize("kind", ["all_found", "none_found", "fp_in_front", "van_under_car", "van_fp", "short_absorbed",
                                  "tall_not_absorbed", "height25"])
def test_hand_cases(kind):
    pairs = R.hand_case(kind)
    res, det, _ = _device_eval(pairs)
    _assert_same(pairs, res, det)


@pytest.fixture(scope="module")
def val_set():
    rng = np.random.default_rng(7)
    pairs = [R.synthetic_frame(rng, int(rng.integers(0, 16)), int(rng.integers(0, 5))) for _ in range(100)]
    pairs += [R.synthetic_frame(rng, 0, 3), R.synthetic_frame(rng, 5, 0), R.synthetic_frame(rng, 0, 0)]
    names = {n for g, d in pairs for n in g.names}
    assert names >= {"Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "DontCare", "Misc"}
    return pairs


def test_synthetic_val_set_matches_restatement(val_set):
    res, det, ev = _device_eval(val_set)
    _assert_same(val_set, res, det)
    assert sum(d["counts"][:, 0].sum() for d in det.values()) > 1000  # the set exercises the assignment
    assert any(v > 0 for o in res.values() for c in o.values() for m in c.values() for v in m["R40"])
    # bit-identical across runs and frame orders
    assert ev.compute() == res
    res2, det2, _ = _device_eval(val_set[::-1])
    assert res2 == res
    for k in det:
        assert np.array_equal(det[k]["thresholds"], det2[k]["thresholds"]) and np.array_equal(det[k]["counts"], det2[k]["counts"])


def test_edge_cases():
    rng = np.random.default_rng(11)
    # one frame with 1024 detections (10 per object) beside frames with no detections / no ground truth
    g, d = R.synthetic_frame(rng, 100, 24, dets_per_gt=10.0, spacing=12.0, grid=12)
    keep = min(len(d.names), 1024)
    sel = np.arange(keep)
    d = d._replace(names=[d.names[i] for i in sel], **{f: getattr(d, f)[sel] for f in
                                                        ("class_idx", "truncation", "occlusion", "alpha", "box2d", "hwl", "location",
                                                         "ry", "score", "level")})
    if keep < 1024:
        extra = R.synthetic_frame(rng, 0, 1024 - keep, grid=40)[1]  # false positives half a cell off the objects' grid
        extra = extra._replace(location=extra.location + np.array([6.0, 0.0, 0.0]))
        d = K.Labels(*[list(a) + list(b) if isinstance(a, list) else np.concatenate([a, b]) for a, b in zip(d, extra)])
    assert len(d.names) == 1024
    pairs = [(g, d), R.synthetic_frame(rng, 6, 0), R.synthetic_frame(rng, 0, 4)]
    res, det, _ = _device_eval(pairs)
    _assert_same(pairs, res, det)
    # a class with no valid ground truth: AP 0
    only_cars = R.hand_case("all_found")
    res, det, _ = _device_eval(only_cars)
    assert res["strict"]["Pedestrian"]["bev"]["R40"] == [0.0] * 3 and det[("strict", "Pedestrian", "bev", 1)]["n_valid_gt"] == 0
    assert res["strict"]["Car"]["3d"]["R40"] == [100.0] * 3
    # no frames at all
    assert KittiEvaluator().compute()["loose"]["Cyclist"]["3d"]["R11"] == [0.0] * 3


def test_over_the_limit_raises():
    rng = np.random.default_rng(12)
    g, d = R.synthetic_frame(rng, 2, 0, margins=False)
    big = R.make_labels(["Car"] * 1025, np.tile([0, 1.7, 10, 1.5, 1.6, 3.9, 0], (1025, 1)), np.tile([0, 0, 50, 50], (1025, 1)),
                        score=np.linspace(0, 1, 1025))
    ev = KittiEvaluator()
    ev.add_frame(g, big)
    with pytest.raises(RuntimeError, match="1024"):
        ev.compute()
    many = R.make_labels(["Car"] * 257, np.tile([0, 1.7, 10, 1.5, 1.6, 3.9, 0], (257, 1)), np.tile([0, 0, 50, 50], (257, 1)))
    ev = KittiEvaluator()
    ev.add_frame(many, d)
    with pytest.raises(RuntimeError, match="256"):
        ev.compute()


def _calib(seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.01, 0.01, 3)
    cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    r0 = (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
          np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])).astype(np.float32)
    v2c = np.array([[0.0, -1.0, 0.0, 0.02], [0.0, 0.0, -1.0, -0.08], [1.0, 0.0, 0.0, -0.27]], np.float32)
    c2v = np.zeros_like(v2c)
    c2v[:, :3] = v2c[:, :3].T
    c2v[:, 3] = -v2c[:, :3].T @ v2c[:, 3]
    p2 = np.array([[721.5, 0, 609.6, 44.9], [0, 721.5, 172.9, 0.2], [0, 0, 1, 0.003]], np.float32)
    return K.Calib(V2C=v2c, C2V=c2v, R0=r0, P2=p2, WH=np.r_[1224, 370])


def _clear_of_thresholds(gt, dt_labels):
    """indices of detections whose IoUs with every ground truth sit >= 1e-4 from every minimum overlap and whose 2-D height sits
    >= 1e-3 px from every MIN_HEIGHT (the two detection paths may differ by an ulp)."""
    bev, d3 = R.overlaps(R.camera_boxes(dt_labels), R.camera_boxes(gt))
    ok = np.ones(len(dt_labels.names), bool)
    for t in R.THRESHOLDS:
        ok &= (np.abs(bev - t) >= 1e-4).all(1) & (np.abs(d3 - t) >= 1e-4).all(1)
    h = np.abs(dt_labels.box2d[:, 3] - dt_labels.box2d[:, 1])
    for m in (25, 40):
        ok &= np.abs(h - m) >= 1e-3
    return np.nonzero(ok)[0]


def test_model_output_matches_result_files(tmp_path):
    """Second.inference -> add_frame(model tensors) gives the same dict as write_kitti_results -> read_labels -> add_frame(Labels),
    and the CLI on those files prints the same summary."""
    from vision3d_amd import synth
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    from vision3d_amd.core.config import second_car_cfg
    from vision3d_amd.detector import Second
    cfg = second_car_cfg()
    for a in cfg.ANCHORS:
        a["score_thresh"] = 0.0
    torch.manual_seed(0)
    model = Second(cfg).cuda().eval()
    anchors = AnchorGenerator(cfg).anchors.cuda()
    clouds = [synth.make_cloud(s, n_points=8192) for s in range(4)]
    with torch.no_grad():
        boxes, bidx, cidx, scores = model.inference(Preprocessor(cfg)(dict(points=clouds, anchors=anchors)))
    names = [a["names"][0] for a in cfg.ANCHORS]
    (tmp_path / "label_2").mkdir()
    (tmp_path / "results").mkdir()
    rng = np.random.default_rng(5)
    kept = []
    for b in range(len(clouds)):
        calib = _calib(b)
        m = bidx == b
        fb, fc, fs = boxes[m], cidx[m], scores[m]
        assert fb.shape[0] > 0, "the model emitted no detection for a frame"
        path = tmp_path / "results" / f"{b:06d}.txt"
        write_kitti_results(path, fb, fc, fs, calib, names)
        dt = K.read_labels(path)
        # ground truth: some of the detections themselves, jittered (so that matches happen), plus a few others
        cam = R.camera_boxes(dt)
        pick = rng.choice(len(cam), min(len(cam), 8), replace=False)
        g_cam = cam[pick] + np.c_[rng.normal(0, 0.2, (len(pick), 3)), np.zeros((len(pick), 4))]
        g_2d = np.tile([100.0, 100.0, 200.0, 170.0], (len(pick), 1))
        gt = R.make_labels(["Car"] * len(pick), g_cam, g_2d, np.zeros(len(pick)), np.zeros(len(pick), np.int64))
        with open(tmp_path / "label_2" / f"{b:06d}.txt", "w") as f:
            for k in range(len(pick)):
                x, yb, z, h, w, l, ry = g_cam[k]
                f.write(f"Car 0 0 0 {' '.join(f'{v:.9g}' for v in g_2d[k])} {h:.9g} {w:.9g} {l:.9g} {x:.9g} {yb:.9g} {z:.9g} {ry:.9g}\n")
        gt = K.read_labels(tmp_path / "label_2" / f"{b:06d}.txt")
        sel = _clear_of_thresholds(gt, dt)
        kept.append((gt, calib, fb[sel], fc[sel], fs[sel]))
        # rewrite the result file with the retained detections only
        write_kitti_results(path, fb[sel], fc[sel], fs[sel], calib, names)
    ev_model = KittiEvaluator(classes=("Car",), det_names=names)
    ev_file = KittiEvaluator(classes=("Car",))
    for b, (gt, calib, fb, fc, fs) in enumerate(kept):
        ev_model.add_frame(gt, (fb, fc, fs, calib))
        ev_file.add_frame(gt, K.read_labels(tmp_path / "results" / f"{b:06d}.txt"))
    got, want = ev_model.compute(), ev_file.compute()
    assert got == want
    assert sum(d["counts"][:, 0].sum() for d in ev_file.details.values()) > 0
    # the CLI prints the file evaluator's numbers (all three classes)
    ev_all = KittiEvaluator()
    for b, (gt, *_rest) in enumerate(kept):
        ev_all.add_frame(gt, K.read_labels(tmp_path / "results" / f"{b:06d}.txt"))
    out = subprocess.run([sys.executable, "-m", "vision3d_amd.evaluation", "--labels", str(tmp_path / "label_2"), "--results",
                          str(tmp_path / "results"), "--r11"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == ev_all.summary(r11=True).strip()
    assert "Car AP_R40@0.70, 0.70: bev: " in out.stdout

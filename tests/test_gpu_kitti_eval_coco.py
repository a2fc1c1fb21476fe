"""GPU: the COCO-style KITTI AP (overlap set "coco": ten minimum overlaps per class, vision3d_amd/evaluation/kitti.py) against
the float64 restatements of tests/kitti_eval_ref.py and tests/kitti_eval_image_ref.py run at every level: per-level details
and AP exactly, the means exactly, AOS within 1e-6; the levels that coincide with an official minimum overlap against the
official combos of the same call; determinism; official results unchanged; the family pass 2 against the per-combo pass 2;
model output against result files; the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_eval_image_ref as RI  # noqa: E402
import kitti_eval_ref as R  # noqa: E402

from vision3d_amd.dataset import kitti as K  # noqa: E402
from vision3d_amd.evaluation import KittiEvaluator, write_kitti_results  # noqa: E402
from vision3d_amd.evaluation import kitti as E  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("Car", "Pedestrian", "Cyclist")
SETS = ("strict", "loose", "coco")


@pytest.fixture(scope="module")
def sweep_margins():
    """The generators keep every overlap >= 1e-3 from the minimum overlaps they know; widen those to every sweep level."""
    saved = R.THRESHOLDS, RI.IMAGE_THRESHOLDS
    levels = {float(v) for lv in E.COCO_LEVELS.values() for v in lv} | set(R.THRESHOLDS) | set(RI.IMAGE_THRESHOLDS)
    R.THRESHOLDS = RI.IMAGE_THRESHOLDS = tuple(sorted(levels))
    yield
    R.THRESHOLDS, RI.IMAGE_THRESHOLDS = saved


@pytest.fixture(scope="module")
def bev_set(sweep_margins):
    rng = np.random.default_rng(23)
    pairs = [R.synthetic_frame(rng, int(rng.integers(0, 16)), int(rng.integers(0, 5))) for _ in range(100)]
    # one frame whose overlap tile (> 12 k pairs) does not fit the family kernel's LDS budget: the global-memory path
    pairs.append(R.synthetic_frame(rng, 100, 40))
    return pairs


@pytest.fixture(scope="module")
def image_set(sweep_margins):
    rng = np.random.default_rng(29)
    pairs = [RI.synthetic_frame(rng, int(rng.integers(0, 16)), int(rng.integers(0, 6))) for _ in range(100)]
    assert {n for g, _ in pairs for n in g.names} >= {"Car", "Pedestrian", "Cyclist", "DontCare"}
    return pairs


def _device_eval(pairs, **kw):
    ev = KittiEvaluator(**kw)
    for g, d in pairs:
        ev.add_frame(g, d)
    return ev.compute(), ev.details, ev


def _mean(values):
    total = 0.0
    for v in values:
        total += float(v)
    return total / len(values)


def _assert_detail(got, want, key, sim=False):
    assert got["n_valid_gt"] == want["n_valid_gt"], key
    assert np.array_equal(got["thresholds"], want["thresholds"]), key
    assert np.array_equal(got["counts"], want["counts"]), key
    if sim:
        assert np.abs(got["similarity"] - want["similarity"]).max(initial=0.0) <= 1e-6, key


def _same_bits(a, b, key):
    assert a.keys() == b.keys(), key
    for f in a:
        assert np.array_equal(a[f], b[f]), (key, f)


def test_coco_bev_3d_matches_restatement(bev_set):
    res, det, ev = _device_eval(bev_set, overlaps=SETS)
    frames = [R.make_frame(g, d) for g, d in bev_set]
    for c in CLASSES:
        levels = E.COCO_LEVELS[c]
        for m in ("bev", "3d"):
            for d in range(3):
                key = ("coco", c, m, d)
                dd = det[key]
                assert dd["levels"].dtype == np.float32 and np.array_equal(dd["levels"], levels)
                assert dd["ap"].shape == (10, 2) and len(dd["per_level"]) == 10 and "aos" not in dd
                want = [R.evaluate_combo(frames, c, m, d, float(t)) for t in levels]
                for k, w in enumerate(want):
                    _assert_detail(dd["per_level"][k], w, key + (k,))
                    assert dd["ap"][k, 0] == w["R11"] and dd["ap"][k, 1] == w["R40"], key + (k,)
                for kind in ("R11", "R40"):
                    assert res["coco"][c][m][kind][d] == _mean([w[kind] for w in want]), key + (kind,)
    assert sum(d["counts"][:, 0].sum() for k, v in det.items() if k[0] == "coco" for d in v["per_level"]) > 1000
    assert any(0 < v < 100 for c in CLASSES for m in ("bev", "3d") for v in res["coco"][c][m]["R40"])
    # the float32 levels that equal an official minimum overlap give the official combo's bits, in the same call
    for c, k, o in (("Car", 0, "loose"), ("Car", 4, "strict"), ("Pedestrian", 0, "loose"), ("Cyclist", 0, "loose"),
                    ("Pedestrian", 5, "strict"), ("Cyclist", 5, "strict")):
        assert E.COCO_LEVELS[c][k] == np.float32(E.MIN_OVERLAP[o][c])
        for m in ("bev", "3d"):
            for d in range(3):
                _same_bits(det[("coco", c, m, d)]["per_level"][k], det[(o, c, m, d)], (c, k, o, m, d))
                assert det[("coco", c, m, d)]["ap"][k].tolist() == [res[o][c][m]["R11"][d], res[o][c][m]["R40"][d]]
    # official results and details unchanged by the sweep
    res_off, det_off, _ = _device_eval(bev_set)
    for o in ("strict", "loose"):
        assert res[o] == res_off[o]
    for k in det_off:
        _same_bits(det[k], det_off[k], k)
    # bit-identical across a repeated call and a shuffled frame order
    assert ev.compute() == res
    order = np.random.default_rng(3).permutation(len(bev_set))
    res2, det2, _ = _device_eval([bev_set[i] for i in order], overlaps=SETS)
    assert res2 == res
    for k in det:
        if k[0] == "coco":
            assert np.array_equal(det[k]["ap"], det2[k]["ap"]), k
            for a, b in zip(det[k]["per_level"], det2[k]["per_level"]):
                _same_bits(a, b, k)


def test_coco_bbox_aos_matches_restatement(image_set):
    res, det, ev = _device_eval(image_set, metrics=("bbox", "aos"), overlaps=SETS)
    frames = [RI.make_frame(g, d) for g, d in image_set]
    for c in CLASSES:
        levels = E.COCO_LEVELS[c]
        for d in range(3):
            key = ("coco", c, "bbox", d)
            dd = det[key]
            assert dd["aos"].shape == (10, 2)
            want = [RI.evaluate_combo(frames, c, d, float(t)) for t in levels]
            for k, w in enumerate(want):
                _assert_detail(dd["per_level"][k], w, key + (k,), sim=True)
                assert dd["ap"][k, 0] == w["R11"] and dd["ap"][k, 1] == w["R40"], key + (k,)
                assert np.abs(dd["aos"][k] - [w["aos_R11"], w["aos_R40"]]).max() <= 1e-6, key + (k,)
            for kind in ("R11", "R40"):
                assert res["coco"][c]["bbox"][kind][d] == _mean([w[kind] for w in want]), key + (kind,)
                assert abs(res["coco"][c]["aos"][kind][d] - _mean([w["aos_" + kind] for w in want])) <= 1e-6, key + (kind,)
    assert any(0 < v < 100 for c in CLASSES for v in res["coco"][c]["aos"]["R40"])
    # bbox levels 0.7 (Car) and 0.5 (Pedestrian, Cyclist) against the official bbox combos (0.7 / 0.5 in both sets)
    for c, k in (("Car", 4), ("Pedestrian", 5), ("Cyclist", 5)):
        assert E.COCO_LEVELS[c][k] == np.float32(E.MIN_OVERLAP_IMAGE[c])
        for o in ("strict", "loose"):
            for d in range(3):
                _same_bits(det[("coco", c, "bbox", d)]["per_level"][k], det[(o, c, "bbox", d)], (c, k, o, d))
                assert det[("coco", c, "bbox", d)]["aos"][k].tolist() == [res[o][c]["aos"]["R11"][d], res[o][c]["aos"]["R40"][d]]
    res_off, det_off, _ = _device_eval(image_set, metrics=("bbox", "aos"))
    for o in ("strict", "loose"):
        assert res[o] == res_off[o]
    for k in det_off:
        _same_bits(det[k], det_off[k], k)
    assert ev.compute() == res
    order = np.random.default_rng(4).permutation(len(image_set))
    res2, _, _ = _device_eval([image_set[i] for i in order], metrics=("bbox", "aos"), overlaps=SETS)
    assert res2 == res
    lines = ev.summary(r11=True).splitlines()
    assert lines[12] == "Car coco AP_R11@0.50:0.05:0.95: bbox: " + ", ".join(f"{v:.4f}" for v in res["coco"]["Car"]["bbox"]["R11"]) + \
        "  aos: " + ", ".join(f"{v:.4f}" for v in res["coco"]["Car"]["aos"]["R11"])
    assert lines[15].startswith("Pedestrian coco AP_R40@0.25:0.05:0.70: bbox: ")


def test_family_pass2_matches_per_combo_pass2(bev_set, image_set, monkeypatch):
    """A sweep runs its ten levels of one (class, metric, difficulty) as one family through kitti_pass2_family_kernel; one level
    at a time they are lone combos and run through kitti_pass2_kernel.  Counts and similarity agree bit for bit, on frames
    whose overlap tile is staged in LDS and on the one whose tile is read from global memory."""
    pairs = list(bev_set) + list(image_set)
    metrics = ("bbox", "bev", "3d", "aos")
    _, det, ev = _device_eval(pairs, metrics=metrics, overlaps=("coco",))
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        ev.compute()
        torch.cuda.synchronize()
    names = " ".join(e.key for e in prof.key_averages() if e.device_time_total > 0)
    if "kitti_" in names:  # (where the profiler records the library's kernels) every level ran in the family kernel
        assert "kitti_pass2_family_kernel" in names and "kitti_pass2_kernel" not in names
    levels = dict(E.COCO_LEVELS)
    for k in range(10):
        monkeypatch.setattr(E, "COCO_LEVELS", {c: v[k:k + 1] for c, v in levels.items()})
        _, det1, _ = _device_eval(pairs, metrics=metrics, overlaps=("coco",))
        for key, v in det1.items():
            _same_bits(v["per_level"][0], det[key]["per_level"][k], key + (k,))
            assert np.array_equal(v["ap"][0], det[key]["ap"][k]), key + (k,)
            if key[2] == "bbox":
                assert np.array_equal(v["aos"][0], det[key]["aos"][k]), key + (k,)


def test_model_output_matches_result_files_coco(tmp_path, sweep_margins):
    """Second.inference -> add_frame(model tensors) gives the same COCO-style APs as write_kitti_results -> read_labels ->
    add_frame(Labels); the CLI with --overlaps coco prints the block."""
    import test_gpu_kitti_eval as TB
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
    rng = np.random.default_rng(6)
    kept = []
    for b in range(len(clouds)):
        calib = TB._calib(b)
        m = bidx == b
        fb, fc, fs = boxes[m], cidx[m], scores[m]
        assert fb.shape[0] > 0, "the model emitted no detection for a frame"
        path = tmp_path / "results" / f"{b:06d}.txt"
        write_kitti_results(path, fb, fc, fs, calib, names)
        dt = K.read_labels(path)
        cam = R.camera_boxes(dt)
        pick = rng.choice(len(cam), min(len(cam), 8), replace=False)
        g_cam = cam[pick] + np.c_[rng.normal(0, 0.15, (len(pick), 3)), np.zeros((len(pick), 4))]
        with open(tmp_path / "label_2" / f"{b:06d}.txt", "w") as f:
            for k in range(len(pick)):
                x, yb, z, h, w, l, ry = g_cam[k]
                f.write(f"Car 0 0 0 100 100 200 170 {h:.9g} {w:.9g} {l:.9g} {x:.9g} {yb:.9g} {z:.9g} {ry:.9g}\n")
        gt = K.read_labels(tmp_path / "label_2" / f"{b:06d}.txt")
        sel = TB._clear_of_thresholds(gt, dt)  # (R.THRESHOLDS holds every sweep level here)
        kept.append((gt, calib, fb[sel], fc[sel], fs[sel]))
        write_kitti_results(path, fb[sel], fc[sel], fs[sel], calib, names)
    ev_model = KittiEvaluator(classes=("Car",), overlaps=("coco",), det_names=names)
    ev_file = KittiEvaluator(classes=("Car",), overlaps=("coco",))
    for b, (gt, calib, fb, fc, fs) in enumerate(kept):
        ev_model.add_frame(gt, (fb, fc, fs, calib))
        ev_file.add_frame(gt, K.read_labels(tmp_path / "results" / f"{b:06d}.txt"))
    got, want = ev_model.compute(), ev_file.compute()
    assert got == want
    for k, w in ev_file.details.items():
        for a, b in zip(ev_model.details[k]["per_level"], w["per_level"]):
            _same_bits(a, b, k)
    assert sum(d["counts"][:, 0].sum() for v in ev_file.details.values() for d in v["per_level"]) > 0
    assert any(v > 0 for v in want["coco"]["Car"]["bev"]["R40"])
    ev_all = KittiEvaluator(overlaps=SETS)
    for b, (gt, *_rest) in enumerate(kept):
        ev_all.add_frame(gt, K.read_labels(tmp_path / "results" / f"{b:06d}.txt"))
    ev_all.compute()
    out = subprocess.run([sys.executable, "-m", "vision3d_amd.evaluation", "--labels", str(tmp_path / "label_2"), "--results",
                          str(tmp_path / "results"), "--overlaps", "strict,loose,coco"], cwd=REPO, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == ev_all.summary().strip()
    assert "Car coco AP_R40@0.50:0.05:0.95: bev: " in out.stdout
    plain = subprocess.run([sys.executable, "-m", "vision3d_amd.evaluation", "--labels", str(tmp_path / "label_2"), "--results",
                            str(tmp_path / "results")], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "coco" not in plain.stdout
    assert plain.stdout.strip() == "\n".join(ev_all.summary().splitlines()[:6])

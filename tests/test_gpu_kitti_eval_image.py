"""GPU: KITTI 2-D bbox AP and AOS on the device (csrc/kitti_eval.hip via vision3d_amd.evaluation) against the float64
restatement of tests/kitti_eval_image_ref.py: 2-D overlaps; per bbox combo n_valid_gt, thresholds, (tp, fp, fn) and AP exactly;
similarity and AOS within 1e-6; determinism; BEV / 3-D untouched; model output against result files; the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_eval_image_ref as RI  # noqa: E402
import kitti_eval_ref as R  # noqa: E402

from vision3d_amd import _lib as L  # noqa: E402
from vision3d_amd.dataset import kitti as K  # noqa: E402
from vision3d_amd.evaluation import KittiEvaluator, write_kitti_results  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("bbox", "bev", "3d", "aos")


def _device_eval(pairs, **kw):
    ev = KittiEvaluator(**kw)
    for g, d in pairs:
        ev.add_frame(g, d)
    return ev.compute(), ev.details, ev


def _assert_same(pairs, dev_res, dev_det, classes=("Car", "Pedestrian", "Cyclist")):
    want_res, want_det = RI.evaluate([RI.make_frame(g, d) for g, d in pairs], classes=classes)
    for key, w in want_det.items():
        got = dev_det[key]
        assert got["n_valid_gt"] == w["n_valid_gt"], key
        assert np.array_equal(got["thresholds"], w["thresholds"]), key
        assert np.array_equal(got["counts"], w["counts"]), key
        assert np.abs(got["similarity"] - w["similarity"]).max(initial=0.0) <= 1e-6, key
    for o in want_res:
        for c in want_res[o]:
            assert dev_res[o][c]["bbox"] == want_res[o][c]["bbox"], (o, c)
            for kind in ("R11", "R40"):
                assert np.abs(np.array(dev_res[o][c]["aos"][kind]) - want_res[o][c]["aos"][kind]).max() <= 1e-6, (o, c, kind)


def test_image_overlaps_match_float64():
    rng = np.random.default_rng(0)
    n_dt, n_gt = 300, 120
    x1, y1 = rng.uniform(0, 1100, n_gt), rng.uniform(0, 300, n_gt)
    gt = np.stack((x1, y1, x1 + rng.uniform(5, 200, n_gt), y1 + rng.uniform(5, 100, n_gt)), 1)
    dt = gt[rng.integers(0, n_gt, n_dt)] + rng.normal(0, 15, (n_dt, 4))
    dt[:10] = gt[:10]  # identical boxes
    dt[10, 2] = dt[10, 0]  # zero width
    dt[11, [0, 2]] = dt[11, [2, 0]]  # inverted
    gt[12, 3] = gt[12, 1] - 1.0  # inverted in y
    gt, dt = gt.astype(np.float32), dt.astype(np.float32)
    dev = torch.device("cuda")
    gt5 = torch.from_numpy(np.c_[gt, np.zeros(n_gt, np.float32)]).to(dev).contiguous()
    dt5 = torch.from_numpy(np.c_[dt, np.zeros(n_dt, np.float32)]).to(dev).contiguous()
    gt_off = torch.tensor([0, n_gt], dtype=torch.int32, device=dev)
    dt_off = torch.tensor([0, n_dt], dtype=torch.int32, device=dev)
    ov_off = torch.tensor([0, n_dt * n_gt], dtype=torch.int64, device=dev)
    ov = torch.full((n_dt * n_gt,), -1.0, dtype=torch.float32, device=dev)
    L.check(L.lib().v3d_kitti_eval_overlaps_image(L.ptr(gt5), L.ptr(gt_off), L.ptr(dt5), L.ptr(dt_off), L.ptr(ov_off), 1, n_dt,
                                                  n_gt, L.ptr(ov), L.stream_ptr()), "overlaps_image")
    got = ov.view(n_dt, n_gt).cpu().numpy()
    want = RI.image_overlaps(dt.astype(np.float64), gt.astype(np.float64))
    assert (want > 0).sum() > 500
    assert np.abs(got - want).max() <= 1e-6
    assert (np.abs(np.diag(got[:10, :10]) - 1) <= 1e-6).all()
    assert (got[10] == 0).all() and (got[11] == 0).all() and (got[:, 12] == 0).all()


@pytest.mark.parametrize("kind", ["all_found", "fp_in_front", "dontcare_fp", "dontcare_short", "dontcare_low",
                                  "dontcare_partial", "iou060"])
@pytest.mark.parametrize("d_alpha", [0.0, np.pi / 2, np.pi])
def test_hand_cases(kind, d_alpha):
    pairs = RI.hand_case(kind, d_alpha)
    res, det, _ = _device_eval(pairs, metrics=("bbox", "aos"))
    _assert_same(pairs, res, det)


@pytest.fixture(scope="module")
def val_set():
    rng = np.random.default_rng(17)
    pairs = [RI.synthetic_frame(rng, int(rng.integers(0, 16)), int(rng.integers(0, 6))) for _ in range(100)]
    pairs += [RI.synthetic_frame(rng, 0, 3, n_dc=1), RI.synthetic_frame(rng, 5, 0), RI.synthetic_frame(rng, 0, 0, n_dc=0)]
    names = {n for g, d in pairs for n in g.names}
    assert names >= {"Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "DontCare", "Misc"}
    return pairs


def test_synthetic_val_set_matches_restatement(val_set):
    res, det, ev = _device_eval(val_set, metrics=("bbox", "aos"))
    _assert_same(val_set, res, det)
    assert sum(d["counts"][:, 0].sum() for d in det.values()) > 1000  # the set exercises the assignment
    assert any(0 < v for o in res.values() for c in o.values() for v in c["aos"]["R40"])
    # bit-identical across runs and frame orders, AOS and similarity included
    assert ev.compute() == res
    order = np.random.default_rng(1).permutation(len(val_set))
    res2, det2, _ = _device_eval([val_set[i] for i in order], metrics=("bbox", "aos"))
    assert res2 == res
    for k in det:
        for f in ("thresholds", "counts", "similarity"):
            assert np.array_equal(det[k][f], det2[k][f]), (k, f)


def test_all_four_metrics_leave_bev_and_3d_alone(val_set):
    # the image set's camera boxes are far apart; add the BEV / 3-D set so that those metrics have work to do
    rng = np.random.default_rng(7)
    pairs = list(val_set) + [R.synthetic_frame(rng, int(rng.integers(0, 16)), int(rng.integers(0, 5))) for _ in range(40)]
    res_all, det_all, ev = _device_eval(pairs, metrics=ALL)
    res_def, det_def, ev_def = _device_eval(pairs)
    res_img, det_img, _ = _device_eval(pairs, metrics=("bbox", "aos"))
    for o in res_def:
        for c in res_def[o]:
            assert list(res_all[o][c]) == list(ALL)
            for m in ("bev", "3d"):
                assert res_all[o][c][m] == res_def[o][c][m]
            for m in ("bbox", "aos"):
                assert res_all[o][c][m] == res_img[o][c][m]
    for k in det_def:
        assert all(np.array_equal(det_all[k][f], det_def[k][f]) for f in ("thresholds", "counts")), k
    assert any(v > 0 for o in res_def.values() for c in o.values() for v in c["bev"]["R40"])
    assert ev_def.summary(r11=True).splitlines()[0].startswith("Car AP_R11@0.70, 0.70: bev: ")
    assert ev.summary().splitlines()[0].startswith("Car AP_R40@0.70, 0.70, 0.70: bbox: ")
    assert ev.summary().splitlines()[3].startswith("Car AP_R40@0.70, 0.50, 0.50: bbox: ")  # the loose set
    aos_only = KittiEvaluator(metrics=("aos",))
    for g, d in pairs:
        aos_only.add_frame(g, d)
    r = aos_only.compute()
    assert list(r["strict"]["Car"]) == ["aos"] and r["strict"]["Car"]["aos"] == res_all["strict"]["Car"]["aos"]
    assert KittiEvaluator(metrics=ALL).compute()["loose"]["Cyclist"]["aos"]["R11"] == [0.0] * 3  # no frames
    with pytest.raises(ValueError):
        KittiEvaluator(metrics=("bbox", "2d"))


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


def _label_line(name, box2d, alpha, cam, trunc=0.0, occ=0, score=None):
    x, yb, z, h, w, l, ry = cam
    vals = [trunc, occ, alpha, *box2d, h, w, l, x, yb, z, ry] + ([] if score is None else [score])
    return name + " " + " ".join(f"{float(v):.9g}" for v in vals) + "\n"


def _clear_detections(gt, dt):
    """indices of detections whose 2-D IoUs with every ground truth and inter / area_dt with every DontCare region sit >= 1e-4
    from 0.5 and 0.7, whose 2-D height sits >= 1e-3 px from every MIN_HEIGHT, and whose IoUs on a ground truth sit >= 1e-5 from
    another kept detection's (the two detection paths may differ by an ulp)."""
    f = RI.make_frame(gt, dt)
    ov, ratio = f["ov"]["bbox"], f["dc_ratio"]
    ok = np.ones(len(dt.names), bool)
    for t in RI.IMAGE_THRESHOLDS:
        ok &= (np.abs(ov - t) >= 1e-4).all(1) & (np.abs(ratio - t) >= 1e-4).all(1)
    for m in (25, 40):
        ok &= np.abs(f["dt_h"] - m) >= 1e-3
    kept = []
    for j in np.nonzero(ok)[0]:
        if all(not ((ov[j] > 0) & (ov[k] > 0) & (np.abs(ov[j] - ov[k]) < 1e-5)).any() for k in kept):
            kept.append(j)
    return np.array(kept, np.int64)


def test_model_output_matches_result_files(tmp_path):
    """Second.inference -> add_frame(model tensors) gives the same bbox AP, and AOS within 1e-6, as write_kitti_results ->
    read_labels -> add_frame(Labels); the CLI with --metrics bbox,bev,3d,aos prints exactly summary()."""
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
        # ground truth: some detections' image boxes jittered (so that 2-D matches happen), alphas near theirs, plus a DontCare
        # region over another detection
        cam = R.camera_boxes(dt)
        pick = rng.choice(len(cam), min(len(cam), 8), replace=False)
        lines = []
        for j in pick:
            x1, y1, x2, y2 = dt.box2d[j]
            w, h = max(x2 - x1, 30.0), max(y2 - y1, 45.0)
            box = [x1 + rng.normal(0, 0.05 * w), y1 + rng.normal(0, 0.05 * h), x1 + w * rng.uniform(0.9, 1.1),
                   y1 + h * rng.uniform(0.9, 1.1)]
            lines.append(_label_line("Car", box, dt.alpha[j] + rng.normal(0, 0.4), cam[j]))
        rest = [j for j in range(len(cam)) if j not in set(pick)]
        if rest:
            x1, y1, x2, y2 = dt.box2d[rest[0]]
            lines.append(_label_line("DontCare", [x1 - 10, y1 - 10, x2 + 10, y2 + 10], -10, [-1000, -1000, -1000, -1, -1, -1, -10],
                                     trunc=-1, occ=-1))
        with open(tmp_path / "label_2" / f"{b:06d}.txt", "w") as f:
            f.writelines(lines)
        gt = K.read_labels(tmp_path / "label_2" / f"{b:06d}.txt")
        sel = _clear_detections(gt, dt)
        kept.append((gt, calib, fb[sel], fc[sel], fs[sel]))
        write_kitti_results(path, fb[sel], fc[sel], fs[sel], calib, names)  # the retained detections only
    ev_model = KittiEvaluator(classes=("Car",), metrics=ALL, det_names=names)
    ev_file = KittiEvaluator(classes=("Car",), metrics=ALL)
    for b, (gt, calib, fb, fc, fs) in enumerate(kept):
        ev_model.add_frame(gt, (fb, fc, fs, calib))
        ev_file.add_frame(gt, K.read_labels(tmp_path / "results" / f"{b:06d}.txt"))
    got, want = ev_model.compute(), ev_file.compute()
    for o in want:
        assert got[o]["Car"]["bbox"] == want[o]["Car"]["bbox"]
        for kind in ("R11", "R40"):
            assert np.abs(np.array(got[o]["Car"]["aos"][kind]) - want[o]["Car"]["aos"][kind]).max() <= 1e-6
    for k, w in ev_file.details.items():
        if k[2] == "bbox":
            assert np.array_equal(ev_model.details[k]["counts"], w["counts"]), k
    assert sum(d["counts"][:, 0].sum() for k, d in ev_file.details.items() if k[2] == "bbox") > 0
    # the CLI prints the file evaluator's summary (all three classes, all four metrics)
    ev_all = KittiEvaluator(metrics=ALL)
    for b, (gt, *_rest) in enumerate(kept):
        ev_all.add_frame(gt, K.read_labels(tmp_path / "results" / f"{b:06d}.txt"))
    out = subprocess.run([sys.executable, "-m", "vision3d_amd.evaluation", "--labels", str(tmp_path / "label_2"), "--results",
                          str(tmp_path / "results"), "--metrics", "bbox,bev,3d,aos", "--r11"], cwd=REPO, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == ev_all.summary(r11=True).strip()
    assert "Car AP_R40@0.70, 0.70, 0.70: bbox: " in out.stdout and "  aos: " in out.stdout

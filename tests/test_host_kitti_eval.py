"""CPU: the KITTI BEV / 3-D AP protocol (vision3d_amd/evaluation/kitti.py) restated in float64 (tests/kitti_eval_ref.py) on hand
cases with known answers, the overlap conventions pinned by known IoUs, the evaluator's host-side ignore flags against the
restatement, and the KITTI result writer."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_eval_ref as R  # noqa: E402

from vision3d_amd.dataset import kitti as K  # noqa: E402
from vision3d_amd.evaluation import kitti as E  # noqa: E402
from vision3d_amd.evaluation import lidar_to_camera, write_kitti_results  # noqa: E402


def _car_ap(kind, d=1, metric="bev"):
    frames = [R.make_frame(g, dt) for g, dt in R.hand_case(kind)]
    res, det = R.evaluate(frames, classes=("Car",))
    return res["strict"]["Car"][metric], det[("strict", "Car", metric, d)]


@pytest.mark.parametrize("metric", ["bev", "3d"])
def test_all_found_and_none_found(metric):
    ap, det = _car_ap("all_found", metric=metric)
    assert ap["R40"] == [100.0] * 3 and ap["R11"] == [100.0] * 3
    assert det["n_valid_gt"] == 80 and len(det["thresholds"]) == 41 and list(det["counts"][-1]) == [80, 0, 0]
    ap, det = _car_ap("none_found", metric=metric)
    assert ap["R40"] == [0.0] * 3 and ap["R11"] == [0.0] * 3 and det["n_valid_gt"] == 80


def test_one_false_positive_in_front():
    # every one of the 41 thresholds keeps the FP: precision k / (k + 1) rises with k, so its running maximum is 80 / 81 everywhere
    ap, det = _car_ap("fp_in_front")
    assert len(det["thresholds"]) == 41 and list(det["counts"][-1]) == [80, 1, 0]
    assert all(abs(v - 100 * 80 / 81) < 1e-12 for v in ap["R40"] + ap["R11"])


def test_van_under_car_is_neither_tp_nor_fp():
    ap, det = _car_ap("van_under_car")
    assert ap["R40"] == [100.0] * 3 and list(det["counts"][-1]) == [80, 0, 0] and det["n_valid_gt"] == 80
    _, det = _car_ap("van_fp")  # the same detection without the Van: a false positive
    assert list(det["counts"][-1]) == [80, 1, 0]


def test_short_detection_of_another_class_is_absorbed():
    _, det = _car_ap("short_absorbed")
    assert det["n_valid_gt"] == 81 and list(det["counts"][-1]) == [80, 0, 0]  # the Car it sits on is neither found nor missed
    _, det = _car_ap("tall_not_absorbed")  # a tall Pedestrian detection is not part of the Car evaluation: the Car is missed
    assert det["n_valid_gt"] == 81 and list(det["counts"][-1]) == [80, 0, 1]


def test_height_25_is_ignored_at_moderate():
    frames = [R.make_frame(g, dt) for g, dt in R.hand_case("height25")]
    _, det = R.evaluate(frames, classes=("Car",))
    assert det[("strict", "Car", "bev", 1)]["n_valid_gt"] == 80  # 25 <= MIN_HEIGHT: ignored
    assert det[("strict", "Car", "bev", 2)]["n_valid_gt"] == 80
    assert det[("strict", "Car", "bev", 0)]["n_valid_gt"] == 80  # (and below 40 at easy)
    assert R.clean(frames[0], "Car", 1)[0][-1] == 1


def test_known_answer_ious():
    a = [0, 1.5, 10, 1.5, 2.0, 4.0, 0.0]  # 4 m long (l along the heading), 2 m wide
    along = [1, 1.5, 10, 1.5, 2.0, 4.0, 0.0]
    across = [0, 1.5, 11, 1.5, 2.0, 4.0, 0.0]
    bev, d3 = R.overlaps(np.array([along, across]), np.array([a]))
    assert abs(bev[0, 0] - 0.6) < 1e-12 and abs(bev[1, 0] - 1 / 3) < 1e-12
    assert abs(d3[0, 0] - 0.6) < 1e-12  # same heights: 3-D = BEV
    turned = [0, 1.5, 10, 1.5, 2.0, 4.0, np.pi / 2]
    turned_off = [0, 1.5, 11, 1.5, 2.0, 4.0, np.pi / 2]  # ry = pi/2 turns the length onto camera z
    bev, _ = R.overlaps(np.array([turned_off]), np.array([turned]))
    assert abs(bev[0, 0] - 0.6) < 1e-12
    half_up = [0, 0.75, 10, 1.5, 2.0, 4.0, 0.0]  # y is the bottom, y points down: half the height overlaps
    _, d3 = R.overlaps(np.array([half_up]), np.array([a]))
    assert abs(d3[0, 0] - 1 / 3) < 1e-12


def test_host_ignore_flags_match_the_restatement():
    rng = np.random.default_rng(3)
    for _ in range(20):
        gt, dt = R.synthetic_frame(rng, int(rng.integers(0, 16)), int(rng.integers(0, 5)), margins=False)
        frame = R.make_frame(gt, dt)
        _, gmeta = E._gt_arrays(gt)
        _, dmeta = E._dt_arrays(dt)
        for c in ("Car", "Pedestrian", "Cyclist"):
            for d in range(3):
                ig_gt, ig_dt, _ = R.clean(frame, c, d)
                code, nb = E.CLASS_CODE[c], E.CLASS_CODE.get(E.NEIGHBOUR[c], -1)
                ign = (gmeta[:, 1] >> d) & 1
                want = np.where(gmeta[:, 0] == code, ign, np.where(gmeta[:, 0] == nb, 1, -1))
                assert np.array_equal(want, ig_gt)
                want = np.where((dmeta[:, 1] >> d) & 1, 1, np.where(dmeta[:, 0] == code, 0, -1))
                assert np.array_equal(want, ig_dt)


def _calib(r0=None):
    v2c = np.array([[0.0, -1.0, 0.0, 0.02], [0.0, 0.0, -1.0, -0.08], [1.0, 0.0, 0.0, -0.27]], np.float32)
    c2v = np.zeros_like(v2c)
    c2v[:, :3] = v2c[:, :3].T
    c2v[:, 3] = -v2c[:, :3].T @ v2c[:, 3]
    p2 = np.array([[721.5, 0, 609.6, 44.9], [0, 721.5, 172.9, 0.2], [0, 0, 1, 0.003]], np.float32)
    r0 = np.eye(3, dtype=np.float32) if r0 is None else r0
    return K.Calib(V2C=v2c, C2V=c2v, R0=r0, P2=p2, WH=np.r_[1224, 370])


def _lidar_boxes(rng, n):
    b = np.zeros((n, 7), np.float32)
    b[:, 0] = rng.uniform(5, 60, n)
    b[:, 1] = rng.uniform(-20, 20, n)
    b[:, 2] = rng.uniform(-1.5, -0.5, n)
    b[:, 3:6] = np.array([1.6, 3.9, 1.56]) * rng.uniform(0.8, 1.2, (n, 3))
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


def test_write_kitti_results_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    boxes = _lidar_boxes(rng, 12)
    cls = rng.integers(0, 3, 12)
    scores = rng.random(12).astype(np.float32)
    calib = _calib()
    path = tmp_path / "000001.txt"
    write_kitti_results(path, torch.from_numpy(boxes), torch.from_numpy(cls), torch.from_numpy(scores), calib,
                        ["Car", "Pedestrian", "Cyclist"])
    lab = K.read_labels(path)
    assert lab.names == [["Car", "Pedestrian", "Cyclist"][c] for c in cls]
    assert np.array_equal(lab.score.astype(np.float32), scores)
    assert (lab.truncation == -1).all() and (lab.occlusion == -1).all()
    cam, box2d = lidar_to_camera(torch.from_numpy(boxes), torch.from_numpy(E.calib_rows(calib))[None].expand(12, 26))
    cam, box2d = cam.numpy(), box2d.numpy()
    # every written number reads back to the float32 that was computed
    assert np.array_equal(lab.box2d.astype(np.float32), box2d)
    assert np.array_equal(lab.hwl.astype(np.float32), cam[:, 3:6])
    assert np.array_equal(lab.ry.astype(np.float32), cam[:, 6]) and np.array_equal(lab.ry.astype(np.float32), -boxes[:, 6])
    assert np.array_equal((lab.location[:, 1] + lab.hwl[:, 0] / 2).astype(np.float32), cam[:, 1])
    assert (box2d[:, [0, 2]] >= 0).all() and (box2d[:, [0, 2]] <= 1224).all() and (box2d[:, [1, 3]] <= 370).all()
    want_alpha = -np.arctan2(-boxes[:, 1].astype(np.float64), boxes[:, 0]) - boxes[:, 6]
    assert np.abs(lab.alpha - want_alpha).max() < 1e-5
    # lidar -> camera -> boxes_in_lidar_frame (which applies R0 forward, as the upstream loader does: R0 = I here)
    back = K.boxes_in_lidar_frame(lab, calib)
    assert np.abs(back - boxes).max() < 1e-5


def test_camera_box_is_the_rotated_box():
    """The camera box's corners (l along (cos ry, -sin ry) in (x, z)) project to the written 2-D box."""
    rng = np.random.default_rng(1)
    boxes = _lidar_boxes(rng, 6)
    calib = _calib()
    cam, box2d = lidar_to_camera(torch.from_numpy(boxes), torch.from_numpy(E.calib_rows(calib))[None].expand(6, 26))
    cam, box2d = cam.numpy().astype(np.float64), box2d.numpy()
    for k in range(6):
        x, yb, z, h, w, l, ry = cam[k]
        c = R.bev_corners(x, z, l, w, ry)
        pts = np.array([[px, y, pz, 1.0] for px, pz in c for y in (yb, yb - h)])
        uvw = pts @ calib.P2.astype(np.float64).T
        u, v = uvw[:, 0] / uvw[:, 2], uvw[:, 1] / uvw[:, 2]
        want = np.array([np.clip(u.min(), 0, 1224), np.clip(v.min(), 0, 370), np.clip(u.max(), 0, 1224), np.clip(v.max(), 0, 370)])
        assert np.abs(box2d[k] - want).max() < 1e-2

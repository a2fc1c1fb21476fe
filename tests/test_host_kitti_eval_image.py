"""CPU: the KITTI 2-D bbox AP and AOS rules (vision3d_amd/evaluation/kitti.py) restated in float64
(tests/kitti_eval_image_ref.py) on hand cases with known answers: DontCare absorption, AOS against bbox AP, the per-metric
minimum overlaps, the host-side DontCare flag and image rows of the evaluator, and the combo-metric argument checks of the C
entry points."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_eval_image_ref as RI  # noqa: E402
import kitti_eval_ref as R  # noqa: E402

from vision3d_amd import _lib as L  # noqa: E402
from vision3d_amd.evaluation import kitti as E  # noqa: E402


def _car(kind, d_alpha=0.0, overlap="strict"):
    frames = [RI.make_frame(g, dt) for g, dt in RI.hand_case(kind, d_alpha)]
    res, det = RI.evaluate(frames, classes=("Car",), overlap_sets=(overlap,))
    return res[overlap]["Car"], det[(overlap, "Car", "bbox", 1)]


def test_image_overlaps_known_answers():
    a = [0.0, 0.0, 100.0, 60.0]
    assert RI.image_overlaps([a], [a])[0, 0] == 1.0
    assert abs(RI.image_overlaps([[25.0, 0.0, 125.0, 60.0]], [a])[0, 0] - 0.6) < 1e-15  # 75 / 125
    assert RI.image_overlaps([[100.0, 0.0, 150.0, 60.0]], [a])[0, 0] == 0.0  # touching: iw == 0
    inside = [10.0, 10.0, 30.0, 30.0]
    assert RI.image_overlaps([inside], [a], criterion=0)[0, 0] == 1.0  # inter / area_dt
    assert abs(RI.image_overlaps([inside], [a])[0, 0] - 400 / 6000) < 1e-15


def test_all_found():
    r, det = _car("all_found")
    assert r["bbox"]["R40"] == [100.0] * 3 and r["bbox"]["R11"] == [100.0] * 3
    assert det["n_valid_gt"] == 80 and len(det["thresholds"]) == 41 and list(det["counts"][-1]) == [80, 0, 0]


def test_dontcare_absorbs_a_false_positive_in_front():
    r, det = _car("fp_in_front")
    assert list(det["counts"][-1]) == [80, 1, 0]
    assert all(abs(v - 100 * 80 / 81) < 1e-12 for v in r["bbox"]["R40"] + r["bbox"]["R11"])
    r, det = _car("dontcare_fp")  # the same detection inside a DontCare region: absorbed, AP back to the all-found value
    assert list(det["counts"][-1]) == [80, 0, 0] and r["bbox"]["R40"] == [100.0] * 3 and r["bbox"]["R11"] == [100.0] * 3


@pytest.mark.parametrize("kind", ["dontcare_short", "dontcare_low"])
def test_dontcare_absorbs_neither_short_nor_under_threshold(kind):
    # neither detection is a false positive, so neither may be absorbed: fp stays 0, not -1
    r, det = _car(kind)
    assert (det["counts"][:, 1] == 0).all() and list(det["counts"][-1]) == [80, 0, 0]
    assert r["bbox"]["R40"] == [100.0] * 3


def test_dontcare_partial_cover_is_not_enough():
    _, det = _car("dontcare_partial")  # inter / area_dt = 1/3 <= 0.7
    assert list(det["counts"][-1]) == [80, 1, 0]


def test_aos_against_bbox_ap():
    for kind in ("all_found", "fp_in_front"):
        r, _ = _car(kind)
        assert all(abs(a - b) < 1e-9 for a, b in zip(r["aos"]["R40"] + r["aos"]["R11"], r["bbox"]["R40"] + r["bbox"]["R11"]))
        r, _ = _car(kind, d_alpha=np.pi)
        assert all(abs(a) < 1e-9 for a in r["aos"]["R40"] + r["aos"]["R11"])
        r, det = _car(kind, d_alpha=np.pi / 2)
        assert all(abs(a - b / 2) < 1e-9 for a, b in zip(r["aos"]["R40"] + r["aos"]["R11"], r["bbox"]["R40"] + r["bbox"]["R11"]))
        assert abs(det["similarity"][-1] - 40.0) < 1e-9


def test_loose_set_keeps_bbox_overlap_07_for_car():
    assert E.min_overlap("loose", "Car", "bbox") == 0.7 and E.min_overlap("loose", "Car", "aos") == 0.7
    assert E.min_overlap("loose", "Pedestrian", "bbox") == 0.5 and E.min_overlap("loose", "Cyclist", "aos") == 0.5
    assert E.min_overlap("loose", "Car", "bev") == 0.5 and E.min_overlap("strict", "Car", "3d") == 0.7  # BEV / 3-D unchanged
    for o in ("strict", "loose"):  # 2-D IoU 0.6: found at 0.5, not at 0.7
        r, det = _car("iou060", overlap=o)
        assert r["bbox"]["R40"] == [0.0] * 3 and det["n_valid_gt"] == 80 and len(det["thresholds"]) == 0
    frames = [RI.make_frame(g, dt) for g, dt in RI.hand_case("iou060")]
    assert RI.evaluate_combo(frames, "Car", 1, 0.5)["R40"] == 100.0


def test_dontcare_lowers_bev_ap_but_not_bbox_ap():
    pairs = RI.hand_case("dontcare_fp")
    res, det = R.evaluate([R.make_frame(g, d) for g, d in pairs], classes=("Car",), metrics=("bev",))
    assert list(det[("strict", "Car", "bev", 1)]["counts"][-1]) == [80, 1, 0]
    assert all(abs(v - 100 * 80 / 81) < 1e-12 for v in res["strict"]["Car"]["bev"]["R40"])
    r, _ = _car("dontcare_fp")
    assert r["bbox"]["R40"] == [100.0] * 3


def test_host_arrays_carry_dontcare_and_image_rows():
    rng = np.random.default_rng(4)
    for _ in range(10):
        gt, dt = RI.synthetic_frame(rng, int(rng.integers(0, 12)), int(rng.integers(0, 6)), n_dc=int(rng.integers(0, 3)))
        _, gmeta = E._gt_arrays(gt)
        dc = np.array([n == "DontCare" for n in gt.names], bool)
        assert np.array_equal((gmeta[:, 1] >> E.DONTCARE_BIT) & 1, dc.astype(np.int32))
        assert (gmeta[dc, 0] == E.CODE_OTHER).all()
        for lab in (gt, dt):
            rows = E._image_rows(lab)
            assert rows.dtype == np.float32 and rows.shape == (len(lab.names), 5)
            assert np.array_equal(rows[:, :4], lab.box2d.astype(np.float32)) and np.array_equal(rows[:, 4], lab.alpha.astype(np.float32))


def test_synthetic_generator_properties():
    rng = np.random.default_rng(9)
    pairs = [RI.synthetic_frame(rng, int(rng.integers(0, 16)), int(rng.integers(0, 6))) for _ in range(30)]
    names = {n for g, _ in pairs for n in g.names}
    assert names >= {"Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "DontCare"}
    absorbed_candidates = short_under_dc = 0
    for g, d in pairs:
        f = RI.make_frame(g, d)
        vals = np.concatenate([f["ov"]["bbox"].ravel(), f["dc_ratio"].ravel()])
        for t in (0.5, 0.7):
            assert (np.abs(vals - t) >= 1e-3).all()
        assert np.array_equal(g.alpha, g.alpha.astype(np.float32).astype(np.float64))
        if f["dc_ratio"].size:
            over = (f["dc_ratio"] > 0.7).any(1)
            absorbed_candidates += int(over.sum())
            short_under_dc += int((over & (f["dt_h"] < 25)).sum())
    assert absorbed_candidates > 10 and short_under_dc > 0
    res, det = RI.evaluate([RI.make_frame(g, d) for g, d in pairs], classes=("Car",), overlap_sets=("strict",))
    assert 0 < res["strict"]["Car"]["aos"]["R40"][1] < res["strict"]["Car"]["bbox"]["R40"][1]


def test_pass1_pass2_refuse_bad_combo_metrics_before_launch():
    """V3D_EINVAL for a combo metric outside 0..2 (pass 1 and pass 2) and for a bbox combo without the image arrays or the
    similarity output (pass 2), returned before any launch: the library loads without a GPU (test_capi_symbols.py).  Every
    pointer is a host buffer that the checks never read."""
    lib, einval = L.lib(), -1
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)

    def combos(metric):
        return (L.KittiCombo * 2)(L.KittiCombo(0, 3, 1, E.METRIC_BEV, 0.7), L.KittiCombo(0, 3, 1, metric, 0.7))

    def pass1(c):
        return lib.v3d_kitti_eval_pass1(p, p, p, p, p, p, p, 1, 1, 1, 1, c, 2, 1, p, p, p, None)

    def pass2(c, img=p, sim=p):
        return lib.v3d_kitti_eval_pass2(p, p, img, p, p, p, img, p, p, 1, 1, 1, 1, c, 2, p, p, p, sim, None)

    for bad in (-1, 3):
        assert pass1(combos(bad)) == einval and pass2(combos(bad)) == einval
    assert pass2(combos(E.METRIC_BBOX), img=None) == einval
    assert pass2(combos(E.METRIC_BBOX), sim=None) == einval

"""CPU: the COCO-style KITTI AP (overlap set "coco", vision3d_amd/evaluation/kitti.py): the sweep levels and their float32
rounding, the evaluator's combos and summary header, the CLI's --overlaps, and the C entry points' combo limit above the 64
combos of one by-value table."""
import ctypes

import numpy as np
import pytest

from vision3d_amd import _lib as L
from vision3d_amd.evaluation import KittiEvaluator
from vision3d_amd.evaluation import __main__ as cli
from vision3d_amd.evaluation import kitti as E

V3D_OK, V3D_EINVAL, V3D_EUNSUPPORTED = 0, -1, -3


def test_levels_and_their_float32_rounding():
    for c, (lo, hi) in (("Car", (0.5, 0.95)), ("Pedestrian", (0.25, 0.70)), ("Cyclist", (0.25, 0.70))):
        exact = np.linspace(lo, hi, 10)
        got = E.COCO_LEVELS[c]
        assert got.dtype == np.float32 and got.shape == (10,)
        assert np.array_equal(got, exact.astype(np.float32))
        for g, x in zip(got, exact):  # the nearest float32: no neighbour is closer
            below, above = np.nextafter(g, np.float32(-1)), np.nextafter(g, np.float32(2))
            assert abs(float(g) - x) <= min(abs(float(below) - x), abs(float(above) - x))
    # the levels that coincide with the official minimum overlaps are the same float32 values
    assert E.COCO_LEVELS["Car"][0] == np.float32(0.5) and E.COCO_LEVELS["Car"][4] == np.float32(0.7)
    for c in ("Pedestrian", "Cyclist"):
        assert E.COCO_LEVELS[c][0] == np.float32(0.25) and E.COCO_LEVELS[c][5] == np.float32(0.5)
    assert float(E.COCO_LEVELS["Car"][9]) == pytest.approx(0.95, abs=1e-7)


def test_evaluator_accepts_coco():
    ev = KittiEvaluator(overlaps=("coco",))
    assert len(ev.combos) == 3 * 2 * 3 * 10
    assert sorted({k for *_, k in ev.combos}) == list(range(10))
    ev = KittiEvaluator(metrics=("bbox", "bev", "3d", "aos"), overlaps=("strict", "loose", "coco"))
    assert len(ev.combos) == 2 * 3 * 3 * 3 + 3 * 3 * 3 * 10  # 324: beyond one by-value table of 64
    with pytest.raises(ValueError):
        KittiEvaluator(overlaps=("coco", "tight"))
    # the default stays strict / loose
    assert KittiEvaluator().overlaps == ("strict", "loose")


def test_summary_header_and_empty_result():
    ev = KittiEvaluator(metrics=("bbox", "bev", "3d", "aos"), overlaps=("strict", "coco"))
    res = ev.compute()  # no frames: no device work
    assert res["coco"]["Car"]["bev"] == {"R11": [0.0] * 3, "R40": [0.0] * 3}
    det = ev.details[("coco", "Pedestrian", "bbox", 2)]
    assert np.array_equal(det["levels"], E.COCO_LEVELS["Pedestrian"]) and det["ap"].shape == (10, 2)
    assert det["aos"].shape == (10, 2) and len(det["per_level"]) == 10
    assert det["per_level"][3]["n_valid_gt"] == 0 and len(det["per_level"][3]["counts"]) == 0
    lines = ev.summary(r11=True).splitlines()
    assert len(lines) == 12
    zeros = ", ".join(["0.0000"] * 3)
    assert lines[0] == f"Car AP_R11@0.70, 0.70, 0.70: bbox: {zeros}  bev: {zeros}  3d: {zeros}  aos: {zeros}"
    assert lines[6] == f"Car coco AP_R11@0.50:0.05:0.95: bbox: {zeros}  bev: {zeros}  3d: {zeros}  aos: {zeros}"
    assert lines[7].startswith("Car coco AP_R40@0.50:0.05:0.95: bbox: ")
    assert lines[9].startswith("Pedestrian coco AP_R40@0.25:0.05:0.70: ")
    assert lines[11].startswith("Cyclist coco AP_R40@0.25:0.05:0.70: ")
    assert E.coco_header("Car") == "coco AP_R40@0.50:0.05:0.95"
    # without coco the summary is what it was
    plain = KittiEvaluator()
    plain.compute()
    assert [ln.split(":")[0] for ln in plain.summary().splitlines()] == \
        ["Car AP_R40@0.70, 0.70", "Pedestrian AP_R40@0.50, 0.50", "Cyclist AP_R40@0.50, 0.50",
         "Car AP_R40@0.50, 0.50", "Pedestrian AP_R40@0.25, 0.25", "Cyclist AP_R40@0.25, 0.25"]


def test_cli_overlaps_option():
    _, args = cli.parse_args(["--labels", "l", "--results", "r"])
    assert args.overlaps == ("strict", "loose") and args.metrics == ("bev", "3d")
    _, args = cli.parse_args(["--labels", "l", "--results", "r", "--overlaps", "strict, loose,coco", "--metrics", "bbox,aos"])
    assert args.overlaps == ("strict", "loose", "coco") and args.metrics == ("bbox", "aos")
    _, args = cli.parse_args(["--labels", "l", "--results", "r", "--overlaps", "coco"])
    assert args.overlaps == ("coco",)


def test_entry_points_take_more_than_64_combos():
    """n_frames = 0 with 100 or 300 combos is V3D_OK (one by-value table holds 64); thresholds and AP (no frame count) pass
    the combo limit and stop at the null output; beyond V3D_KITTI_MAX_COMBOS (1 024) every entry point is V3D_EUNSUPPORTED.
    All returned before any launch: the library loads without a GPU.  Every pointer is a host buffer the checks never read."""
    lib = L.lib()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)

    def combos(n):
        return (L.KittiCombo * n)(*[L.KittiCombo(k % 3, -1, k % 3, k % 3, 0.5 + 0.001 * k) for k in range(n)])

    for n in (100, 300):
        c = combos(n)
        assert lib.v3d_kitti_eval_pass1(p, p, p, p, p, p, p, 1, 0, 1, 1, c, n, 1, p, p, p, None) == V3D_OK
        assert lib.v3d_kitti_eval_pass2(p, p, p, p, p, p, p, p, p, 1, 0, 1, 1, c, n, p, p, p, p, None) == V3D_OK
        assert lib.v3d_kitti_eval_thresholds(p, 1, p, p, n, None, p, None) == V3D_EINVAL
        assert lib.v3d_kitti_eval_ap(p, None, p, n, None, None, None) == V3D_EINVAL
    n = 1025
    c = combos(n)
    assert lib.v3d_kitti_eval_pass1(p, p, p, p, p, p, p, 1, 0, 1, 1, c, n, 1, p, p, p, None) == V3D_EUNSUPPORTED
    assert lib.v3d_kitti_eval_pass2(p, p, p, p, p, p, p, p, p, 1, 0, 1, 1, c, n, p, p, p, p, None) == V3D_EUNSUPPORTED
    assert lib.v3d_kitti_eval_thresholds(p, 1, p, p, n, None, p, None) == V3D_EUNSUPPORTED
    assert lib.v3d_kitti_eval_ap(p, None, p, n, None, None, None) == V3D_EUNSUPPORTED

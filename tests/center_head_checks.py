"""The comparisons of the centre-head tests against tests/center_head_ref.py, shared by the CPU tests (torch statements on host tensors)
and the GPU tests (native calls and torch statements on the device).  numpy only.  Every function prints its largest figures before
it asserts, and returns them.

Bars (derived for the shapes of tests/center_head_cases.py):
    heat        exactly 1 at live centres, exactly 0 outside every window; elsewhere 4e-6 relative: the exponent is at most 9 in
                magnitude and carries at most three fp32 roundings of 6e-8 each (1.6e-6), plus 2 ulp of expf (2.4e-7)
    reg[0:2]    4e-5 absolute: two fp32 roundings at magnitude below 256 (3e-5)
    reg[2:8]    4 fp32 ulps of the value or 5e-7 absolute
    losses      1e-5 relative; gradient 1e-5 of its largest entry (the bars of tests/test_gpu_proposal_loss.py)
    decode      x, y 3e-5 absolute (4 ulp at 80 m); w, l, h 1e-6 relative; yaw, score 1e-6 absolute; pad slots exact zeros"""
import numpy as np


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def check_targets(got, ref, what=""):
    """got: (heat, ind, mask, cls, reg) numpy arrays; ref: center_head_ref.targets(...)."""
    heat, ind, mask, cls, reg = (np.asarray(a) for a in got)
    rows = ref["ind"].shape[1]
    np.testing.assert_array_equal(ind[:, :rows], ref["ind"])
    np.testing.assert_array_equal(mask[:, :rows], ref["mask"])
    np.testing.assert_array_equal(cls[:, :rows], ref["cls"])
    want = ref["heat"]
    assert heat.dtype == np.float32 and heat.shape == want.shape
    assert (heat[~ref["window"]] == 0).all(), f"{what}: heat outside every window is not an exact zero"
    assert (heat[want == 1] == 1).all() and int((want == 1).sum()) >= 1, f"{what}: a centre is not exactly 1"
    inside = ref["window"]
    rel = float((np.abs(heat[inside] - want[inside]) / want[inside]).max()) if inside.any() else 0.0
    m = ref["mask"] > 0
    e_off = float(np.abs(reg[:, :rows, :2][m] - ref["reg"][..., :2][m]).max()) if m.any() else 0.0
    rest, rest_ref = reg[:, :rows, 2:][m].astype(np.float64), ref["reg"][..., 2:][m]
    err = np.abs(rest - rest_ref)
    e_rest_ulp = float((err / ulp32(rest_ref)).max()) if m.any() else 0.0
    e_rest_abs = float(err.max()) if m.any() else 0.0
    print(f"[center targets {what}] heat rel {rel:.3e} (bar 4e-6), offsets abs {e_off:.3e} (bar 4e-5), rest {e_rest_ulp:.2f} ulp / "
          f"{e_rest_abs:.3e} abs (bar 4 ulp or 5e-7)")
    assert rel <= 4e-6, f"{what}: heat relative error {rel:.3e}"
    assert e_off <= 4e-5, f"{what}: offset error {e_off:.3e}"
    assert ((err <= 4 * ulp32(rest_ref)) | (err <= 5e-7)).all(), f"{what}: reg error {e_rest_ulp:.2f} ulp / {e_rest_abs:.3e}"
    assert (reg[:, :rows][~m] == 0).all(), f"{what}: the reg row of an object that is not live is not zero"
    return dict(heat_rel=rel, offsets_abs=e_off, rest_ulp=e_rest_ulp, rest_abs=e_rest_abs)


def check_loss(hm, rl, d_hm, d_reg, ref, n_cls, what=""):
    """hm, rl: the two losses; d_hm / d_reg: their gradients with respect to the fused maps (same shape), numpy."""
    e_hm, e_rl = abs(float(hm) - ref["hm"]) / abs(ref["hm"]), abs(float(rl) - ref["reg"]) / abs(ref["reg"])
    g_hm = float(np.abs(d_hm - ref["d_hm"]).max() / np.abs(ref["d_hm"]).max())
    g_rl = float(np.abs(d_reg - ref["d_reg"]).max() / np.abs(ref["d_reg"]).max())
    print(f"[center loss {what}] hm rel {e_hm:.3e}, reg rel {e_rl:.3e} (bar 1e-5); gradient / max: heat {g_hm:.3e}, box {g_rl:.3e} (bar 1e-5)")
    assert e_hm <= 1e-5 and e_rl <= 1e-5, f"{what}: losses off by {e_hm:.3e} / {e_rl:.3e} relative"
    assert g_hm <= 1e-5 and g_rl <= 1e-5, f"{what}: gradients off by {g_hm:.3e} / {g_rl:.3e} of their maximum"
    assert (np.asarray(d_reg)[:, n_cls:][ref["d_reg"][:, n_cls:] == 0] == 0).all(), f"{what}: a box gradient away from the object cells"
    assert (np.asarray(d_reg)[:, :n_cls] == 0).all() and (np.asarray(d_hm)[:, n_cls:] == 0).all()
    return dict(hm_rel=e_hm, reg_rel=e_rl, grad_heat=g_hm, grad_box=g_rl)


def cells_of(boxes, scores, case):
    """The cell of every decoded slot, found by its z (copied bit for bit by decode; the cases' z channel holds distinct values):
    (B, n_cls, topk) int64, -1 for a pad slot (score 0)."""
    maps, n_cls, topk = case["maps"], case["n_cls"], case["topk"]
    B = maps.shape[0]
    z = np.asarray(boxes, np.float32).reshape(B, n_cls, topk, 7)[..., 2]
    s = np.asarray(scores).reshape(B, n_cls, topk)
    out = np.full((B, n_cls, topk), -1, np.int64)
    for b in range(B):
        zmap = maps[b, n_cls + 2].reshape(-1)
        order = np.argsort(zmap)
        pos = np.clip(np.searchsorted(zmap[order], z[b]), 0, len(order) - 1)
        found = order[pos]
        assert ((zmap[found] == z[b]) | (s[b] == 0)).all(), "a decoded z is no value of the map"
        out[b] = np.where(s[b] == 0, -1, found)
    return out


def check_decode(boxes, scores, case, what="", ref=None):
    ref = case["ref"] if ref is None else ref
    boxes, scores = np.asarray(boxes), np.asarray(scores)
    assert boxes.shape == ref["boxes"].shape and scores.shape == ref["scores"].shape
    np.testing.assert_array_equal(cells_of(boxes, scores, case), ref["cells"], err_msg=f"{what}: selected cells / their order")
    pad = (ref["cells"] < 0).reshape(scores.shape)
    assert (boxes[pad] == 0).all() and (scores[pad] == 0).all(), f"{what}: pad slots are not exact zeros"
    b, r = boxes[~pad].astype(np.float64), ref["boxes"][~pad]
    e_xy = float(np.abs(b[:, :2] - r[:, :2]).max())
    e_wlh = float((np.abs(b[:, 3:6] - r[:, 3:6]) / r[:, 3:6]).max())
    e_yaw = float(np.abs(b[:, 6] - r[:, 6]).max())
    e_s = float(np.abs(scores[~pad] - ref["scores"][~pad]).max())
    assert (b[:, 2] == r[:, 2]).all()
    print(f"[center decode {what}] xy abs {e_xy:.3e} (bar 3e-5), wlh rel {e_wlh:.3e} (bar 1e-6), yaw abs {e_yaw:.3e}, score abs {e_s:.3e} "
          f"(bar 1e-6); {int((~pad).sum())} boxes, {int(pad.sum())} pad slots")
    assert e_xy <= 3e-5 and e_wlh <= 1e-6 and e_yaw <= 1e-6 and e_s <= 1e-6, f"{what}: {e_xy:.3e} {e_wlh:.3e} {e_yaw:.3e} {e_s:.3e}"
    return dict(xy=e_xy, wlh=e_wlh, yaw=e_yaw, score=e_s)

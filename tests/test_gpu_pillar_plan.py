"""GPU: the pillar plan (cfg.PILLAR.PLAN) -- v3d_pillar_encode_planes / v3d_pillar_planes_clear (csrc/pillar.hip "the plan's front")
alone, runtime PillarPlan (vision3d_amd/pillar_plan.py), and Second's raw-point entry points on it.  tests/test_host_pillar_plan.py
holds the key's gating and the sanitizer run of the header.

Yardsticks of the op tests, all code that existed before the plan: the planes equal v3d_nchw_to_split_nhwc(canvas(v3d_pillar_encode
rows), the same arithmetic, the same entry) bit for bit, the bitmap equals v3d_bev_occupancy_bits of the same list, and the range
flag is 0 under an entry computed from the rows and 2 once a row passes entry[2].

The one tolerance (test_f16s_head_maps_against_float64): the fused head maps of the plan path and of the module path
head(rpn(vfe(item))) against model.double() on the CPU, largest |error| relative to the largest |reference| entry;
err_plan <= 2 * err_module.  Both run f16s arithmetic (2^-22 per product); the factor covers the one systematic difference -- the
plan's scale entries carry CALIB_HEADROOM_BITS of headroom where the modules take exact per-call maxima --, while a structural fault
(wrong pixel, stale plane, missed channel) is as large as the values themselves.  Measured on an MI355X (profiles/pillar_plan.txt):
see MEASURED below; the test prints both figures on every run.
"""
import copy

import numpy as np
import pytest
import torch

import pillar_cases as cases

pytestmark = pytest.mark.gpu

MEASURED = dict(err_plan=6.4e-8, err_module=6.4e-8)  # profiles/pillar_plan.txt (documentation; the test measures again on every run)

MAPS = [(20, 16), (7, 33), (5, 65)]  # one-word rows, and two word-boundary crossings
ROWS = [0, 1, 3, 4, 5, 257]          # around a workgroup's wave count, and many workgroups


# --------------------------------------------------------------------------------------------------------------------- op tests
def _net(H, W, P, seed):
    """PillarFeatureNet (C = 4, 128 channels) on an H x W map of 0.4 m pillars, seeded weights and BatchNorm statistics."""
    from gpu_util import randomize_bn
    from vision3d_amd.core.config import pillar_car_cfg
    from vision3d_amd.detector.pillar import PillarFeatureNet
    cfg = pillar_car_cfg()
    cfg.merge_from_dict(dict(GRID_BOUNDS=[0.0, 0.0, -3.0, 0.4 * W, 0.4 * H, 1.0], MAX_OCCUPANCY=P, MAX_VOXELS=400))
    torch.manual_seed(seed)
    net = PillarFeatureNet(cfg)
    randomize_bn(net, seed)
    assert net.map_shape == (H, W)
    return net.cuda().eval()


def _pillars(rng, M, cap, P, B, H, W):
    """`cap` rows: the first M in distinct cells (the last cell of the last frame among them), points inside their cell, occupancies
    from 1 to P; the rows behind them hold other live-looking pillars (they must not be touched when the count says M)."""
    cells = rng.choice(B * H * W, size=min(cap, B * H * W), replace=False)
    if cap > len(cells):
        cells = np.concatenate([cells, rng.choice(B * H * W, size=cap - len(cells))])
    if M:
        at = np.flatnonzero(cells == B * H * W - 1)
        if len(at):
            cells[at[0]] = cells[0]  # (a swap: the distinct cells stay distinct)
        cells[0] = B * H * W - 1
    co = np.zeros((cap, 4), np.int32)
    co[:, 0], co[:, 2], co[:, 3] = cells // (H * W), cells % (H * W) // W, cells % W
    occ = rng.integers(1, P + 1, size=cap).astype(np.int32)
    if cap >= 2:
        occ[0], occ[1] = P, 1
    feat = np.zeros((cap, P, 4), np.float32)
    for m in range(cap):
        n = int(occ[m])
        u = rng.uniform(0.05, 0.95, size=(n, 3))
        feat[m, :n, 0] = (co[m, 3] + u[:, 0]) * 0.4
        feat[m, :n, 1] = (co[m, 2] + u[:, 1]) * 0.4
        feat[m, :n, 2] = -3.0 + u[:, 2] * 4.0
        feat[m, :n, 3] = rng.uniform(0.0, 1.0, size=n)
    return torch.from_numpy(feat).cuda(), torch.from_numpy(occ).cuda(), torch.from_numpy(co).cuda()


def _rows(net, feat, occ, co):
    from vision3d_amd.detector.pillar import pillar_encode
    scale, shift = net._folded()
    return pillar_encode(feat, occ, co, net.geom, net.linear.weight.detach(), scale, shift)


def _yardstick(net, feat, occ, co, keep, B, prec, entry):
    """The parent's path on the rows `keep` names: v3d_pillar_encode -> canvas -> v3d_nchw_to_split_nhwc(prec, entry); and
    v3d_bev_occupancy_bits of the same list.  -> (hi, lo (B, H, W, 128) int16, bitmap)."""
    from vision3d_amd import _lib as L
    H, W = net.map_shape
    f, o, c = feat[keep].contiguous(), occ[keep].contiguous(), co[keep].contiguous()
    n = f.shape[0]
    bev = net.canvas(_rows(net, f, o, c), c, B).contiguous() if n else torch.zeros((B, 128, H, W), device="cuda")
    hi, lo = torch.empty((2, B, H, W, 128), dtype=torch.int16, device="cuda")
    L.check(L.lib().v3d_nchw_to_split_nhwc(L.ptr(bev), B, 128, H, W, L.ptr(hi), L.ptr(lo), prec, L.ptr(entry), L.stream_ptr()), "split")
    bits = torch.full((B * H, (W + 31) // 32), -1, dtype=torch.int32, device="cuda")
    if n:
        L.check(L.lib().v3d_bev_occupancy_bits(L.ptr(c), L.ptr(torch.tensor([n], dtype=torch.int32, device="cuda")), n, B, H, W, L.ptr(bits),
                                               L.stream_ptr()), "bits")
    return hi, lo, bits


def _entry(rows, prec):
    from vision3d_amd.runtime import act_entry_from_tensor
    if prec == 0:
        return None
    return act_entry_from_tensor(rows) if rows.numel() else torch.tensor([1.0, 1.0, 32768.0, 0.0], device="cuda")


def _encode_planes(net, feat, occ, co, count, B, prec, entry, hi=None, lo=None, bits=None, flag=None, clear=True):
    """v3d_pillar_planes_clear (no list) + v3d_pillar_encode_planes into zeroed planes (or the caller's).  -> (hi, lo, bits, flag)."""
    from vision3d_amd import _lib as L
    H, W = net.map_shape
    cap, P, C = feat.shape
    if hi is None:
        hi, lo = torch.zeros((2, B, H, W, 128), dtype=torch.int16, device="cuda")
    if bits is None:
        bits = torch.zeros((B * H, (W + 31) // 32), dtype=torch.int32, device="cuda")  # (NOT all ones: the clear call must make it so)
    if flag is None:
        flag = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    n_dev = torch.tensor([count], dtype=torch.int32, device="cuda")
    scale, shift = net._folded()
    lib = L.lib()
    if clear:
        L.check(lib.v3d_pillar_planes_clear(None, None, cap, B, H, W, 128, L.ptr(hi), L.ptr(lo), L.ptr(bits), L.ptr(flag), L.stream_ptr()), "clear")
    L.check(lib.v3d_pillar_encode_planes(L.ptr(feat), L.ptr(occ), L.ptr(co), L.ptr(n_dev), cap, P, C, L.host_f32(net.geom),
                                         L.ptr(net.linear.weight.detach()), 128, L.ptr(scale), L.ptr(shift), B, H, W, prec, L.ptr(entry),
                                         L.ptr(flag) if prec else None, L.ptr(hi), L.ptr(lo), L.ptr(bits), L.stream_ptr()), "encode_planes")
    return hi, lo, bits, flag


@pytest.mark.parametrize("prec", [0, 1], ids=["bf16x3", "f16s"])
@pytest.mark.parametrize("H,W", MAPS)
def test_planes_bitmap_and_flag_against_the_parent_path(H, W, prec):
    rng = np.random.default_rng([11, H, W, prec])
    checked = 0
    for P in (1, 32, 64):
        net = _net(H, W, P, seed=P)
        for B in (1, 3):
            for M in ROWS:
                M = min(M, B * H * W)
                for cap in sorted({M, M + 6}):
                    feat, occ, co = _pillars(rng, M, cap, P, B, H, W)
                    counts = {M}
                    if P == 32:  # the device count below, equal to and above the capacity (and the rows behind it live-looking)
                        counts |= {max(M - 2, 0), cap, cap + 9}
                    for count in sorted(counts):
                        live = min(count, cap)
                        if len(torch.unique((co[:live, 0] * H + co[:live, 2]) * W + co[:live, 3])) < live:
                            continue  # (live rows behind the M distinct cells share pixels: the repeated-pixel test's subject)
                        keep = torch.arange(live, device="cuda")
                        entry = _entry(_rows(net, feat[:live].contiguous(), occ[:live].contiguous(), co[:live].contiguous()), prec) if live else _entry(feat[:0], prec)
                        want = _yardstick(net, feat, occ, co, keep, B, prec, entry)
                        hi, lo, bits, flag = _encode_planes(net, feat, occ, co, count, B, prec, entry)
                        what = dict(P=P, B=B, M=M, cap=cap, count=count)
                        assert torch.equal(hi, want[0]) and torch.equal(lo, want[1]), what
                        assert torch.equal(bits, want[2]), what
                        assert int(flag.item()) == 0, what  # reset by the clear call; the rows lie inside an entry made from them
                        checked += 1
    print("pillar-plan-op-cases", dict(map=(H, W), prec=prec, checked=checked))
    assert checked >= 60


def test_range_flag_is_raised_by_a_row_beyond_the_limit():
    rng = np.random.default_rng(5)
    net = _net(20, 16, 32, seed=3)
    feat, occ, co = _pillars(rng, 37, 37, 32, 1, 20, 16)
    entry = _entry(_rows(net, feat, occ, co), 1)
    _, _, _, flag = _encode_planes(net, feat, occ, co, 37, 1, 1, entry)
    assert int(flag.item()) == 0
    loud = feat.clone()
    loud[29, :, 3] *= 1.0e5  # one pillar's reflectance: its row passes entry[2] = 2^15 / s (at most four times the calibrated maximum)
    rows = _rows(net, loud, occ, co)
    assert float(rows[29].max()) > float(entry[2]) and float(rows[:29].max()) <= float(entry[2])
    hi, lo, bits, flag = _encode_planes(net, loud, occ, co, 37, 1, 1, entry)
    assert int(flag.item()) == 2
    _, _, _, flag = _encode_planes(net, loud, occ, co, 29, 1, 1, entry)  # ... and not by a row behind the count
    assert int(flag.item()) == 0
    # bf16x3 has no entry and touches no flag
    flag = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    _encode_planes(net, loud, occ, co, 37, 1, 0, None, flag=flag, clear=False)
    assert int(flag.item()) == 7


@pytest.mark.parametrize("prec", [0, 1], ids=["bf16x3", "f16s"])
def test_rows_outside_the_map_are_skipped(prec):
    """A hand-fed list: rows whose (b, y, x) lies outside the map on every side (and far outside) store nothing and mark nothing --
    the planes sit between guard bands that must stay untouched -- and a row's z index does not move its pixel."""
    rng = np.random.default_rng(9)
    H, W, B = 7, 33, 3
    net = _net(H, W, 8, seed=4)
    feat, occ, co = _pillars(rng, 40, 40, 8, B, H, W)
    bad = {3: (-1, 0, 0, 0), 7: (B, 0, 0, 0), 11: (0, 0, -1, 0), 12: (0, 0, H, 0), 20: (0, 0, 0, -1), 21: (0, 0, 0, W),
           30: (2 ** 31 - 1, 0, 2 ** 31 - 1, 2 ** 31 - 1), 31: (0, 0, -2 ** 31, 5)}
    for m, c in bad.items():
        co[m] = torch.tensor(c, dtype=torch.int32)
    co[5, 1], co[6, 1] = 3, -2  # z indices of in-map rows: ignored, as canvas() ignores them
    keep = torch.tensor([m for m in range(40) if m not in bad], device="cuda")
    entry = _entry(_rows(net, feat[keep].contiguous(), occ[keep].contiguous(), co[keep].contiguous()), prec)
    want = _yardstick(net, feat, occ, co, keep, B, prec, entry)  # (canvas() writes every row at z = 0 whatever its z index holds)
    n, pad = B * H * W * 128, 4096
    guard = torch.full((2, n + 2 * pad), 0x5A5A, dtype=torch.int16, device="cuda")
    guard[:, pad:pad + n] = 0
    hi, lo = guard[0, pad:pad + n].view(B, H, W, 128), guard[1, pad:pad + n].view(B, H, W, 128)
    wpr = (W + 31) // 32
    gbits = torch.full((B * H * wpr + 128,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    bits = gbits[64:64 + B * H * wpr].view(B * H, wpr)
    _encode_planes(net, feat, occ, co, 40, B, prec, entry, hi=hi, lo=lo, bits=bits)
    assert torch.equal(hi, want[0]) and torch.equal(lo, want[1]) and torch.equal(bits, want[2])
    assert bool((guard[:, :pad] == 0x5A5A).all()) and bool((guard[:, pad + n:] == 0x5A5A).all())
    assert bool((gbits[:64] == 0x5A5A5A5A).all()) and bool((gbits[64 + B * H * wpr:] == 0x5A5A5A5A).all())


def test_a_repeated_pixel_holds_either_row():
    """Two rows on one pixel (the voxelizer produces none): every stored 16-bit piece is the piece of one of the two rows, as .dense()
    leaves one of them; every other pixel is as without the repeat."""
    rng = np.random.default_rng(13)
    H, W = 20, 16
    net = _net(H, W, 8, seed=5)
    feat, occ, co = _pillars(rng, 12, 12, 8, 1, H, W)
    co[9] = co[2]
    first = torch.tensor([m for m in range(12) if m != 9], device="cuda")
    second = torch.tensor([m for m in range(12) if m != 2], device="cuda")
    for prec in (0, 1):
        entry = _entry(_rows(net, feat, occ, co), prec)
        a, b = _yardstick(net, feat, occ, co, first, 1, prec, entry), _yardstick(net, feat, occ, co, second, 1, prec, entry)
        hi, lo, bits, _ = _encode_planes(net, feat, occ, co, 12, 1, prec, entry)
        y, x = int(co[2, 2]), int(co[2, 3])
        assert not torch.equal(a[0][0, y, x], b[0][0, y, x])
        assert bool(((hi == a[0]) | (hi == b[0])).all()) and bool(((lo == a[1]) | (lo == b[1])).all())
        assert torch.equal(bits, a[2]) and torch.equal(bits, b[2])


def test_unsupported_shapes_launch_nothing():
    from vision3d_amd import _lib as L
    lib, z = L.lib(), torch.zeros(64, device="cuda")
    geom = L.host_f32(cases.geometry())
    for P, C, CH in ((65, 4, 128), (0, 4, 128), (8, 2, 128), (8, 9, 128), (8, 4, 64), (8, 4, 96)):
        assert lib.v3d_pillar_encode_planes(L.ptr(z), L.ptr(z), L.ptr(z), L.ptr(z), 1, P, C, geom, L.ptr(z), CH, L.ptr(z), L.ptr(z), 1, 20, 16, 0,
                                            None, None, L.ptr(z), L.ptr(z), L.ptr(z), L.stream_ptr()) == -3
    torch.cuda.synchronize()
    assert float(z.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------ plan and model
def _clouds(seeds, n_points=4096):
    """Synthetic clouds moved into the tiny grid's bounds (x in [0, 6.4), y in [-4, 4)), as tests/test_gpu_pillar.py's."""
    from vision3d_amd import synth
    out = []
    for s in seeds:
        cloud = synth.make_cloud(s, n_points=n_points).copy()
        cloud[:, 0] = cloud[:, 0] / 70.4 * 6.4
        cloud[:, 1] = cloud[:, 1] / 40.0 * 4.0
        out.append(torch.from_numpy(cloud.astype(np.float32)).cuda())
    return out


def _model(seed=0, precision=None):
    from gpu_util import randomize_bn
    from vision3d_amd.core import AnchorGenerator
    from vision3d_amd.detector import Second
    cfg = cases.tiny_cfg()
    cfg.PILLAR.PLAN = True
    torch.manual_seed(seed)
    model = Second(cfg).cuda()
    randomize_bn(model, seed)
    model.eval()
    if precision is not None:
        model.set_precision(precision)
    return cfg, model, AnchorGenerator(cfg).anchors.cuda()


def _item(cfg, clouds, anchors):
    from vision3d_amd.core import Preprocessor
    return Preprocessor(cfg)(dict(points=[c.clone() for c in clouds], anchors=anchors))


def _same(a, b, nonempty=True):
    """Bit for bit (floats compared as their bit patterns: a NaN equals itself)."""
    assert len(a) == len(b) == 4 and (len(a[0]) > 0 or not nonempty)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y)


def _offsets(clouds):
    return [0] + np.cumsum([c.shape[0] for c in clouds]).tolist()


def test_plan_voxelizer_equals_the_preprocessor():
    from vision3d_amd.pillar_plan import PillarPlan
    cfg, model, anchors = _model()
    clouds = _clouds((0, 1))
    item = _item(cfg, clouds, anchors)
    plan = model.backbone_plan(2, 16384)
    assert isinstance(plan, PillarPlan) and plan is model.backbone_plan(2, 16384) and plan.device == anchors.device
    with torch.no_grad():
        plan.forward_split(torch.cat(clouds), _offsets(clouds))
    slots, occ, co, count = plan.voxels()
    m = int(count.item())
    assert m == item["features"].shape[0] > 50
    assert torch.equal(slots[:m], item["features"]) and torch.equal(occ[:m], item["occupancy"]) and torch.equal(co[:m], item["coordinates"])
    with torch.no_grad():  # the fp32 map of the plan IS the module's
        assert torch.equal(model.bev_from_points(clouds), model.vfe(item))


def test_bf16x3_features_equal_the_module_path():
    cfg, model, anchors = _model(precision="bf16x3")
    clouds = _clouds((0, 1))
    item = _item(cfg, clouds, anchors)
    plan = model.backbone_plan(2, 16384)
    with torch.no_grad():
        hi, lo = plan.forward_split(torch.cat(clouds), _offsets(clouds))
        assert plan.bev_entry() is None and getattr(hi, "v3d_entry", None) is None
        got = model.dense_plan().forward(hi, lo, want_features=True, occ=plan.bev_occupancy(2))[1]
        want = model.rpn(model.vfe(item))
    assert got.shape == want.shape == (2, 128, cases.H, cases.W) and float(want.abs().max()) > 0
    assert torch.equal(got, want)
    assert int(plan.overflow_any().item()) == 0
    plan.check_overflow()


def test_f16s_head_maps_against_float64():
    from vision3d_amd.detector.proposal import fused_convs
    cfg, model, anchors = _model()
    assert model.precision == "fp32"
    clouds = _clouds((0, 1))
    item = _item(cfg, clouds, anchors)
    m64 = copy.deepcopy(model).cpu().double()  # the float64 statement: forward_torch, RPN.fused_forward, the head convolutions
    with torch.no_grad():
        plan_maps = model.fused_head_from_points(clouds)
        module_maps = model.head.native_head(model.rpn(model.vfe(item)))
        item64 = dict(features=item["features"].cpu(), occupancy=item["occupancy"].cpu(), coordinates=item["coordinates"].cpu(), batch_size=2)
        feats = m64.rpn.fused_forward(m64.vfe.forward_torch(item64))
        want = torch.cat([c(feats) for c in fused_convs(m64.head)], 1)
    assert plan_maps.shape == module_maps.shape == want.shape
    top = float(want.abs().max())
    err_plan = float((plan_maps.cpu().double() - want).abs().max()) / top
    err_module = float((module_maps.cpu().double() - want).abs().max()) / top
    print("pillar-plan-f16s-figures", dict(err_plan=err_plan, err_module=err_module, largest=top))
    assert err_plan <= 2 * err_module


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_persistent_planes_follow_the_frames(precision):
    """Frames A, B, A, ... through forward_split(persistent=True): B's pixels overlapping A's, disjoint from them, a superset of them,
    and no pixel at all.  Every result equals the non-persistent forward of that frame bit for bit, bitmap included."""
    cfg, model, anchors = _model(precision=precision)
    (a,) = _clouds((0,))
    left, right = a[a[:, 0] < 3.2], a[a[:, 0] >= 3.2]
    (other,) = _clouds((1,))
    frames = dict(A=left, overlap=a[(a[:, 0] > 1.6) & (a[:, 0] < 4.8)], disjoint=right, superset=torch.cat([left, other]),
                  empty=torch.full((64, 4), 1.0e30, device="cuda"), none=a[:0])
    plan = model.backbone_plan(1, 16384)
    h = cases.H

    def pixels(planes):
        return (planes[0][0] != 0).any(-1)
    with torch.no_grad():
        want = {}
        for name, pts in frames.items():
            hi, lo = plan.forward_split(pts, [0, pts.shape[0]])
            want[name] = (hi.clone(), lo.clone(), plan.bev_occupancy(1).clone())
        pa, po, pd, ps = (pixels(want[k]) for k in ("A", "overlap", "disjoint", "superset"))
        assert bool((pa & po).any()) and bool((pa & ~po).any()) and bool((po & ~pa).any()), "overlapping"
        assert not bool((pa & pd).any()) and bool(pd.any()), "disjoint"
        assert bool((ps | ~pa).all()) and bool((ps & ~pa).any()), "superset"
        assert not bool(pixels(want["empty"]).any()) and not bool(pixels(want["none"]).any())
        for name in ("A", "overlap", "A", "disjoint", "A", "superset", "A", "empty", "A", "none", "A", "A"):
            pts = frames[name]
            hi, lo = plan.forward_split(pts, [0, pts.shape[0]], persistent=True)
            assert hi.data_ptr() == plan.own_planes(1)[0].data_ptr()
            assert torch.equal(hi, want[name][0]) and torch.equal(lo, want[name][1]), name
            assert torch.equal(plan.bev_occupancy(1), want[name][2]) and plan.bev_occupancy(1).shape == (h, 1), name
            # a non-persistent call in between leaves the persistent planes and their list alone
            plan.forward_split(frames["disjoint"], [0, frames["disjoint"].shape[0]])
            assert torch.equal(plan.own_planes(1)[0], want[name][0])


def test_inference_points_is_the_native_tail_on_the_fused_maps():
    cfg, model, anchors = _model()
    clouds = _clouds((0, 1))
    with torch.no_grad():
        got = model.inference_points(clouds, anchors)
        maps = model.fused_head_from_points(clouds)
        _same(got, model.head.inference_native(maps, anchors))
        cls_map, reg_map = model.head_maps_from_points(clouds)
        assert cls_map.shape == (2, 1, 2, cases.H, cases.W) and reg_map.shape == (2, 1, 2, cases.H, cases.W, 7)
        torch_tail = model.inference_points(clouds, anchors, proposals="torch")  # the other form: the op-by-op tail on the same maps
        assert torch_tail[0].shape[1:] == (7,) and len(torch_tail[0]) == len(torch_tail[3]) > 0
    assert set(got[1].tolist()) == {0, 1}


def test_plan_follows_the_weights_and_refuses_training_batchnorm():
    cfg, model, anchors = _model()
    clouds = _clouds((0,))
    plan = model.backbone_plan(1, 16384)
    with torch.no_grad():
        model.inference_points(clouds, anchors)
        assert plan._calib == "done" and not plan.weights_changed()
        gen = plan.calibration_generation
        model.vfe.norm.bias.add_(0.25)
        assert plan.weights_changed()
        model.inference_points(clouds, anchors)  # new weights: taken, and the entry derived again on this frame
        assert not plan.weights_changed() and plan.calibration_generation == gen + 1
        plan.set_throughput_mode(True)
        model.vfe.norm.weight.mul_(1.5)
        model.vfe.train()
        with pytest.raises(RuntimeError, match="eval-mode BatchNorm"):
            plan.sync_weights()


def test_graphed_inference_equals_inference_points():
    cfg, model, anchors = _model()
    c0, c1 = _clouds((0, 1))
    _, other, _ = _model(seed=1)
    loud = c1.clone()
    loud[:, 3] *= 3.0e4  # reflectance far beyond the calibration frame's: the rows pass the entry's limit
    with torch.no_grad():
        run = model.graphed_inference(anchors, [4096])
        _same(run([c0]), model.inference_points([c0], anchors))
        _same(run([c1]), model.inference_points([c1], anchors))          # a replay
        short = c1[:3000]
        _same(run([short]), model.inference_points([short], anchors))    # shorter than the captured capacity: PAD_COORDINATE padding
        _same(run([c0]), model.inference_points([c0], anchors))          # ... whose pixels the next frame's clear removes
        graph = run.graph
        model.load_state_dict(other.state_dict())                        # other weights: captured again
        _same(run([c0]), model.inference_points([c0], anchors))
        assert run.graph is not graph
        gen = run.plan.calibration_generation
        got = [t.clone() for t in run([loud])]                           # RangeOverflow -> recalibrated on this frame -> run again
        assert run.plan.calibration_generation == gen + 1
        _same(got, model.inference_points([loud], anchors))
        fresh_cfg, fresh, _ = _model(seed=1)
        _same(got, fresh.inference_points([loud], anchors))              # what a model calibrated on that very frame returns
        _same(run([loud]), got)                                          # steady state: plain replays


def test_pipelined_inference_returns_the_graphed_results_in_order():
    cfg, model, anchors = _model()
    clouds = _clouds((0, 1, 2))
    with torch.no_grad():
        run = model.graphed_inference(anchors, [4096])
        want = [[t.clone() for t in run([c])] for c in clouds]
        pipe = model.pipelined_inference(anchors, [4096], depth=2)
        order = [0, 1, 2, 2, 0, 1]
        outs = []
        for i in order:
            r = pipe([clouds[i]])
            if r is not None:
                outs.append([t.clone() for t in r])
        outs += [[t.clone() for t in r] for r in pipe.flush()]
    assert len(outs) == len(order)
    for i, o in zip(order, outs):
        _same(o, want[i])


def test_full_size_frame():
    from vision3d_amd import synth
    from vision3d_amd.core import AnchorGenerator
    from vision3d_amd.core.config import pillar_plan_car_cfg
    from vision3d_amd.detector import Second
    cfg = pillar_plan_car_cfg()
    torch.manual_seed(0)
    model = Second(cfg).cuda().eval()
    anchors = AnchorGenerator(cfg).anchors.cuda()
    cloud = torch.from_numpy(synth.make_cloud(0, n_points=16384)).cuda()
    with torch.no_grad():
        eager = model.inference_points([cloud], anchors)
        graphed = model.graphed_inference(anchors, [16384])([cloud])
    torch.cuda.synchronize()
    plan = next(iter(model._plans.values()))
    assert plan.map_shape == (200, 176) and plan.P == 32 and 0 < int(plan.voxels(persistent=True)[3].item()) <= 12000
    assert all(bool(torch.isfinite(t.float()).all()) for t in list(eager) + list(graphed))
    assert len(eager[0]) == len(graphed[0])

"""GPU: the dense RPN's per-frame tile schedule (csrc/dense_conv.hip: D2Sched; runtime.DenseHeadState.sched).  A chain of three 3x3
128 -> 128 layers, a 1x1 up-conv and the head under one DenseHeadState: the first layer's launch builds the tile lists the other two
run.  Every layer's planes and the head maps equal, bit for bit, the same chain WITHOUT `occ` -- the every-pixel path, which the
other dense tests pin against float64 --, and the lists read back from the state equal the numpy restatement (dense_schedule_ref.py;
test_host_dense_schedule.py pins that against the definition).  Maps are small and off the tile grid: 12 x 40 = 3 x 3 tiles with a
ragged last row and column."""
import numpy as np
import pytest
import torch

import dense_schedule_ref as R
from gpu_util import randomize_bn
from vision3d_amd.core.config import second_car_cfg

pytestmark = pytest.mark.gpu

H, W = 12, 40
N_3X3 = 3
_PLANS = {}


class _Rpn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        down = []
        for _ in range(N_3X3):
            down += [torch.nn.Conv2d(128, 128, 3, padding=1, bias=False), torch.nn.BatchNorm2d(128), torch.nn.ReLU()]
        self.down_block = torch.nn.Sequential(*down)
        self.up_block = torch.nn.Sequential(torch.nn.Conv2d(128, 128, 1, bias=False), torch.nn.BatchNorm2d(128), torch.nn.ReLU())


def _split(x, precision, entry):
    """fp32 (b, 128, h, w) -> split planes under a GIVEN scale entry (one entry for all the frames of a test)"""
    from vision3d_amd import _lib as L
    from vision3d_amd.runtime import split_planes_like, tag_planes
    b, c, h, w = x.shape
    hi, lo = split_planes_like(b, h, w, c, x.device)
    L.check(L.lib().v3d_nchw_to_split_nhwc(L.ptr(x.contiguous()), b, c, h, w, L.ptr(hi), L.ptr(lo), L.PRECISIONS[precision], L.ptr(entry),
                                            L.stream_ptr()), "nchw_to_split_nhwc")
    tag_planes(hi, entry)
    return hi, lo


def _plan(precision):
    """one plan per arithmetic for the whole module: random weights, (f16s) calibrated on a full random frame"""
    if precision not in _PLANS:
        from vision3d_amd.detector import Second
        from vision3d_amd.runtime import DenseHeadPlan, act_entry_from_tensor
        torch.manual_seed(11)
        rpn = _Rpn()
        with torch.no_grad():
            for m in rpn.modules():
                if isinstance(m, torch.nn.Conv2d):
                    m.weight.normal_(0, (2.0 / (128 * m.kernel_size[0] ** 2)) ** 0.5)
        randomize_bn(rpn, 11)
        head = Second(second_car_cfg()).head
        with torch.no_grad():
            head.conv_cls.weight.normal_(0, 0.05)
            head.conv_reg.weight.normal_(0, 0.02)
        rpn, head = rpn.cuda().eval(), head.cuda().eval()
        plan = DenseHeadPlan(rpn, head, precision)
        entry = act_entry_from_tensor(torch.full((1,), 8.0, device="cuda")) if precision == "fp32" else None
        if entry is not None:
            g = torch.Generator().manual_seed(5)
            hi, lo = _split(torch.randn(1, 128, H, W, generator=g).cuda(), precision, entry)
            with torch.no_grad():
                plan.calibrate(hi, lo, entry)
        plan.sync_weights()
        _PLANS[precision] = (plan, entry)
    return _PLANS[precision]


def _frame(occ, seed, precision, entry):
    """bool (b, h, w) -> split planes that are zero off the occupied pixels, and the inverted bitmap on the device"""
    g = torch.Generator().manual_seed(seed)
    b, h, w = occ.shape
    x = torch.randn(b, 128, h, w, generator=g) * torch.from_numpy(occ).view(b, 1, h, w)
    hi, lo = _split(x.cuda(), precision, entry)
    return hi, lo, torch.from_numpy(R.occupancy_words(occ).view(np.int32)).cuda()


def _every_pixel(plan, hi, lo, entry):
    """the chain without occ: every 3x3 layer's planes (conv2d_split, fresh planes) and the head maps"""
    from vision3d_amd.runtime import conv2d_split
    planes, x = [], (hi, lo)
    for i in range(N_3X3):
        ly = plan.layers[i]
        x, _ = conv2d_split(x[0], x[1], ly["img"], ly["bias"], ly["relu"], ly["cin"], ly["cout"], ly["k"], pr=plan._pr(i, entry, None))
        planes.append(x)
    return planes, plan.forward(hi, lo, in_entry=entry)


def _check_frame(plan, state, occ, hi, lo, occ_w, entry, tag):
    """one frame through the scheduled chain: lists, state words, planes and maps"""
    n = R.n_tiles(*occ.shape)
    before = None if state.tiles is None else [t.cpu().numpy().copy() for t in state.tiles]
    maps = plan.forward(hi, lo, occ=occ_w, work=state, in_entry=entry)
    torch.cuda.synchronize()
    assert state.sched_first == 0 and sorted(state.sched) == [1, 2], tag
    if before is None:  # the state's first frame: every word starts at 1
        before = [np.ones(n, dtype=np.int32)] * N_3X3
    stale_lists = {}
    for i in range(N_3X3):
        live = R.live_tiles(occ, i + 1)
        assert np.array_equal(state.tiles[i][:n].cpu().numpy() != 0, live), (tag, "state words of layer", i)
        if i == 0:
            continue
        want_live, want_stale = R.schedule(occ, i + 1, before[i])
        got = state.sched[i].cpu().numpy()
        assert got.size == 2 + 2 * n and got[0] == want_live.size and got[1] == want_stale.size, (tag, i, got[:2], want_live.size, want_stale.size)
        assert np.array_equal(got[2:2 + got[0]], want_live), (tag, "live list of layer", i)
        assert np.array_equal(got[2 + n:2 + n + got[1]], want_stale), (tag, "stale list of layer", i)
        stale_lists[i] = want_stale
    ref_planes, ref_maps = _every_pixel(plan, hi, lo, entry)
    for i in range(N_3X3):
        assert torch.equal(state.out[i][0], ref_planes[i][0]) and torch.equal(state.out[i][1], ref_planes[i][1]), (tag, "planes of layer", i)
    assert torch.equal(maps, ref_maps), (tag, "head maps")
    return maps.clone(), stale_lists


def _bitmaps(b):
    rng = np.random.default_rng(b)
    out = {"empty": np.zeros((b, H, W), dtype=bool), "full": np.ones((b, H, W), dtype=bool)}
    c = np.zeros((b, H, W), dtype=bool)
    c[0, 0, 0] = c[0, 0, W - 1] = c[b - 1, H - 1, 0] = c[b - 1, H - 1, W - 1] = True
    out["corners"] = c
    # the liveness edge: a pixel d cells right of / below tile 0's last column / row makes the tile live from reach d on --
    # d = r is "exactly reach", d = r + 1 "reach + 1" for the layers' reaches r = 1, 2, 3
    for d in (1, 2, 3, 4):
        e = np.zeros((b, H, W), dtype=bool)
        e[0, 2, 15 + d] = True
        out[f"edge x {d}"] = e
        e = np.zeros((b, H, W), dtype=bool)
        e[b - 1, 4 + d, 3] = True
        out[f"edge y {d}"] = e
    out["random"] = rng.random((b, H, W)) < 0.10
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("name", sorted(_bitmaps(1)))
def test_scheduled_chain_equals_every_pixel(name, b, precision):
    plan, entry = _plan(precision)
    occ = _bitmaps(b)[name]
    hi, lo, occ_w = _frame(occ, 100 + b, precision, entry)
    with torch.no_grad():
        state = plan.new_state(hi.device)
        _check_frame(plan, state, occ, hi, lo, occ_w, entry, name)
        _check_frame(plan, state, occ, hi, lo, occ_w, entry, name + " (again: nothing is stale)")
        assert all(int(state.sched[i][1]) == 0 for i in state.sched)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_tiles_go_live_dead_live(precision):
    """frames A -> B -> A on one state, disjoint occupied regions: B's stale lists are exactly A's live tiles that B does not have"""
    plan, entry = _plan(precision)
    a, bb = np.zeros((2, H, W), dtype=bool), np.zeros((2, H, W), dtype=bool)
    a[0, 1, 2] = a[1, 10, 38] = True
    bb[0, 11, 37] = bb[1, 0, 20] = True
    frames = {"A": (a,) + _frame(a, 1, precision, entry), "B": (bb,) + _frame(bb, 2, precision, entry)}
    with torch.no_grad():
        state = plan.new_state(frames["A"][1].device)
        for step, name in enumerate(("A", "B", "A")):
            occ, hi, lo, occ_w = frames[name]
            _, stale = _check_frame(plan, state, occ, hi, lo, occ_w, entry, f"{name} (frame {step})")
            if step:
                prev = frames["A" if name == "B" else "B"][0]
                for i in (1, 2):
                    gone = R.live_tiles(prev, i + 1) & ~R.live_tiles(occ, i + 1)
                    assert gone.any() and np.array_equal(stale[i], np.flatnonzero(gone)), (name, i)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_more_live_tiles_than_workgroups(precision):
    """85 x 272, every pixel occupied: 17 x 17 = 289 live tiles on a grid of at most one workgroup per CU (256): the stride loop"""
    plan, entry = _plan(precision)
    occ = np.ones((1, 85, 272), dtype=bool)
    hi, lo, occ_w = _frame(occ, 9, precision, entry)
    with torch.no_grad():
        state = plan.new_state(hi.device)
        _check_frame(plan, state, occ, hi, lo, occ_w, entry, "289 tiles")
        assert int(state.sched[1][0]) == 289


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_captured_graph_replays_two_frames(precision):
    plan, entry = _plan(precision)
    maps = _bitmaps(2)
    frames = [(maps["random"],) + _frame(maps["random"], 21, precision, entry), (maps["corners"],) + _frame(maps["corners"], 22, precision, entry)]
    with torch.no_grad():
        want = []
        eager = plan.new_state(frames[0][1].device)
        for occ, hi, lo, occ_w in frames:
            want.append(_check_frame(plan, eager, occ, hi, lo, occ_w, entry, "eager")[0])
        s_hi, s_lo, s_occ = (t.clone() for t in frames[0][1:])
        state = plan.new_state(s_hi.device)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            plan.forward(s_hi, s_lo, occ=s_occ, work=state, in_entry=entry)  # (warm-up: allocations, the background)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = plan.forward(s_hi, s_lo, occ=s_occ, work=state, in_entry=entry)
        for k in (0, 1, 0):
            for dst, src in zip((s_hi, s_lo, s_occ), frames[k][1:]):
                dst.copy_(src)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want[k]), k
            for i in (1, 2):
                got = state.sched[i].cpu().numpy()
                assert np.array_equal(got[2:2 + got[0]], np.flatnonzero(R.live_tiles(frames[k][0], i + 1))), (k, i)
        del graph

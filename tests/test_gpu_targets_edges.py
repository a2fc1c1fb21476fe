"""v3d_assign_targets and v3d_direction_targets (csrc/targets.hip) against tests/targets_ref.py -- float64, an IoU clipper of its own --
on the cases of tests/targets_cases.py: G_cls, M_cls, M_reg and matches equal the reference exactly, on EVERY anchor; G_reg at the
positives to rtol 1e-5 / atol 1e-6 of float64 (the bar of tests/test_gpu_targets.py) and exactly 0 elsewhere; G_dir exactly; two calls
give the same bits, and so does a call without `matches`.  Every call gets a workspace filled with 0xFF and outputs filled with
sentinels: nothing is read before it is written, nothing is left unwritten.  tests/test_host_targets_ref.py shows on the host that the
cases are well-posed (margins of 1e-5 and more, the named ties exact in fp32 and float64) and which case notices which mistake.

Which run reaches what (run ids of tests/targets_cases.py):
  grid-A{1,63,64,65,255,256,257,513}   the last workgroup empty but for one thread, full, one over; from 257 on a ground truth's maximum is
                                       an atomicMax from two workgroups
  band-{at_lo,at_hi,above_lo,above_hi}  best == lo, best == hi, and one float32 step under each
  first_max[-reversed]                  two ground truths tie at every anchor: the strict `>`; the staged order differs from the input's
  interleaved-c{3,16}                   16 classes (the limit), an empty class, class ids outside [0, n_cls)
  low_quality-*[-rule_off]              positive by the rule alone; bit-identical anchors in two workgroups both attain the maximum; a
                                        ground truth that overlaps nothing makes every anchor positive
  crowd-{128,129,200,257}, crowd-mixed  a class of more than 128 ground truths is walked in chunks: the decisive one is the last; the mixed
                                        crowd has positives on both sides of the chunk boundary, also through ProposalTargetAssigner
  encode-{yaw,size}                     the wrap at 0, just under 0, +-(float)pi, +-2 (float)pi; logf of ratios from 1/8 to 8
  direction n = 262 145, 300 000        the second trip of ta_direction_kernel's loop; matches -1, n_gt and 2^40 give 0

Largest G_reg error observed on the MI355X, in units of the bar (atol + rtol |ref|): 0.055 (crowd-mixed), 0.046 (interleaved-c16),
0.03 and less on every other case -- the kernel's fp32 encoding sits a factor of 18 inside the bar.  The file's 49 tests run in 3.7 s.
"""
import functools

import numpy as np
import pytest
import torch

import targets_cases as cases
import targets_ref as ref
from gpu_util import dev

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-6  # tests/test_gpu_targets.py
EINVAL, EWORKSPACE = -1, -2
KEYS = ("G_cls", "M_cls", "G_reg", "M_reg", "matches")


def entry(c, low_quality, ws=None, with_matches=True, short=0, n_cls=None, A=None, null=()):
    """one v3d_assign_targets call -> (return code, dict of the outputs on the GPU); outputs pre-filled with 7 / NaN / -7"""
    from vision3d_amd import _lib as L
    lib = L.lib()
    shape = c["anchors"].shape[:2]
    n_cls = shape[0] if n_cls is None else n_cls
    A = shape[1] if A is None else A
    n = len(c["gt"])
    gt, cls, an = (dev(c["gt"].copy()) if n else None), (dev(c["gt_class"].copy()) if n else None), dev(c["anchors"].copy())
    out = dict(G_cls=torch.full(shape, 7, dtype=torch.int8, device="cuda"), M_cls=torch.full(shape, 7, dtype=torch.uint8, device="cuda"),
               G_reg=torch.full(shape + (7,), float("nan"), device="cuda"), M_reg=torch.full(shape, 7, dtype=torch.uint8, device="cuda"),
               matches=torch.full(shape, -7, dtype=torch.int64, device="cuda") if with_matches else None)
    if ws is None:
        nbytes = int(lib.v3d_assign_targets_workspace(n, max(n_cls, 1), max(A, 1))) - short
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    thresh = L.host_f32([float(t) for t in c["thresh"].reshape(-1)])
    p = {k: (0 if k in null else L.ptr(v)) for k, v in out.items()}
    code = lib.v3d_assign_targets(L.ptr(gt), L.ptr(cls), n, L.ptr(an), n_cls, A, thresh, int(low_quality), p["G_cls"], p["M_cls"], p["G_reg"],
                                  p["M_reg"], p["matches"], L.ptr(ws), ws.numel(), L.stream_ptr())
    torch.cuda.synchronize()
    return code, out


def untouched(out):
    return bool((out["G_cls"] == 7).all() and (out["M_cls"] == 7).all() and (out["M_reg"] == 7).all() and out["G_reg"].isnan().all()
                and (out["matches"] is None or (out["matches"] == -7).all()))


def same_bits(a, b):
    return all(a[k] is None or b[k] is None or torch.equal(a[k].view(torch.int32) if k == "G_reg" else a[k], b[k].view(torch.int32) if k == "G_reg" else b[k])
               for k in KEYS)


def check(what, got, w):
    """got: arrays in the reference's shapes.  -> the largest G_reg error at the positives in units of the bar"""
    np.testing.assert_array_equal(got["M_cls"].astype(np.int64), w["M_cls"].astype(np.int64), err_msg=f"{what}: M_cls")
    np.testing.assert_array_equal(got["G_cls"], w["G_cls"], err_msg=f"{what}: G_cls")
    np.testing.assert_array_equal(got["M_reg"].astype(np.int64), w["M_reg"].astype(np.int64), err_msg=f"{what}: M_reg")
    if got.get("matches") is not None:
        np.testing.assert_array_equal(got["matches"], w["matches"], err_msg=f"{what}: matches")
    pos = w["M_reg"]
    reg = got["G_reg"].astype(np.float64)
    assert (got["G_reg"][~pos].view(np.int32) == 0).all(), f"{what}: G_reg is +0.0 off the positives"
    bar = ATOL + RTOL * np.abs(w["G_reg"][pos])
    worst = float((np.abs(reg[pos] - w["G_reg"][pos]) / bar).max()) if pos.any() else 0.0
    print(f"{what}: {int(pos.sum())} positives, largest G_reg error {worst:.3f} of the bar")
    np.testing.assert_allclose(reg[pos], w["G_reg"][pos], rtol=RTOL, atol=ATOL, err_msg=f"{what}: G_reg")
    return worst


def to_numpy(out):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


@pytest.mark.parametrize("run", cases.RUNS, ids=cases.RUN_IDS)
def test_the_c_entry_on_every_case(run):
    name, low_quality = run
    c, w = cases.case(name), cases.reference(name, low_quality)
    code, out = entry(c, low_quality)
    assert code == 0
    check(cases.RUN_IDS[cases.RUNS.index(run)], to_numpy(out), w)
    code, again = entry(c, low_quality)
    assert code == 0 and same_bits(out, again), "two calls, the same bits"
    code, bare = entry(c, low_quality, with_matches=False)
    assert code == 0 and same_bits(out, bare), "without `matches`, the same outputs"


CFG_RUNS = [(r, i) for r, i in zip(cases.RUNS, cases.RUN_IDS) if "cfg" in cases.case(r[0])]


@pytest.mark.parametrize("run", [r for r, _ in CFG_RUNS], ids=[i for _, i in CFG_RUNS])
def test_the_assigner_on_the_grid_shaped_cases(run, monkeypatch):
    """ProposalTargetAssigner.forward on the crowds: the fused path (its torch statement is barred), direction targets included"""
    from vision3d_amd.core import ProposalTargetAssigner
    name, low_quality = run
    c, w = cases.case(name), cases.reference(name, low_quality)
    n_cls, A = c["anchors"].shape[:2]
    assigner = ProposalTargetAssigner(cases.make_cfg(*c["cfg"], low_quality=low_quality))
    shape = tuple(assigner.anchors.shape[:-1])
    assert shape == (n_cls, 2, 5, 7) and np.array_equal(assigner.anchors.cpu().numpy().reshape(n_cls, A, 7), c["anchors"])
    monkeypatch.setattr(assigner, "forward_torch", lambda item: pytest.fail("the torch statement ran: not the fused path"))
    item = assigner(dict(boxes=torch.from_numpy(c["gt"].copy()), class_idx=torch.from_numpy(c["gt_class"].copy()),
                         box_ignore=torch.zeros(len(c["gt"]), dtype=torch.bool)))
    assert item["G_cls"].dtype == torch.int8 and item["M_cls"].dtype == torch.bool and item["M_reg"].dtype == torch.bool
    assert item["G_cls"].shape == shape and item["G_reg"].shape == shape + (7,) and item["M_reg"].shape == shape + (1,)
    got = dict(G_cls=item["G_cls"].cpu().numpy().reshape(n_cls, A), M_cls=item["M_cls"].cpu().numpy().reshape(n_cls, A),
               M_reg=item["M_reg"].cpu().numpy().reshape(n_cls, A), G_reg=item["G_reg"].cpu().numpy().reshape(n_cls, A, 7))
    check(f"assigner {name}", got, w)
    assert item["G_dir"].dtype == torch.int8 and item["G_dir"].shape == shape
    want_dir = ref.direction(c["gt"], w["matches"], w["M_reg"])
    np.testing.assert_array_equal(item["G_dir"].cpu().numpy().reshape(n_cls, A), want_dir)
    if name == "crowd-mixed":
        assert set(want_dir[w["M_reg"]].tolist()) == {0, 1}, "both bits among the positives"


def test_a_workspace_reused_across_frames():
    """a frame of high maxima, then one of low maxima through the same workspace, the low-quality rule on: the second frame's
    positives exist only if its per-ground-truth maxima started from zero"""
    from vision3d_amd import _lib as L
    hi, lo = cases.case("stale-high"), cases.case("stale-low")
    nbytes = int(L.lib().v3d_assign_targets_workspace(len(hi["gt"]), 1, hi["anchors"].shape[1]))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    code, first = entry(hi, True, ws=ws)
    assert code == 0
    check("stale-high", to_numpy(first), cases.reference("stale-high", True))
    code, second = entry(lo, True, ws=ws)
    assert code == 0
    check("stale-low after stale-high", to_numpy(second), cases.reference("stale-low", True))
    code, fresh = entry(lo, True)
    assert code == 0 and same_bits(second, fresh)
    assert int(second["M_reg"].sum()) == 2


def test_refusals():
    c = cases.case("low_quality-clear")
    for kw, want_code in ((dict(n_cls=0), EINVAL), (dict(n_cls=17), EINVAL), (dict(n_cls=-1), EINVAL), (dict(A=0), EINVAL),
                          (dict(short=16), EWORKSPACE), (dict(null=("G_cls",)), EINVAL), (dict(null=("M_cls",)), EINVAL),
                          (dict(null=("G_reg",)), EINVAL), (dict(null=("M_reg",)), EINVAL)):
        code, out = entry(c, True, **kw)
        assert code == want_code, kw
        assert untouched(out), kw
    # 16 classes are served (interleaved-c16); 17 anchor sets of the same kind are refused before anything is read
    c16 = cases.case("interleaved-c16")
    code, out = entry(c16, True, n_cls=17)
    assert code == EINVAL and untouched(out)
    from vision3d_amd import _lib as L
    with pytest.raises(RuntimeError, match="assign_targets"):
        L.check(code, "assign_targets")


@functools.lru_cache(maxsize=None)
def _direction_want(n):
    c = cases.direction_case(n)
    out = ref.direction(c["gt"], c["matches"], c["m_reg"])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("n", cases.DIRECTION_SIZES)
def test_direction_targets_past_one_grid(n):
    from vision3d_amd import _lib as L
    c = cases.direction_case(n)
    gt, matches, m_reg = dev(c["gt"].copy()), dev(c["matches"].copy()), dev(c["m_reg"].astype(np.uint8))
    got = torch.full((n + 64,), 7, dtype=torch.int8, device="cuda")  # 64 guard elements behind the last
    for _ in range(2):
        code = L.lib().v3d_direction_targets(L.ptr(gt), cases.DIRECTION_N_GT, L.ptr(matches), L.ptr(m_reg), n, float(ref.direction_ref.OFFSET),
                                             L.ptr(got), L.stream_ptr())
        torch.cuda.synchronize()
        assert code == 0
        np.testing.assert_array_equal(got[:n].cpu().numpy(), _direction_want(n))
        assert (got[n:] == 7).all(), "nothing written behind the last element"
    if n == 255:  # no ground truth at all: every match is out of range
        none = torch.full((n,), 7, dtype=torch.int8, device="cuda")
        assert L.lib().v3d_direction_targets(0, 0, L.ptr(matches), L.ptr(m_reg), n, 0.0, L.ptr(none), L.stream_ptr()) == 0
        assert not none.any()
        assert L.lib().v3d_direction_targets(L.ptr(gt), 5, L.ptr(matches), L.ptr(m_reg), 0, 0.0, L.ptr(none), L.stream_ptr()) == EINVAL
        assert L.lib().v3d_direction_targets(0, 5, L.ptr(matches), L.ptr(m_reg), n, 0.0, L.ptr(none), L.stream_ptr()) == EINVAL

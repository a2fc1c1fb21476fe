"""v3d_sparse_bn_relu_fwd / _bwd (csrc/sparse_bn.hip) and v3d_dense_train_bn_finalize / _bn_relu_apply / _bn_relu_bwd (csrc/dense_train.hip)
against tests/bn_ref.py -- float64, every output within the bar derived there -- on the cases of tests/bn_cases.py.
tests/test_host_bn_ref.py shows on the host that the cases are what they are named for, that a float32 model of the kernels keeps half of
every chain bar, and which case notices which mistake.  Every call gets a workspace filled with 0xFF and outputs filled with NaN: nothing is
read before it is written, nothing is left unwritten.

Which run reaches what (ids of tests/bn_cases.py):
  unroll-c{16,64,256}-n*     one chunk at RL - 1 .. 4 RL + 1 rows: no unrolled trip, exactly one, one and a tail; both loops of both passes
  unroll-c{4,8}-n*           the widths whose unrolled statistics loop cannot run; n = 2, 3: biased against unbiased variance
  chunks-*, merge-*          G = 2, 3, 5 with a short last chunk; G one under, at and over the merge's Q = 1024 / C groups
  cap-c{4,16}-n*             512 chunks; from 131 073 rows on chunk 511 is empty (count 0, mean 0, M2 0) and must weigh nothing
  kind-*                     |mean| / std of 1e2 and 1e4 (the two-pass statistics), sorted rows (the between-chunk term), a constant
                             channel, an outlier row, gamma of both signs and 0, no ReLU, and the TIE kind: a quarter of the rows on the
                             ReLU's edge -- backward's mask must be the forward's on every element
  book-*, one_row            momentum 0.01 / 1 / 0 from non-trivial running values, NULL running pair, NULL counter; n = 1
  dense finalize             1 .. 1025 tiles through the 32-part column sums, count at and under 128 tiles, count = 1
  dense apply / backward     one block, one pixel over; 4096 blocks of the apply (65 536 pixels) and 512 of the reduction (8192) one over;
                             dx written over dy; the tie kind: the mask recovered from dx equals (y > 0) everywhere
The sparse backward is called with the GPU's own save_mean / save_invstd and judged against bn_backward on those values with
mask = (y_gpu > 0): no element is left out, the tie kind included.  Since dt_bn_bwd_* decide the mask with the forward's fmaf(x, sc, sh),
the same holds for the dense kernels.  Separately (y_gpu > 0) equals the float64 mask off the near-zero set.

Largest error observed on the MI355X, in units of the bar (the host model of tests/test_host_bn_ref.py gives the SAME figures to three
digits on every sparse output: it is the kernels' arithmetic):
  sparse   y 0.274 (kind-outlier-n513), save_mean 0.229, var_unbiased 0.209 (unroll-c256-n7), save_invstd 0.262 (unroll-c256-n5),
           dx 0.446 (kind-tie-n513), dgamma 0.246 (unroll-c256-n7), dbeta 0.220 (unroll-c256-n9); the running pair 0.617 / 0.640
           (unroll-c256-n8 / -n9): four roundings, a bar that is attained, not approached (test_host_bn_ref.worst)
  dense    dgamma 0.128 (bwd 16-1-iid), dbeta 0.016 (bwd 17-0-iid); y, dx and the four outputs of the finalize 0.98 - 1.00: their bar
           IS the one final rounding (half a bf16 ulp; the float32 cast of a float64 result)
Dense tie kind, mask recovered from dx against (y_gpu > 0): 53 528 of 524 189 decided elements differed at M = 4096 (105 216 of 1 050 560 at
M = 8209) while the backward kernels evaluated fmaf(xhat, gamma, beta) > 0; 0 since they evaluate the forward's expression.
|mean| / std = 100 through the finalize: bf16 pixels near 100 are multiples of 0.5, so the float32 tile sums of x and x^2 are EXACT and
E[x^2] - mean^2 in float64 loses nothing (3.5e-12 of the variance against the pixels' own float64 variance; 1.1e-7 after the float32
cast of invstd).  Stated, not asserted.  The file's 153 tests run in 9.9 s.
"""
import numpy as np
import pytest
import torch

import bn_cases as cases
import bn_ref as ref
from bn_cases import dense_bwd_fractions, dense_finalize_fractions, sparse_float64_mask_fractions, sparse_fractions
from gpu_util import dev

pytestmark = pytest.mark.gpu

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
F = np.float32


def _lib():
    from vision3d_amd import _lib as L
    return L, L.lib()


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def report(what, fr):
    print(f"{what}: in units of the bars: " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()))
    assert max(fr.values()) <= 1, (what, fr)


# ------------------------------------------------------------------------------------------------------------------ sparse
def sparse_forward(c, n=None, C=None, short=0, running="both", x=None):
    """one v3d_sparse_bn_relu_fwd call -> (code, dict of device tensors)"""
    L, lib = _lib()
    n, C = c["n"] if n is None else n, c["C"] if C is None else C
    t = dict(x=dev(c["x"].copy()) if x is None else x, gamma=dev(c["gamma"].copy()), beta=dev(c["beta"].copy()), y=nan(*c["x"].shape),
             save_mean=nan(c["C"]), save_invstd=nan(c["C"]), var_unbiased=nan(c["C"]),
             running_mean=dev(c["r_mean"].copy()) if c["r_mean"] is not None else None,
             running_var=dev(c["r_var"].copy()) if c["r_var"] is not None else None,
             nbt=torch.tensor(c["nbt"], dtype=torch.int64, device="cuda") if c["nbt"] is not None else None)
    ws = torch.full((int(lib.v3d_sparse_bn_workspace(max(n, 1), max(C, 1))) - short,), 0xFF, dtype=torch.uint8, device="cuda")
    rm = L.ptr(t["running_mean"]) if running in ("both", "mean") else 0
    rv = L.ptr(t["running_var"]) if running in ("both", "var") else 0
    code = lib.v3d_sparse_bn_relu_fwd(L.ptr(t["x"]), n, C, L.ptr(t["gamma"]), L.ptr(t["beta"]), c["eps"], c["relu"], L.ptr(t["y"]),
                                      L.ptr(t["save_mean"]), L.ptr(t["save_invstd"]), L.ptr(t["var_unbiased"]), rm, rv, c["momentum"],
                                      L.ptr(t["nbt"]), L.ptr(ws), ws.numel(), L.stream_ptr())
    torch.cuda.synchronize()
    return code, t


def sparse_backward(c, t, short=0, n=None, C=None):
    L, lib = _lib()
    n, C = c["n"] if n is None else n, c["C"] if C is None else C
    t.update(dy=dev(c["dy"].copy()), dx=nan(*c["x"].shape), dgamma=nan(c["C"]), dbeta=nan(c["C"]))
    ws = torch.full((int(lib.v3d_sparse_bn_workspace(max(n, 1), max(C, 1))) - short,), 0xFF, dtype=torch.uint8, device="cuda")
    code = lib.v3d_sparse_bn_relu_bwd(L.ptr(t["x"]), L.ptr(t["dy"]), n, C, L.ptr(t["gamma"]), L.ptr(t["beta"]), L.ptr(t["save_mean"]),
                                      L.ptr(t["save_invstd"]), c["relu"], L.ptr(t["dx"]), L.ptr(t["dgamma"]), L.ptr(t["dbeta"]), L.ptr(ws),
                                      ws.numel(), L.stream_ptr())
    torch.cuda.synchronize()
    return code


SPARSE_OUT = ("y", "save_mean", "save_invstd", "var_unbiased", "running_mean", "running_var", "dx", "dgamma", "dbeta")


@pytest.mark.parametrize("name", cases.SPARSE_IDS)
def test_the_sparse_entries_on_every_case(name):
    c = cases.sparse_case(name)
    code, t = sparse_forward(c)
    assert code == 0
    assert sparse_backward(c, t) == 0
    got = {k: t[k].cpu().numpy() for k in SPARSE_OUT if t[k] is not None}
    assert all(np.isfinite(v).all() for v in got.values()), "every output written"
    report(name, sparse_fractions(name, got))  # the backward: mask = (y_gpu > 0), no element left out
    if c["nbt"] is not None:
        assert int(t["nbt"]) == c["nbt"] + 1
    if c["kind"] != "tie":  # and against the float64 mask, the near-zero set left out; (y_gpu > 0) is the float64 mask off that set
        report(name + " (float64 mask)", sparse_float64_mask_fractions(name, got))
    if name == "one_row":
        assert np.array_equal(got["y"][0], np.maximum(c["beta"], 0)) and not got["dx"].any() and not got["var_unbiased"].any()
        assert np.array_equal(got["save_mean"], c["x"][0])
    # a second run, the same bits
    code, again = sparse_forward(c)
    assert code == 0 and sparse_backward(c, again) == 0
    for k in SPARSE_OUT:
        assert t[k] is None or torch.equal(bits(t[k]), bits(again[k])), f"{name}: {k} differs between two runs"


def test_sparse_refusals():
    c = cases.sparse_case("unroll-c16-n65")
    x_wide = torch.zeros((65, 512), device="cuda")
    for kw, want in ((dict(C=3), EUNSUPPORTED), (dict(C=12), EUNSUPPORTED), (dict(C=512, x=x_wide), EUNSUPPORTED), (dict(n=0), EUNSUPPORTED),
                     (dict(short=16), EWORKSPACE), (dict(running="mean"), EINVAL), (dict(running="var"), EINVAL)):
        code, t = sparse_forward(c, **kw)
        assert code == want, kw
        assert all(t[k].isnan().all() for k in ("y", "save_mean", "save_invstd", "var_unbiased")), kw
        assert torch.equal(t["running_mean"], dev(c["r_mean"].copy())) and int(t["nbt"]) == c["nbt"], kw
    code, t = sparse_forward(c)
    assert code == 0
    for kw, want in ((dict(C=3), EUNSUPPORTED), (dict(C=12), EUNSUPPORTED), (dict(n=0), EUNSUPPORTED), (dict(short=16), EWORKSPACE)):
        assert sparse_backward(c, t, **kw) == want, kw
        assert t["dx"].isnan().all() and t["dgamma"].isnan().all() and t["dbeta"].isnan().all(), kw
    L, lib = _lib()
    with pytest.raises(RuntimeError, match="sparse_bn"):
        L.check(EUNSUPPORTED, "sparse_bn")


# ------------------------------------------------------------------------------------------------------------------ dense
def bf16_dev(a):
    """bf16-valued float32 array -> bf16 tensor on the GPU"""
    return torch.from_numpy(cases.bf16_bits(a).view(np.int16)).cuda().view(torch.bfloat16)


def bf16_host(t):
    return cases.bf16_value(t.view(torch.int16).cpu().numpy().view(np.uint16))


@pytest.mark.parametrize("run", cases.FINALIZE_RUNS, ids=cases.run_id)
def test_dense_finalize(run):
    L, lib = _lib()
    c = cases.finalize_case(*run)
    t = dict(mean=nan(128), invstd=nan(128), running_mean=dev(c["r_mean"].copy()), running_var=dev(c["r_var"].copy()))
    nbt = torch.tensor(c["nbt"], dtype=torch.int64, device="cuda")
    part = dev(c["partial"].copy())
    args = (L.ptr(part), c["tiles"], c["count"], c["eps"], c["momentum"], L.ptr(t["mean"]), L.ptr(t["invstd"]))
    assert lib.v3d_dense_train_bn_finalize(*args, L.ptr(t["running_mean"]), L.ptr(t["running_var"]), L.ptr(nbt), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in t.items()}
    report("finalize " + cases.run_id(run), dense_finalize_fractions(c, got))
    assert int(nbt) == c["nbt"] + 1
    if run[1] == "offset" and run[2] == "full":  # stated, not asserted: what the fp32 partials have lost before the kernel sees them
        fin = ref.dense_finalize(c["partial"], c["count"], c["eps"])
        var_gpu = 1.0 / got["invstd"].astype(np.float64) ** 2 - float(F(c["eps"]))
        print(f"finalize {cases.run_id(run)}: |mean| / std = 100: variance of the GPU against the pixels' float64 variance, largest relative "
              f"difference {(np.abs(var_gpu - c['true_var']) / c['true_var']).max():.3e} (float64 on the same partials: "
              f"{(np.abs(fin['var'] - c['true_var']) / c['true_var']).max():.3e})")
    # without the running pair: the same mean / invstd, nothing else touched
    bare = dict(mean=nan(128), invstd=nan(128))
    assert lib.v3d_dense_train_bn_finalize(L.ptr(part), c["tiles"], c["count"], c["eps"], c["momentum"], L.ptr(bare["mean"]),
                                           L.ptr(bare["invstd"]), 0, 0, 0, L.stream_ptr()) == 0
    assert torch.equal(bits(bare["mean"]), bits(t["mean"])) and torch.equal(bits(bare["invstd"]), bits(t["invstd"]))
    if run == cases.FINALIZE_RUNS[0]:
        assert lib.v3d_dense_train_bn_finalize(*args, L.ptr(t["running_mean"]), 0, 0, L.stream_ptr()) == EINVAL
        assert lib.v3d_dense_train_bn_finalize(L.ptr(part), 0, 1, c["eps"], 0.1, L.ptr(t["mean"]), L.ptr(t["invstd"]), 0, 0, 0, L.stream_ptr()) == EINVAL
        assert lib.v3d_dense_train_bn_finalize(L.ptr(part), 1, 0, c["eps"], 0.1, L.ptr(t["mean"]), L.ptr(t["invstd"]), 0, 0, 0, L.stream_ptr()) == EINVAL


def dense_apply(c, x=None):
    L, lib = _lib()
    x = bf16_dev(c["x"]) if x is None else x
    p = {k: dev(c[k].copy()) for k in ("mean", "invstd", "gamma", "beta")}
    y = torch.full((c["M"] + 16, 128), float("nan"), dtype=torch.bfloat16, device="cuda")  # 16 guard pixels behind the last
    assert lib.v3d_dense_train_bn_relu_apply(L.ptr(x), c["M"], L.ptr(p["mean"]), L.ptr(p["invstd"]), L.ptr(p["gamma"]), L.ptr(p["beta"]),
                                             c["relu"], L.ptr(y), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert y[c["M"]:].isnan().all(), "nothing written behind the last pixel"
    return x, p, y[:c["M"]]


def dense_backward(c, x, p, alias=False):
    L, lib = _lib()
    dy = torch.cat([bf16_dev(c["dy"]), torch.full((16, 128), float("nan"), dtype=torch.bfloat16, device="cuda")])
    dx = dy if alias else torch.full_like(dy, float("nan"))
    dgamma, dbeta = nan(128), nan(128)
    ws = torch.full((int(lib.v3d_dense_train_bn_bwd_workspace()),), 0xFF, dtype=torch.uint8, device="cuda")
    assert lib.v3d_dense_train_bn_relu_bwd(L.ptr(x), L.ptr(dy), c["M"], L.ptr(p["mean"]), L.ptr(p["invstd"]), L.ptr(p["gamma"]),
                                           L.ptr(p["beta"]), c["relu"], L.ptr(dx), L.ptr(dgamma), L.ptr(dbeta), L.ptr(ws), ws.numel(),
                                           L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert dx[c["M"]:].isnan().all(), "nothing written behind the last pixel"
    return dict(dx=dx[:c["M"]], dgamma=dgamma, dbeta=dbeta)


@pytest.mark.parametrize("run", cases.APPLY_RUNS, ids=cases.run_id)
def test_dense_apply(run):
    c = cases.apply_case(*run)
    _, _, y = dense_apply(c)
    got = bf16_host(y)
    assert np.isfinite(got).all()
    report("apply " + cases.run_id(run), dict(y=ref.in_bars(got, c["y"], c["bar_y"])))
    if c["relu"]:
        near = ref.near_zero(c["v"], c["bar_v"])
        assert np.array_equal((got > 0)[~near], (c["v"] > 0)[~near])
    _, _, again = dense_apply(c)
    assert torch.equal(bits(y), bits(again))


def recovered_mask(c, got, y):
    """which of its two candidate values each dx is: gamma invstd (dy - k0 - xhat k1) or gamma invstd (-k0 - xhat k1), from the GPU's own
    sums; decided where the candidates lie more than 8 bars of dx apart -> (mask, decided)"""
    g, is_, M = c["gamma"].astype(np.float64), c["invstd"].astype(np.float64), c["M"]
    xhat = (c["x"].astype(np.float64) - c["mean"]) * is_
    rest = -got["dbeta"].astype(np.float64) / M - xhat * got["dgamma"].astype(np.float64) / M
    passed, stopped = g * is_ * (c["dy"] + rest), g * is_ * rest
    bw = ref.bn_backward(c["x"], c["dy"], c["mean"], c["invstd"], c["gamma"], c["beta"], 1, mask=y > 0)
    bar = ref.backward_bars(bw, c["gamma"], c["invstd"], ref.dense_geometry(M)["k_bwd"], bf16=True)["dx"]
    decided = np.abs(passed - stopped) > 8 * np.maximum(bar, ref.bf16_half_ulp(np.maximum(np.abs(passed), np.abs(stopped))))
    dx = got["dx"].astype(np.float64)
    return np.abs(dx - passed) < np.abs(dx - stopped), decided


@pytest.mark.parametrize("run", cases.BWD_RUNS, ids=cases.run_id)
def test_dense_backward(run):
    c = cases.bwd_case(*run)
    x, p, y = dense_apply(c)
    y = bf16_host(y)
    out = dense_backward(c, x, p)
    got = dict(dx=bf16_host(out["dx"]), dgamma=out["dgamma"].cpu().numpy(), dbeta=out["dbeta"].cpu().numpy())
    assert all(np.isfinite(v).all() for v in got.values())
    if c["relu"]:  # the mask the backward used, read off dx
        mask, decided = recovered_mask(c, got, y)
        differ = decided & (mask != (y > 0))
        print(f"bwd {cases.run_id(run)}: the mask recovered from dx differs from y > 0 on {int(differ.sum())} of {int(decided.sum())} decided elements"
              f" ({int((c['x'] == c['x'][0]).all(1).sum()) * 128} on tied rows)")
        assert decided.mean() > 0.5
        assert not differ.any(), f"{int(differ.sum())} elements take the gradient against the stored output"
    report("bwd " + cases.run_id(run), dense_bwd_fractions(c, got, y))  # mask = (y_gpu > 0): nothing left out
    if c["kind"] != "tie":
        near, geo = c["near"], ref.dense_geometry(c["M"])
        bw = ref.bn_backward(c["x"], c["dy"], c["mean"], c["invstd"], c["gamma"], c["beta"], c["relu"])
        bb = ref.backward_bars(bw, c["gamma"], c["invstd"], geo["k_bwd"], bf16=True, near=near, dy=c["dy"])
        report("bwd " + cases.run_id(run) + " (float64 mask)",
               dict(dx=ref.in_bars(got["dx"][~near], bw["dx"][~near], bb["dx"][~near]), dgamma=ref.in_bars(got["dgamma"], bw["dgamma"], bb["dgamma"]),
                    dbeta=ref.in_bars(got["dbeta"], bw["dbeta"], bb["dbeta"])))
    # dx written over dy: the same bits
    over = dense_backward(c, x, p, alias=True)
    for k in ("dx", "dgamma", "dbeta"):
        assert torch.equal(bits(out[k]), bits(over[k])), f"{k}: dx aliasing dy changes the result"


def test_dense_refusals():
    L, lib = _lib()
    c = cases.bwd_case(16, 1, "iid")
    x, p, _ = dense_apply(c)
    dy, dx, dg, db = bf16_dev(c["dy"]), torch.full((16, 128), float("nan"), dtype=torch.bfloat16, device="cuda"), nan(128), nan(128)
    ws = torch.full((int(lib.v3d_dense_train_bn_bwd_workspace()),), 0xFF, dtype=torch.uint8, device="cuda")
    tail = (L.ptr(p["mean"]), L.ptr(p["invstd"]), L.ptr(p["gamma"]), L.ptr(p["beta"]), 1, L.ptr(dx), L.ptr(dg), L.ptr(db), L.ptr(ws))
    assert lib.v3d_dense_train_bn_relu_bwd(L.ptr(x), L.ptr(dy), 16, *tail, ws.numel() - 16, L.stream_ptr()) == EWORKSPACE
    assert lib.v3d_dense_train_bn_relu_bwd(L.ptr(x), L.ptr(dy), 0, *tail, ws.numel(), L.stream_ptr()) == EINVAL
    assert lib.v3d_dense_train_bn_relu_apply(L.ptr(x), 0, L.ptr(p["mean"]), L.ptr(p["invstd"]), L.ptr(p["gamma"]), L.ptr(p["beta"]), 1, L.ptr(dx),
                                             L.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert dx.isnan().all() and dg.isnan().all() and db.isnan().all()

"""v3d_sparse_conv_bwd_weight (csrc/spconv.hip: spconv_bwd_weight_tiles + spconv_bwd_weight_reduce_kernel) and the data gradient of
SparseConvFunction.backward (spconv/functional.py) against tests/spconv_grad_ref.py -- float64, written from the forward rulebook alone --
on the cases of tests/spconv_grad_cases.py.  Integer-valued cases must EQUAL the reference; real-valued weight gradients keep the bar
derived in spconv_grad_ref, real-valued data gradients gpu_util.assert_features_close (bf16x3 floor 1e-4).  tests/test_host_spconv_grad_ref.py
shows on the host that the reference is torch's float64 conv3d autograd, that a float32 model of the kernel is exact / keeps half the bar,
and which case notices which mistake.  Every raw call gets a workspace of 0xFF bytes with a guard behind it, a NaN dW with GUARD floats on
both sides, and its inputs are compared with their copies afterwards.

Which dW case reaches what:
  live-{1 .. 257}            the tail consume alone; a whole batch of 16; 17 = a batch and a leftover moved; the 64-row wave sub-slab one
                             under, at and over; the 256-row slab one under, at and over (257: a second slab with ONE row)
  live-{16383, 16384, 16385} 64 slabs of 256 rows, the last a row short, full; 33 slabs of 512 (sub-slabs of 128: two table batches, the queue
                             carries leftovers over) the last with one row
  live-{32768, 32769}        64 slabs of 512; 43 slabs of 768 (three batches per wave)
  dens-*                     all five densities side by side; `none`: zeros written; q79: the queue at 79 (n >= 16 385)
  single-*                   one live pair in the whole column: row 0, the last row of slab 0, row n - 1
  src-one-*, src-3n-*        every pair reads X[0]; sources spread over 3 n rows
  chan-*                     all nine TI x TJ instantiations; ragged channel counts (masks on ci, co; 80 x 48 masks inside the second of
                             two groups); 64 x 128, 128 x 16 (two groups on blockIdx.z), 128 x 128 (four); k1-*, k27-*: gridDim.y = 1, 27
  cap-*, over-256            cap > n with live-looking rows behind n: bit-equal to the cap == n run; n = 0: zeros over the NaN fill;
                             *n_ptr = cap + 44: bit-equal to n = cap
Which data-gradient run takes which route (the transposed layer is Cout -> Cin; cases.route, checked against the library on the host):
  packed (bf16x3)   16->16, 16->32, 32->32, 32->64, 64->64, 32->16, 64->32, 128->128        scalar   4->16, 4->32 (Cin % 16), 64->128,
  wave (fp32 MFMA)  16->4 (module.algo = 1)                                                          16->8, 8->16, 48->16 (no MFMA kernel
                                                                                                     for the swapped pair: these RAISED before)
  every submanifold kernel and every strided geometry at 16->16; the scalar kernel's grid-stride loop on a synthetic K = 1 table of 65 537
  rows (32 outputs beyond 8192 x 256 threads: the last row's gradient); 20 000 rows 3x3x3 64->64: the packed route above its ring kernel.

Largest error observed on the MI355X, in units of the bar:
  dW, raw calls    0.382 (real-256, over-256: the one_per_64 column, 4 pairs under a chain bound of 6), 0.232 (real-257, cap-257-4096), 0.079
                   (real-257-128x128), 0.047 (real-257-17x33), 0.031 (real-16385, cap-16385-65536), 0.017 (real-32769), 0.004 (real-16385-64x128).
                   The host model of tests/test_host_spconv_grad_ref.py gives 0.382 / 0.232 / 0.076 / 0.049 / 0.027 / 0.011 / 0.003: the same
                   figures where a short column decides, close to them where the order inside an MFMA (not promised, not modelled) does.
  dW, module path  at most 0.064 (submanifold 64->64 and 64->128 on 429 rows); 0.006 at 20 000 rows
  dX               worst element, in units of assert_features_close's elementwise bar: packed 0.343 (strided 32->16), 0.248 / 0.183 (64->64),
                   0.232 (20 000 rows); scalar 0.014; wave 0.004.  Max norm: at most 5.6e-6 of max|dX| against the bar of 1e-4.
Every integer case equals float64; nothing in spconv_bwd_weight_* had to change.  The file's 115 tests run in 4.6 s.
"""
import functools

import numpy as np
import pytest
import torch

import geometry_cases as gc
import geometry_ref as gref
import spconv_grad_cases as cases
import spconv_grad_ref as ref
from gpu_util import assert_features_close, dev

pytestmark = pytest.mark.gpu

EINVAL, EWORKSPACE = -1, -2
GUARD = cases.GUARD
WS_GUARD = 4096  # bytes behind the workspace


def _lib():
    from vision3d_amd import _lib as L
    return L, L.lib()


def bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ dW, raw calls
def raw_dw(c, short=0, null=None, **over):
    """one v3d_sparse_conv_bwd_weight call on the case -> (code, dW (K, Cin, Cout) device tensor or None where the guards or the inputs
    were touched -- asserted, dict of the buffers)"""
    L, lib = _lib()
    K, cin, cout, cap = (over.get(k, c[k]) for k in ("K", "cin", "cout", "cap"))
    elems = c["K"] * c["cin"] * c["cout"]
    t = dict(X=dev(np.array(c["X"])), dY=dev(np.array(c["dY"])), nbr=dev(np.array(c["nbr"])),
             n_out=torch.tensor([c["n_ptr"]], dtype=torch.int32, device="cuda"),
             dW=torch.full((GUARD + elems + GUARD,), float("nan"), device="cuda"))
    nbytes = int(lib.v3d_sparse_conv_bwd_weight_workspace(c["K"], c["cin"], c["cout"]))
    t["workspace"] = torch.full((nbytes + WS_GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    copies = {k: t[k].clone() for k in ("X", "dY", "nbr", "n_out")}
    p = {k: (0 if k == null else L.ptr(v)) for k, v in t.items()}
    if null != "dW":
        p["dW"] += 4 * GUARD
    code = lib.v3d_sparse_conv_bwd_weight(p["X"], p["dY"], p["nbr"], p["n_out"], cap, K, cin, cout, p["dW"], p["workspace"], nbytes - short,
                                          L.stream_ptr())
    torch.cuda.synchronize()
    for k, v in copies.items():
        assert torch.equal(t[k], v), f"{c['name']}: input {k} was written"
    assert t["dW"][:GUARD].isnan().all() and t["dW"][GUARD + elems:].isnan().all(), f"{c['name']}: written outside dW"
    assert (t["workspace"][nbytes:] == 0xFF).all(), f"{c['name']}: written behind the workspace"
    return code, t["dW"][GUARD:GUARD + elems].view(c["K"], c["cin"], c["cout"]), t


@pytest.mark.parametrize("name", cases.DW_IDS)
def test_the_weight_gradient_on_every_case(name):
    c = cases.dw_case(name)
    want, bar = cases.dw_reference(name)
    code, dW, _ = raw_dw(c)
    assert code == 0
    got = dW.cpu().numpy()
    assert np.isfinite(got).all(), "every element written"
    if c["kind"] == "int":
        assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} of {got.size} elements differ from float64"
    else:
        fr = ref.in_bars(got, want, bar)
        print(f"{name}: dW at {fr:.3f} of the bar (chain {ref.dw_chain(c['nbr'], c['n']).tolist()})")
        assert fr <= 1, (name, fr)
    for k, d in enumerate(c["cols"]):
        if d == "none" or c["n"] == 0:
            assert not got[k].any(), "a column without a live pair is exactly 0"
    code, again, _ = raw_dw(c)  # a repeated call: the same bits
    assert code == 0 and torch.equal(bits(dW), bits(again)), f"{name}: two runs differ"
    if name in cases.SAME_BITS:  # the slab split depends on n only
        code, base, _ = raw_dw(cases.dw_case(cases.SAME_BITS[name]))
        assert code == 0 and torch.equal(bits(dW), bits(base)), f"{name}: differs from the run with cap == n"


def test_the_weight_gradient_return_codes():
    c = cases.dw_case("live-257")
    for kw in [dict(null=k) for k in ("X", "dY", "nbr", "n_out", "dW", "workspace")] + \
              [dict(cap=0), dict(cap=-1), dict(K=0), dict(K=65536), dict(cin=0), dict(cout=0)]:
        code, dW, t = raw_dw(c, **kw)
        assert code == EINVAL, kw
        assert dW.isnan().all() and (t["workspace"] == 0xFF).all(), (kw, "nothing is written")
    code, dW, t = raw_dw(c, short=1)
    assert code == EWORKSPACE and dW.isnan().all() and (t["workspace"] == 0xFF).all()
    code, dW, _ = raw_dw(c)
    assert code == 0 and not dW.isnan().any()


def test_the_wrapper_and_the_raw_call_agree_on_no_rows():
    """sparse_conv_bwd_weight short-circuits n = 0 in Python; a training plan calls the C function (cap-0-256 above): both give zeros"""
    from vision3d_amd.spconv.functional import sparse_conv_bwd_weight
    from vision3d_amd.spconv.tensor import Rulebook
    c = cases.dw_case("cap-0-256")
    rb = Rulebook(dev(np.array(c["nbr"])), c["cap"], 0, torch.zeros(1, dtype=torch.int32, device="cuda"), None, None)
    dw = sparse_conv_bwd_weight(dev(np.array(c["X"])), dev(np.array(c["dY"])), rb, c["K"], c["cin"], c["cout"])
    assert dw.shape == (c["K"], c["cin"], c["cout"]) and not dw.any()


# ------------------------------------------------------------------------------------------------------------------ dX, through autograd
@functools.lru_cache(maxsize=None)
def subm_table(case, ks):
    c = gc.build(case)
    return gref.subm_rulebook(c["coords"], len(c["coords"]), c["shape"], list(ks))


@functools.lru_cache(maxsize=None)
def strided_table(case, geom):
    c = gc.build(case)
    co, nbr, _, overflow = gref.sparse_rulebook(c["coords"], len(c["coords"]), c["shape"], *gc.STRIDED_GEOMETRIES[geom])
    assert not overflow
    return co, nbr


def forward64(nbr, n, X, W):
    out = np.zeros((n, W.shape[2]))
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k, :n] >= 0)[0]
        out[o] += X[nbr[k, o]].astype(np.float64) @ W[k].astype(np.float64)
    return out


def layer(c, nbr, n_out, cin, cout, kind, what, subm, ks, st=1, pd=0, algo=0, wide=False, out_coords=None):
    """one module forward + backward on the sites of c against the reference on the table nbr -> the largest fraction of the dW bar (real)"""
    from vision3d_amd import spconv
    n_in, K = len(c["coords"]), nbr.shape[0]
    rng = cases._rng(what)
    X, W, dY = cases.values(kind, rng, (n_in, cin)), cases.values(kind, rng, (K, cin, cout)), cases.values(kind, rng, (n_out, cout))
    conv = (spconv.SubMConv3d(cin, cout, ks, bias=False) if subm else spconv.SparseConv3d(cin, cout, ks, st, padding=pd, bias=False)).cuda()
    conv.algo = algo
    with torch.no_grad():
        conv.weight.copy_(dev(W).view(*conv.weight.shape))
    x = spconv.SparseConvTensor(dev(X).requires_grad_(True), dev(np.array(c["coords"]), torch.int32), c["shape"], c["batch"])
    out = conv(x)
    assert out.features.shape == (n_out, cout)
    if out_coords is not None:
        assert np.array_equal(out.indices.cpu().numpy(), out_coords)
    g = dev(dY)
    if wide:  # a gradient that is a strided view: every other column of a (n, 2 Cout) buffer
        buf = torch.full((n_out, 2 * cout), float("nan"), device="cuda")
        buf[:, ::2] = g
        g = buf[:, ::2]
        assert not g.is_contiguous()
    out.features.backward(g)
    torch.cuda.synchronize()
    y, gx, gw = out.features.detach().cpu().numpy(), x.features.grad.cpu().numpy(), conv.weight.grad.cpu().numpy().reshape(K, cin, cout)
    want_y, want_x, want_w = forward64(nbr, n_out, X, W), ref.dx(nbr, n_out, n_in, dY, W), ref.dw(nbr, n_out, X, dY)
    fed = ref.fed_rows(nbr, n_out, n_in)
    assert not gx[~fed].any(), f"{what}: an input row that feeds no output has a gradient"
    if kind == "int":
        assert np.array_equal(y, want_y), f"{what}: forward"
        assert np.array_equal(gx, want_x), f"{what}: dX, {int((gx != want_x).any(1).sum())} of {n_in} rows differ from float64"
        assert np.array_equal(gw, want_w), f"{what}: dW"
        return 0.0, fed
    assert_features_close(y, want_y, f"{what}: forward")
    assert_features_close(gx, want_x, f"{what}: dX")
    fr = ref.in_bars(gw, want_w, ref.dw_bar(nbr, n_out, X, dY))
    err = np.abs(gx - want_x)
    print(f"{what} [{cases.route(cin, cout)}]: dW at {fr:.3f} of the bar; dX max error {err.max() / np.abs(want_x).max():.3e} of max|dX| "
          f"(bar 1e-4), worst element at {(err / (1e-4 * np.abs(want_x) + 1e-4 * np.sqrt((want_x[want_x != 0] ** 2).mean()))).max():.3f} of its bar")
    assert fr <= 1, (what, fr)
    return fr, fed


def subm_layer(cin, cout, kind, ks=(3, 3, 3), case="few_hundred", **kw):
    c = gc.build(case)
    n = len(c["coords"])
    return layer(c, subm_table(case, tuple(ks)), n, cin, cout, kind, f"subm k{ks[0]}{ks[1]}{ks[2]} {cin}->{cout} {kind}", True, list(ks), **kw)


def strided_layer(cin, cout, kind, geom="k3s2p1", case="odd_grid", **kw):
    c = gc.build(case)
    ks, st, pd = gc.STRIDED_GEOMETRIES[geom]
    co, nbr = strided_table(case, geom)
    return layer(c, nbr, len(co), cin, cout, kind, f"strided {geom} {cin}->{cout} {kind}", False, ks, st, pd, out_coords=co, **kw)


@pytest.mark.parametrize("ks", gc.SUBM_KERNELS, ids=lambda ks: "k%d%d%d" % tuple(ks))
def test_every_submanifold_kernel_reverses_its_offsets(ks):
    assert set(gc.build("few_hundred")["coords"][:, 0]) == {0, 1}, "two frames"
    subm_layer(16, 16, "int", ks)


@pytest.mark.parametrize("geom", list(gc.STRIDED_GEOMETRIES))
def test_every_strided_geometry_through_the_transposed_table(geom):
    _, fed = strided_layer(16, 16, "int", geom)
    if geom in ("k1s2p0", "k2s2p0", "k3s3p0"):  # the geometries that must leave rows unfed (test_host_spconv_grad_ref): zero rows, checked
        assert (~fed).sum() >= 100


@pytest.mark.parametrize("cin,cout", cases.FORWARD_PAIRS + cases.ALGO1_LAYERS, ids=lambda v: str(v))
def test_every_layer_whose_forward_runs_trains(cin, cout):
    """route: see cases.route and the module docstring; the ALGO1_LAYERS run their forward on the scalar kernel (module.algo = 1)"""
    algo = 1 if (cin, cout) in cases.ALGO1_LAYERS else 0
    subm_layer(cin, cout, "int", algo=algo)
    strided_layer(cin, cout, "int", algo=algo)


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (16, 4), (32, 16), (48, 16)], ids=lambda v: str(v))
def test_real_values_on_every_route(cin, cout):
    algo = 1 if (cin, cout) in cases.ALGO1_LAYERS else 0
    subm_layer(cin, cout, "real", algo=algo)
    strided_layer(cin, cout, "real", algo=algo)


def test_real_values_above_the_ring_kernel():
    """20 000 live rows, 3x3x3, 64 -> 64: forward and data gradient on the packed route's large-row kernel"""
    s = cases.large_sites()
    n = len(s["coords"])
    nbr = gref.subm_rulebook(s["coords"], n, s["shape"], [3, 3, 3])
    layer(s, nbr, n, 64, 64, "real", "subm k333 64->64 real, 20 000 rows", True, [3, 3, 3])


def test_a_strided_view_as_grad_out():
    subm_layer(16, 16, "int", wide=True)
    strided_layer(32, 16, "int", wide=True)


def test_a_single_input_row():
    c = dict(coords=np.array([[0, 2, 3, 4]], np.int32), shape=[5, 11, 13], batch=1)
    nbr = gref.subm_rulebook(c["coords"], 1, c["shape"], [3, 3, 3])
    assert (nbr >= 0).sum() == 1 and nbr[13, 0] == 0
    layer(c, nbr, 1, 16, 16, "int", "subm one row", True, [3, 3, 3])
    co, nbr, _, _ = gref.sparse_rulebook(c["coords"], 1, c["shape"], *gc.STRIDED_GEOMETRIES["k3s2p1"])
    assert len(co) == (nbr >= 0).sum() == 2  # 2 o = c + 1 - k: k = 1 in z and x, k = 0 or 2 in y
    layer(c, nbr, len(co), 16, 32, "int", "strided one row", False, *gc.STRIDED_GEOMETRIES["k3s2p1"], out_coords=co)


@pytest.mark.parametrize("need", ["features", "weight", "both"])
@pytest.mark.parametrize("subm", [True, False], ids=["subm", "strided"])
def test_needs_input_grad_combinations(need, subm):
    from vision3d_amd import spconv
    from vision3d_amd.spconv.conv import build_sparse_rulebook, build_subm_rulebook
    from vision3d_amd.spconv.functional import SparseConvFunction
    case, geom = ("few_hundred", None) if subm else ("odd_grid", "k3s2p011")
    c = gc.build(case)
    n_in = len(c["coords"])
    x = spconv.SparseConvTensor(torch.zeros((n_in, 1), device="cuda"), dev(np.array(c["coords"]), torch.int32), c["shape"], c["batch"])
    if subm:
        rb, nbr = build_subm_rulebook(x, [3, 3, 3]), subm_table(case, (3, 3, 3))
    else:
        rb, nbr = build_sparse_rulebook(x, *gc.STRIDED_GEOMETRIES[geom]), strided_table(case, geom)[1]
    assert np.array_equal(rb.nbr.cpu().numpy()[:, :rb.n], nbr)
    rng = cases._rng("needs " + need)
    X, W, dY = cases.values("int", rng, (n_in, 16)), cases.values("int", rng, (27, 16, 32)), cases.values("int", rng, (rb.n, 32))
    f = dev(X).requires_grad_(need != "weight")
    w = dev(W).view(3, 3, 3, 16, 32).requires_grad_(need != "features")
    SparseConvFunction.apply(f, w, rb, subm, 0).backward(dev(dY))
    assert (f.grad is None) == (need == "weight") and (w.grad is None) == (need == "features")
    if f.grad is not None:
        assert np.array_equal(f.grad.cpu().numpy(), ref.dx(nbr, rb.n, n_in, dY, W))
    if w.grad is not None:
        assert np.array_equal(w.grad.cpu().numpy().reshape(27, 16, 32), ref.dw(nbr, rb.n, X, dY))


def test_the_scalar_kernels_grid_stride_loop():
    """a 32 -> 8 layer on the scalar kernel (algo 1): its data gradient is the 8 -> 32 scalar launch (no MFMA kernel for that pair; 4 -> 32
    has one, which the data gradient would take) over 65 537 x 32 outputs, 32 more than its 8192 x 256 threads -- the last input row's
    gradient is written by the loop's second trip"""
    assert cases.route(cases.GRID_STRIDE["cin"], cases.GRID_STRIDE["cout"]) == "scalar"
    from vision3d_amd.spconv.functional import SparseConvFunction
    from vision3d_amd.spconv.tensor import Rulebook
    rows, cin, cout = (cases.GRID_STRIDE[k] for k in ("rows", "cin", "cout"))
    nbr = cases.grid_stride_table()
    rng = cases._rng("grid_stride values")
    X, W, dY = cases.values("int", rng, (rows, cin)), cases.values("int", rng, (1, cin, cout)), cases.values("int", rng, (rows, cout))
    rb = Rulebook(dev(nbr), rows, rows, torch.tensor([rows], dtype=torch.int32, device="cuda"), None, None)
    f, w = dev(X).requires_grad_(True), dev(W).requires_grad_(True)
    out = SparseConvFunction.apply(f, w, rb, False, 1)
    out.backward(dev(dY))
    assert np.array_equal(out.detach().cpu().numpy(), forward64(nbr, rows, X, W))
    want = ref.dx(nbr, rows, rows, dY, W)
    got = f.grad.cpu().numpy()
    assert want[rows - 1].any(), "the row of the second trip has a gradient"
    assert np.array_equal(got[rows - 1], want[rows - 1]), "the loop's second trip"
    assert np.array_equal(got, want)
    assert np.array_equal(w.grad.cpu().numpy(), ref.dw(nbr, rows, X, dY))

"""Host: tests/spconv_grad_ref.py against torch's float64 autograd of the dense F.conv3d, the cases of tests/spconv_grad_cases.py against
what they are named for, and a plain numpy float32 MODEL of v3d_sparse_conv_bwd_weight in the kernel's own order.  What this file
establishes for tests/test_gpu_spconv_grad_edges.py:
  * ref.dw / ref.dx ARE the gradients of the dense cross-correlation (the statement tests/test_gpu_backward.py uses), on every
    submanifold kernel and every strided geometry of tests/geometry_cases.py;
  * the integer cases stay under 2^24 in every partial sum; the strided geometries that must leave input rows unfed do;
  * each dW case has the slab geometry and the queue length it is named for;
  * the model (slabs from bw_rows_per_block, four sub-slabs, the 128-entry queue consumed 16 pairs at a time with its leftovers moved
    to the front, wave order, the store through the channel masks in dispatch order, slab order) is EXACT on every integer case and
    stays within HALF of the bar on every real one;
  * each of these mistakes, made in the model, is noticed by the named cases and not by their neighbours (no mutated library is built):
      last partial 64-row batch dropped    live-1, -15, -17, -63, -65, -257       (not live-64, live-256)
      the < 16 tail not consumed           live-15, live-17, dens-257             (the `all` column of live-16 alone would not)
      leftovers not moved to the front     live-17, live-16385                    (not live-15, live-16: nothing is left over)
      reduce takes its slab count from cap cap-257-4096, cap-16385-65536          (not over-256, nor any cap == n case)
      ci >= Cin unmasked (load and store)  chan-*-5x20, -17x33, -80x48, -1x1      (not the multiples of 16)
      ci / co swapped in the store         live-257, chan-257-16x32
    and, on a float64 statement of SparseConvFunction.backward's gather form (own table + reversed offsets; transposed table):
      no offset reversal, submanifold      every kernel but [1, 1, 1]
      reversal on a strided layer          every geometry but k1s2p0
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import geometry_cases as gc
import geometry_ref as gref
import spconv_grad_cases as cases
import spconv_grad_ref as ref

F = np.float32
HALF = 0.5
EXACT = 2 ** 24


# ------------------------------------------------------------------------------------------------------------------ the dW model
def tiles(c):
    return 4 if c > 32 else (2 if c > 16 else 1)


def consumed(nk, wlo, whi, mut):
    """the (source, output row) pairs one wave hands to its MFMAs, in order: 64 table entries at a time, live ones appended to the queue,
    whole batches of 16 consumed, the leftovers moved to the front, the tail at the end"""
    out, q = [], np.empty((0, 2), np.int64)
    peak = 0
    for o0 in range(wlo, whi, 64):
        hi = min(o0 + 64, whi)
        if mut == "drop_partial_batch" and hi - o0 < 64:
            continue
        rows = np.arange(o0, hi)
        src = nk[rows]
        q = np.concatenate([q, np.stack([src[src >= 0], rows[src >= 0]], 1)])
        peak = max(peak, len(q))
        g = len(q) // ref.BW_BATCH * ref.BW_BATCH
        out.append(q[:g])
        if g:
            q = q[:len(q) - g] if mut == "no_move" else q[g:]
    if len(q) and mut != "no_tail":
        out.append(q)
    assert peak <= ref.BW_Q
    return np.concatenate(out) if out else q


def dw_model(c, mut=None):
    """v3d_sparse_conv_bwd_weight in numpy float32 -> dW (K, Cin, Cout) float32.  The workspace starts as 0xFF bytes (NaN)."""
    nbr, K, cap, cin, cout = c["nbr"], c["K"], c["cap"], c["cin"], c["cout"]
    n = min(c["n_ptr"], cap)
    R = ref.rows_per_block(n)
    sub = R // 4
    grid_slabs = min(ref.BW_MAX_SPLITS, -(-cap // 256))
    live_slabs = [s for s in range(grid_slabs) if s * R < n]
    ti, tj = tiles(cin), tiles(cout)
    gi, gj = -(-(-(-cin // 16)) // ti), -(-(-(-cout // 16)) // tj)
    Pi, Pj = gi * ti * 16, gj * tj * 16
    # operands as the lanes read them: channel c of row r is flat[r * C + c]; masked beyond C
    Xp, Yp = np.zeros((c["n_in"], Pi), F), np.zeros((cap, Pj), F)
    Xp[:, :cin], Yp[:, :cout] = c["X"], c["dY"]
    if mut == "ci_unmasked":
        flat = np.concatenate([c["X"].ravel(), np.zeros(Pi, F)])
        Xp = flat[np.arange(c["n_in"])[:, None] * cin + np.arange(Pi)[None, :]]
    elems = K * cin * cout
    partial = np.full(ref.BW_MAX_SPLITS * elems + 64 + Pi * Pj, np.nan, F)
    S = len(live_slabs)
    red = np.zeros((K, S, Pi, Pj), F)
    for k in range(K):
        lists = [consumed(nbr[k], s * R + w * sub, min(n, s * R + R, s * R + (w + 1) * sub), mut) for s in live_slabs for w in range(4)]
        lens = np.array([len(p) for p in lists])
        order = np.argsort(-lens, kind="stable")
        Lk = int(lens.max()) if len(lens) else 0
        src, row = np.zeros((len(lists), Lk), np.int64), np.zeros((len(lists), Lk), np.int64)
        for b, p in enumerate(lists):
            src[b, :len(p)], row[b, :len(p)] = p[:, 0], p[:, 1]
        src, row, sl = src[order], row[order], lens[order]
        acc = np.zeros((len(lists), Pi, Pj), F)
        for t in range(Lk):
            m = int((sl > t).sum())
            acc[:m] = acc[:m] + Xp[src[:m, t]][:, :, None] * Yp[row[:m, t]][:, None, :]  # the product rounded, then the addition
        back = np.empty_like(acc)
        back[order] = acc
        back = back.reshape(S, 4, Pi, Pj)
        for s in range(S):
            r_ = back[s, 0]
            for w in (1, 2, 3):
                r_ = r_ + back[s, w]
            red[k, s] = r_
    if mut == "swap_store":  # every 16 x 16 tile stored transposed
        red = red.reshape(K, S, Pi // 16, 16, Pj // 16, 16).transpose(0, 1, 2, 5, 4, 3).reshape(K, S, Pi, Pj)
    # the stores, in dispatch order (slab fastest, then k, then the channel tile group)
    for z in range(gi * gj):
        ci = (z // gj) * ti * 16 + np.arange(ti * 16)
        co = (z % gj) * tj * 16 + np.arange(tj * 16)
        keep = ((ci < cin) | (mut == "ci_unmasked"))[:, None] & (co < cout)[None, :]
        off = (ci[:, None] * cout + co[None, :])[keep]
        for k in range(K):
            for j, s in enumerate(live_slabs):
                partial[(s * K + k) * cin * cout + off] = red[k, j][np.ix_(ci, co)][keep]
    n_r = cap if mut == "slabs_from_cap" else n
    R_r = ref.rows_per_block(n_r)
    dW = np.zeros(elems, F)
    for sp in range(-(-n_r // R_r)):
        dW = dW + partial[sp * elems:(sp + 1) * elems]
    return dW.reshape(K, cin, cout)


def noticed(name, mut):
    c = cases.dw_case(name)
    want, bar = cases.dw_reference(name)
    with np.errstate(invalid="ignore"):
        got = dw_model(c, mut)
    if c["kind"] == "int":
        return not np.array_equal(got, want)
    return not np.isfinite(got).all() or ref.in_bars(got, want, bar) > 1


# ------------------------------------------------------------------------------------------------------------------ ref is torch's
def dense_gradients(coords, shape, batch, ks, stride, pad, X, W, out_coords, dY):
    """float64 autograd of F.conv3d on the densified rows -> (dX rows, dW (K, Cin, Cout))"""
    ft = torch.tensor(X, dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(W.reshape(*ks, W.shape[1], W.shape[2]), dtype=torch.float64, requires_grad=True)
    idx = torch.from_numpy(np.array(coords)).long()
    grid = torch.zeros((batch, *shape, X.shape[1]), dtype=torch.float64)
    dense = grid.index_put((idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]), ft).permute(0, 4, 1, 2, 3)
    y = TF.conv3d(dense, wt.permute(4, 3, 0, 1, 2), stride=stride, padding=pad)
    oc = np.array(out_coords)
    rows = y[oc[:, 0], :, oc[:, 1], oc[:, 2], oc[:, 3]]
    rows.backward(torch.tensor(dY, dtype=torch.float64))
    return ft.grad.numpy(), wt.grad.numpy().reshape(W.shape)


@functools.lru_cache(maxsize=None)
def subm_table(ks):
    c = gc.build("few_hundred")
    return gref.subm_rulebook(c["coords"], len(c["coords"]), c["shape"], list(ks))


@functools.lru_cache(maxsize=None)
def strided_table(geom):
    c = gc.build("odd_grid")
    return gref.sparse_rulebook(c["coords"], len(c["coords"]), c["shape"], *gc.STRIDED_GEOMETRIES[geom])


def int_layer(name, n_in, n_out, K, cin, cout):
    rng = cases._rng(name)
    return cases.values("int", rng, (n_in, cin)), cases.values("int", rng, (K, cin, cout)), cases.values("int", rng, (n_out, cout))


@pytest.mark.parametrize("ks", gc.SUBM_KERNELS, ids=lambda ks: "k%d%d%d" % tuple(ks))
def test_the_reference_is_dense_conv3d_autograd_submanifold(ks):
    c = gc.build("few_hundred")
    n, nbr = len(c["coords"]), subm_table(tuple(ks))
    X, W, dY = int_layer("host-subm", n, n, nbr.shape[0], 3, 5)
    gx, gw = dense_gradients(c["coords"], c["shape"], c["batch"], ks, 1, [k // 2 for k in ks], X, W, c["coords"], dY)
    np.testing.assert_allclose(ref.dx(nbr, n, n, dY, W), gx, rtol=0, atol=1e-10)
    np.testing.assert_allclose(ref.dw(nbr, n, X, dY), gw, rtol=0, atol=1e-10)
    # the gather form SparseConvFunction.backward relies on, and the two mistakes
    assert np.array_equal(dx_gather(nbr, n, n, dY, W, subm=True), ref.dx(nbr, n, n, dY, W))
    assert np.array_equal(dx_gather(nbr, n, n, dY, W, subm=True, mut=True), ref.dx(nbr, n, n, dY, W)) == (ks == [1, 1, 1])


@pytest.mark.parametrize("geom", list(gc.STRIDED_GEOMETRIES))
def test_the_reference_is_dense_conv3d_autograd_strided(geom):
    c = gc.build("odd_grid")
    ks, st, pd = gc.STRIDED_GEOMETRIES[geom]
    co, nbr, _, overflow = strided_table(geom)
    n_in, n = len(c["coords"]), len(co)
    assert not overflow and n > 0
    X, W, dY = int_layer("host-strided", n_in, n, nbr.shape[0], 3, 5)
    gx, gw = dense_gradients(c["coords"], c["shape"], c["batch"], ks, st, pd, X, W, co, dY)
    want = ref.dx(nbr, n, n_in, dY, W)
    np.testing.assert_allclose(want, gx, rtol=0, atol=1e-10)
    np.testing.assert_allclose(ref.dw(nbr, n, X, dY), gw, rtol=0, atol=1e-10)
    assert np.array_equal(dx_gather(nbr, n, n_in, dY, W, subm=False), want)
    assert np.array_equal(dx_gather(nbr, n, n_in, dY, W, subm=False, mut=True), want) == (geom == "k1s2p0")
    fed = ref.fed_rows(nbr, n, n_in)
    assert not want[~fed].any(), "rows that feed nothing have no gradient"
    if geom in UNFED:
        assert (~fed).sum() >= 100, (geom, int((~fed).sum()))


# on the odd grid [7, 41, 47]: kernel 1 at stride 2 skips the odd coordinates; kernel 2 at stride 2 and kernel 3 at stride 3 leave the
# last planes outside out_shape.  (3 at stride 2 tiles an odd extent exactly: every row is fed.)
UNFED = ("k1s2p0", "k2s2p0", "k3s3p0")


def dx_gather(nbr, n, n_in, dY, W, subm, mut=False):
    """SparseConvFunction.backward in float64: dX[i] = sum_k dY[T[k][i]] @ Wt[k]; submanifold T = the forward table, Wt = W reversed
    along k and transposed; strided T = the transposed table, Wt = W transposed.  mut: the offsets the other way round."""
    K = nbr.shape[0]
    T = nbr[:, :n] if subm else gref.transpose(nbr, n, n_in)
    rev = subm != mut
    out = np.zeros((n_in, W.shape[1]))
    for k in range(K):
        i = np.nonzero(T[k] >= 0)[0]
        out[i] += dY[T[k, i]].astype(np.float64) @ W[K - 1 - k if rev else k].astype(np.float64).T
    return out


# ------------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", cases.DW_IDS)
def test_a_dw_case_is_what_it_is_named_for_and_the_model_meets_it(name):
    c = cases.dw_case(name)
    want, bar = cases.dw_reference(name)
    n, cap, K = c["n"], c["cap"], c["K"]
    assert c["nbr"].shape == (K, cap) and c["X"].shape == (c["n_in"], c["cin"]) and c["dY"].shape == (cap, c["cout"])
    assert c["nbr"].max() < c["n_in"] and n == min(c["n_ptr"], cap)
    if cap > n:
        assert (c["nbr"][:, n:] >= 0).all() and np.abs(c["dY"][n:]).min() > 0, "the rows behind the live ones look live"
    g = ref.geometry(n)
    assert g["slabs"] <= min(ref.BW_MAX_SPLITS, -(-cap // 256)), "the host's grid covers the live slabs"
    if n in cases.LIVE_COUNTS:
        assert (g["R"], g["slabs"]) == {1: (256, 1), 255: (256, 1), 256: (256, 1), 257: (256, 2), 16383: (256, 64), 16384: (256, 64),
                                       16385: (512, 33), 32768: (512, 64), 32769: (768, 43)}.get(n, (256, 1))
    for k, d in enumerate(c["cols"]):
        live = c["nbr"][k, :n] >= 0
        if d == "all":
            assert live.all()
        if d == "none":
            assert not live.any() and not want[k].any()
        if d == "q79":
            assert cases.queue_peak(c["nbr"][k], n) == (79 if n >= 16385 else min(n, 15))
        if d == "random" and n >= 255:
            assert 0.05 < live.mean() < 0.45
        if d.startswith("row"):
            assert live.sum() == 1 and live[{"row0": 0, "row255": 255, "rowlast": n - 1}[d]]
    with np.errstate(invalid="ignore"):
        got = dw_model(c)
    assert got.dtype == F and np.isfinite(got).all()
    if c["kind"] == "int":
        assert ref.dw_abs(c["nbr"], n, c["X"], c["dY"]).max() < EXACT
        assert np.array_equal(got, want), "fp32 is exact on an integer case, in any order"
    else:
        fr = ref.in_bars(got, want, bar)
        print(f"{name}: model at {fr:.3f} of the bar, chain {ref.dw_chain(c['nbr'], n).tolist()}")
        assert fr <= HALF, fr
    if name in cases.SAME_BITS:
        with np.errstate(invalid="ignore"):
            base = dw_model(cases.dw_case(cases.SAME_BITS[name]))
        assert np.array_equal(got.view(np.int32), base.view(np.int32)), "the slab split depends on n only"


def test_the_cases_cover_every_tile_instantiation_and_both_group_counts():
    seen, groups = set(), set()
    for name in cases.DW_IDS:
        c = cases.DW_CASES[name]
        ti, tj = tiles(c["cin"]), tiles(c["cout"])
        seen.add((ti, tj))
        groups.add(-(-(-(-c["cin"] // 16)) // ti) * -(-(-(-c["cout"] // 16)) // tj))
    assert seen == {(a, b) for a in (1, 2, 4) for b in (1, 2, 4)}
    assert {1, 2, 4} <= groups  # 64 x 128 and 128 x 16: two groups; 128 x 128: four


MUTATIONS = [
    ("drop_partial_batch", ["live-1", "live-15", "live-17", "live-63", "live-65", "live-257"], ["live-64", "live-256"]),
    ("no_tail", ["live-15", "live-17", "dens-257"], []),
    ("no_move", ["live-17", "live-16385"], ["live-15", "live-16"]),
    ("slabs_from_cap", ["cap-257-4096", "cap-16385-65536"], ["over-256", "live-257", "real-257"]),
    ("ci_unmasked", ["chan-257-5x20", "chan-257-17x33", "chan-257-80x48", "chan-257-1x1", "chan-16385-80x48"],
     ["chan-257-16x32", "chan-257-64x64"]),
    ("swap_store", ["live-257", "chan-257-16x32"], []),
]


@pytest.mark.parametrize("mut,names,blind", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_a_mistake_in_the_model_is_noticed_by_the_named_cases(mut, names, blind):
    for name in names:
        assert noticed(name, mut), (mut, name)
    for name in blind:
        assert not noticed(name, mut), (mut, name, "the neighbour that cannot see it")


def test_the_data_gradient_cases():
    # integer bound of the data gradient: at most 27 offsets x 128 channels x |2 * 2|
    assert 27 * 128 * 4 < EXACT
    # and of the weight gradients and forwards of the module-path runs: at most one pair per output row and column
    assert 4 * max(cases.GRID_STRIDE["rows"], 20000, len(gc.build("odd_grid")["coords"])) < EXACT
    t = cases.grid_stride_table()
    rows = cases.GRID_STRIDE["rows"]
    live = t[0][t[0] >= 0]
    assert len(np.unique(live)) == len(live), "every input feeds at most one output"
    assert rows * cases.GRID_STRIDE["cin"] > 8192 * 256 >= (rows - 1) * cases.GRID_STRIDE["cin"], "the loop's second trip is the last row"
    assert (t[0] == rows - 1).sum() == 1, "and that row has a gradient"
    assert 0.7 < (t[0] >= 0).mean() < 0.9
    s = cases.large_sites()
    assert len(s["coords"]) == 20000 > 16384 and len(np.unique(s["coords"], axis=0)) == 20000


def test_the_routes_are_the_librarys():
    """cases.route states the dispatch of spconv/functional.py: the library's own table, asked for the swapped pair"""
    from vision3d_amd import _lib as L
    lib = L.lib()
    pairs = {(a, b) for a in (1, 4, 8, 16, 17, 32, 48, 64, 128) for b in (1, 4, 8, 16, 32, 33, 48, 64, 128)}
    assert {p for p in pairs if lib.v3d_sparse_conv_packed_supported(*p)} == set(cases.FORWARD_PAIRS)
    want = {(4, 16): "scalar", (4, 32): "scalar", (64, 128): "scalar", (16, 16): "packed", (16, 32): "packed", (32, 32): "packed",
            (32, 64): "packed", (64, 64): "packed", (32, 16): "packed", (64, 32): "packed", (128, 128): "packed",
            (16, 8): "scalar", (8, 16): "scalar", (48, 16): "scalar", (16, 4): "wave"}
    assert {p: cases.route(*p) for p in cases.FORWARD_PAIRS + cases.ALGO1_LAYERS} == want

"""Seeded cases of the sparse convolution's two gradients, shared by tests/test_host_spconv_grad_ref.py and
tests/test_gpu_spconv_grad_edges.py.  numpy only; nothing here computes an expected value (tests/spconv_grad_ref.py does).

Two value kinds.  "int": X, dY and W drawn from {-2 .. 2}.  Every partial sum of a weight gradient is then at most 4 x 32 769 pairs and
every partial sum of a data gradient at most 27 x 128 x 4, far below 2^24, so fp32 is exact in ANY order, and so is the bf16x3 split (the
hi piece is the value, the lo piece 0): these cases are compared for EQUALITY with float64, element for element -- one dropped, doubled
or misplaced pair fails them.  "real": standard normal values, judged by the bars of tests/spconv_grad_ref.py; they watch the
arithmetic and the summation order.

dW cases (`dw_case(name)`) are synthetic tables: nbr (K, cap) int32 uploaded as they are, no geometry behind them; the sources of the live
entries are random rows of X (n_in rows, set apart from n).  One density per COLUMN, so one case carries several:
  all          every row live                                none        no row live: dW[k] is exactly 0
  q79          relative to the wave's sub-slab, 64-row batch 0, 2, .. has its first 15 rows live and batch 1, 3, .. all 64: the queue holds
               15 leftovers + 64 = 79 entries from a sub-slab of 128 rows on (n >= 16 385); below it is a lone tail of 15
  one_per_64   row 37 of every 64                            random      a share of 10 - 40 % of the rows, drawn per column
  row<o>       the single row o
Behind the n live rows (cap > n) the table holds live-LOOKING entries and dY non-zero rows: whatever reads them is noticed.
A case whose spec names `data` draws its live part from that other case's generator: the same rows, sources and values under another
capacity, so the two results can be compared bit for bit.
"""
import numpy as np

import spconv_grad_ref as ref

F = np.float32
LIVE_COUNTS = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 16383, 16384, 16385, 32768, 32769]
FOUR = ["all", "q79", "one_per_64", "random"]
FIVE = ["all", "none", "q79", "one_per_64", "random"]
CHANNELS = [(4, 16), (16, 16), (16, 32), (32, 64), (64, 64), (64, 128), (128, 128), (128, 16)]
RAGGED = [(1, 1), (5, 20), (17, 33), (80, 48)]
REST = [(16, 64), (32, 16), (64, 32)]  # the tile shapes 1 x 4, 2 x 1 and 4 x 2, which the two lists above leave out
CHANNEL_ROWS = [257, 16385]
GUARD = 4096  # floats in front of and behind dW that must stay untouched

# the (Cin, Cout) pairs the forward MFMA kernels exist for (csrc/spconv.hip, v3d_i_sparse_conv_packed_supported)
FORWARD_PAIRS = [(4, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (4, 32), (32, 16), (64, 32), (64, 128), (128, 128)]
ALGO1_LAYERS = [(16, 8), (8, 16), (48, 16), (16, 4)]  # layers only the scalar forward runs (module.algo = 1)


def route(cin, cout):
    """the kernel the data gradient of a Cin -> Cout layer takes: the transposed layer is Cout -> Cin"""
    if (cout, cin) not in FORWARD_PAIRS:
        return "scalar"
    return "packed" if cout >= 16 else "wave"


def _rng(name):
    return np.random.default_rng([20262, sum(ord(ch) * (i + 1) for i, ch in enumerate(name))])


def values(kind, rng, shape):
    if kind == "int":
        return rng.integers(-2, 3, size=shape).astype(F)
    return rng.standard_normal(shape).astype(F)


def live_mask(density, n, rng):
    o = np.arange(n)
    if density == "all":
        return np.ones(n, bool)
    if density == "none":
        return np.zeros(n, bool)
    if density == "q79":
        sub = ref.geometry(max(n, 1))["sub"]
        batch, lane = (o % sub) // 64, o % 64  # sub is a multiple of 64
        return (batch % 2 == 1) | (lane < 15)
    if density == "one_per_64":
        return o % 64 == 37
    if density == "random":
        return rng.random(n) < rng.uniform(0.1, 0.4)
    if density.startswith("row"):
        return o == (n - 1 if density == "rowlast" else int(density[3:]))
    raise KeyError(density)


def _spec(n, cols, cin=16, cout=16, kind="int", **kw):
    return dict(n=n, cols=list(cols), cin=cin, cout=cout, kind=kind, **kw)


DW_CASES = {}
for _n in LIVE_COUNTS:
    DW_CASES[f"live-{_n}"] = _spec(_n, FOUR)
for _n in (257, 16385, 32769):
    DW_CASES[f"dens-{_n}"] = _spec(_n, FIVE)
DW_CASES["single-first"] = _spec(600, ["row0"])
DW_CASES["single-slab-end"] = _spec(600, ["row255"])
DW_CASES["single-last"] = _spec(600, ["rowlast"])
DW_CASES["src-one-257"] = _spec(257, FOUR, n_in=1)
DW_CASES["src-one-16385"] = _spec(16385, FOUR, n_in=1)
DW_CASES["src-3n-16385"] = _spec(16385, FOUR, n_in=3 * 16385)
for _n in CHANNEL_ROWS:
    for _ci, _co in CHANNELS + RAGGED + REST:
        DW_CASES[f"chan-{_n}-{_ci}x{_co}"] = _spec(_n, ["all", "q79", "random"], _ci, _co)
    DW_CASES[f"k1-{_n}"] = _spec(_n, ["random"], 32, 32)
    DW_CASES[f"k27-{_n}"] = _spec(_n, (FIVE * 6)[:27], 32, 32)
for _n in (256, 257, 16385, 32769):
    DW_CASES[f"real-{_n}"] = _spec(_n, FOUR, kind="real")
DW_CASES["real-16385-64x128"] = _spec(16385, ["all", "q79", "random"], 64, 128, kind="real")
DW_CASES["real-257-17x33"] = _spec(257, ["all", "q79", "random"], 17, 33, kind="real")
DW_CASES["real-257-128x128"] = _spec(257, ["all", "q79", "random"], 128, 128, kind="real")
# capacity: the slab split depends on n only, so these equal the cap == n result bit for bit
DW_CASES["cap-257-4096"] = _spec(257, FOUR, kind="real", cap=4096, data="real-257")
DW_CASES["cap-16385-65536"] = _spec(16385, FOUR, kind="real", cap=65536, data="real-16385")
DW_CASES["cap-0-256"] = _spec(0, FOUR, kind="real", cap=256, n_in=64)
DW_CASES["over-256"] = _spec(256, FOUR, kind="real", cap=256, n_ptr=256 + 44, data="real-256")
SAME_BITS = {"cap-257-4096": "real-257", "cap-16385-65536": "real-16385", "over-256": "real-256"}
DW_IDS = list(DW_CASES)
INT_IDS = [k for k, v in DW_CASES.items() if v["kind"] == "int"]
REAL_IDS = [k for k, v in DW_CASES.items() if v["kind"] == "real"]

_CACHE = {}


def dw_case(name):
    """-> dict(nbr (K, cap) int32, n, n_ptr, cap, n_in, K, cin, cout, X (n_in, cin), dY (cap, cout), kind, cols); built once per
    process, the arrays are read-only"""
    if name in _CACHE:
        return _CACHE[name]
    s = DW_CASES[name]
    n, K, cin, cout, kind = s["n"], len(s["cols"]), s["cin"], s["cout"], s["kind"]
    cap, n_in = s.get("cap", max(n, 1)), s.get("n_in", max(n, 1))
    rng = _rng(s.get("data", name))
    nbr = np.full((K, cap), -1, np.int32)
    for k, d in enumerate(s["cols"]):
        nbr[k, :n] = np.where(live_mask(d, n, rng), rng.integers(0, n_in, n), -1)
    X = values(kind, rng, (n_in, cin))
    dY = np.empty((cap, cout), F)
    dY[:n] = values(kind, rng, (n, cout))
    pad = _rng(name + "/pad")
    nbr[:, n:] = pad.integers(0, n_in, (K, cap - n))
    dY[n:] = values(kind, pad, (cap - n, cout)) + F(3)
    c = dict(name=name, nbr=nbr, n=n, n_ptr=s.get("n_ptr", n), cap=cap, n_in=n_in, K=K, cin=cin, cout=cout, X=X, dY=dY, kind=kind,
             cols=s["cols"])
    for a in (nbr, X, dY):
        a.setflags(write=False)
    _CACHE[name] = c
    return c


_REF = {}


def dw_reference(name):
    """-> (dW float64, bar) of the case, computed once"""
    if name not in _REF:
        c = dw_case(name)
        want = ref.dw(c["nbr"], c["n"], c["X"], c["dY"])
        bar = ref.dw_bar(c["nbr"], c["n"], c["X"], c["dY"]) if c["kind"] == "real" else np.zeros_like(want)
        want.setflags(write=False)
        bar.setflags(write=False)
        _REF[name] = (want, bar)
    return _REF[name]


def queue_peak(nbr_k, n):
    """the longest the wave queue of spconv_bwd_weight_tiles gets on one column: entries held after a 64-row batch was appended"""
    g = ref.geometry(max(n, 1))
    peak = 0
    for lo in range(0, n, g["sub"]):
        cnt = 0
        for o0 in range(lo, min(n, lo + g["sub"]), 64):
            cnt += int((nbr_k[o0:min(o0 + 64, n, lo + g["sub"])] >= 0).sum())
            peak = max(peak, cnt)
            cnt %= ref.BW_BATCH
    return peak


# ------------------------------------------------------------------------------------------------ the data gradient
# the transposed layer is 8 -> 32, a pair without an MFMA kernel: the scalar kernel writes 65 537 x 32 outputs, 32 more than 8192 x 256 threads
GRID_STRIDE = dict(rows=65537, cin=32, cout=8)


def grid_stride_table():
    """(1, rows) forward table of a K = 1 layer: a random matching of outputs to inputs (every input feeds at most one output, as in any
    rulebook), a fifth of the outputs without a source; the LAST input row is fed: its 32 gradients are the ones the loop's second
    trip writes"""
    rows = GRID_STRIDE["rows"]
    rng = _rng("grid_stride")
    perm = rng.permutation(rows).astype(np.int32)
    nbr = np.where(rng.random(rows) < 0.8, perm, -1).astype(np.int32)
    nbr[np.nonzero(perm == rows - 1)[0]] = rows - 1
    return nbr[None]


def large_sites():
    """20 000 sites on the [8, 80, 80] x 2 grid: above the 16 384 rows up to which the packed route runs its ring kernel"""
    import geometry_cases as gc
    return dict(coords=gc._sites(_rng("large_sites"), [8, 80, 80], 2, n=20000), shape=[8, 80, 80], batch=2)

"""Seeded inputs for the two training BatchNorm + ReLU implementations (csrc/sparse_bn.hip; dt_bn_* of csrc/dense_train.hip) at their
unroll, chunk, cap, merge and grid edges; shared by tests/test_host_bn_ref.py, which proves on the float64 reference alone that every case
has the property it is named for, and tests/test_gpu_bn_edges.py.  Every builder is cached, its arrays read-only, its generator seeded with
the crc32 of its arguments (tests/proposal_cases.py).

SPARSE  sparse_case(id) -> dict(x, dy (n, C) f32, gamma, beta (C,) f32, eps, relu, momentum, r_mean, r_var (C,) f32 or None, nbt int or
None, kind).  RL = 1024 / C rows are in flight; the statistics take 4 RL rows per trip, the backward sums 2 RL, a tail loop the rest.
  unroll-c{16,64,256}-n{RL-1,RL,RL+1,2RL-1,2RL,2RL+1,4RL-1,4RL,4RL+1}   one chunk (n within [2, 256])
  unroll-c{4,8}-n{2,3,255,256}      RL = 256 / 128: a chunk holds at most 256 rows, the unrolled statistics loop needs 1024 / 512 -- these
                                    widths run the tail loops only (and, for C = 8, one unrolled backward trip from n = 129 on)
  chunks-c{16,128}-n{257,511,512,513,1025}     G = 2, 2, 2, 3, 5; the last chunk short
  merge-c4-n{65280,65536,65537}     G = 255, 256, 257 against Q = 256 merge groups;   merge-c256-n{768,1024,1025}: G = 3, 4, 5 against Q = 4
  cap-c{4,16}-n{131071,131072,131073,140000}   G = 512; from 131 073 on ceil(n / 512) rows a chunk leave chunk 511 EMPTY
  kind-{iid,offset_1e2,offset_1e4,sorted,constant,outlier,gamma_mixed,no_relu,tie}-n{5000,513}   at C = 16 / 128:
      offset_*   mean = 1e2 / 1e4 std (1e4: the rows keep 0.3 std away from the ReLU's edge -- there the bar of v is itself 0.05 std)
      sorted     every channel ascending: the chunk means are far apart, n_b (mean_b - mean)^2 is most of the variance
      constant   one channel constant;   outlier: one row at mean + 1e4 std;   gamma_mixed: both signs, every fifth gamma = 0
      tie        a quarter of the rows equal one row x0, beta = -(x0 - mean) invstd gamma: v(x0) = 0 but for rounding
  book-{mom_0.01,mom_1,mom_0,no_running,no_counter}   running statistics from non-trivial values; NULL pair; NULL counter
  one_row    n = 1: served by the C ABI (torch refuses it)

DENSE  bf16 NHWC, 128 channels; every input is rounded to bf16 first and carried as the float32 of that value (bits: bf16_bits).
  finalize_case(tiles, kind, below)  tiles in FINALIZE_TILES, kind iid / offset (|mean| / std = 100), count = 128 tiles or 77 less
  finalize_case(1, "iid", "one")     count = 1
  apply_case(M, relu)                M in APPLY_M (16 pixels a block, 4096 blocks: the stride starts at 65 537)
  bwd_case(M, relu, kind)            M in BWD_M (512 blocks: the reduction strides from 8193 on); kinds at M = 8209, the tie also at 4096

JUDGING A RUN  sparse_fractions, sparse_float64_mask_fractions, dense_finalize_fractions, dense_bwd_fractions: the outputs of a run -- the
host model's in tests/test_host_bn_ref.py, the GPU's in tests/test_gpu_bn_edges.py -- in units of their bars.
"""
import functools
import zlib

import numpy as np

import bn_ref as ref

F = np.float32
EPS = 1e-3

# ------------------------------------------------------------------------------------------------------------------ sparse
UNROLL_C = [16, 64, 256]
SMALL_C, SMALL_N = [4, 8], [2, 3, 255, 256]
CHUNK_C, CHUNK_N = [16, 128], [257, 511, 512, 513, 1025]
MERGE = {4: [65280, 65536, 65537], 256: [768, 1024, 1025]}
CAP_C, CAP_N = [4, 16], [131071, 131072, 131073, 140000]
KINDS = ["iid", "offset_1e2", "offset_1e4", "sorted", "constant", "outlier", "gamma_mixed", "no_relu", "tie"]
KIND_SHAPES = [(5000, 16), (513, 128)]
BOOK = {"mom_0.01": dict(momentum=0.01), "mom_1": dict(momentum=1.0), "mom_0": dict(momentum=0.0), "no_running": dict(running=False),
        "no_counter": dict(counter=False)}
# (G, rows per chunk, empty chunks), worked by hand from clamp(ceil(n / 256), 1, 512) and ceil(n / G); test_host_bn_ref.py checks them
GEOMETRY = {257: (2, 129, 0), 511: (2, 256, 0), 512: (2, 256, 0), 513: (3, 171, 0), 1025: (5, 205, 0), 5000: (20, 250, 0),
            65280: (255, 256, 0), 65536: (256, 256, 0), 65537: (257, 256, 0), 768: (3, 256, 0), 1024: (4, 256, 0),
            131071: (512, 256, 0), 131072: (512, 256, 0), 131073: (512, 257, 1), 140000: (512, 274, 1)}


def unroll_sizes(C):
    RL = 1024 // C
    return [n for n in (RL - 1, RL, RL + 1, 2 * RL - 1, 2 * RL, 2 * RL + 1, 4 * RL - 1, 4 * RL, 4 * RL + 1) if 2 <= n <= 256]


def _table():
    t = {}
    for C in UNROLL_C:
        for n in unroll_sizes(C):
            t[f"unroll-c{C}-n{n}"] = (n, C, "iid", {})
    for C in SMALL_C:
        for n in SMALL_N:
            t[f"unroll-c{C}-n{n}"] = (n, C, "iid", {})
    for C in CHUNK_C:
        for n in CHUNK_N:
            t[f"chunks-c{C}-n{n}"] = (n, C, "iid", {})
    for C, sizes in MERGE.items():
        for n in sizes:
            t[f"merge-c{C}-n{n}"] = (n, C, "iid", {})
    for C in CAP_C:
        for n in CAP_N:
            t[f"cap-c{C}-n{n}"] = (n, C, "iid", {})
    for n, C in KIND_SHAPES:
        for kind in KINDS:
            t[f"kind-{kind}-n{n}"] = (n, C, kind, {})
    for name, opt in BOOK.items():
        t[f"book-{name}"] = (513, 16, "iid", opt)
    t["one_row"] = (1, 16, "iid", {})
    return t


SPARSE = _table()
SPARSE_IDS = list(SPARSE)
# a seed per case where the default one puts more than 0.1 % of the pre-activations within their bar of 0 (test_host_bn_ref.py asserts)
SEEDS = {}


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _stats(x, eps=EPS):
    x = np.asarray(x, np.float64)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, 1.0 / np.sqrt(var + float(F(eps)))


@functools.lru_cache(maxsize=None)
def sparse_case(name):
    n, C, kind, opt = SPARSE[name]
    rng = _rng("sparse", name, SEEDS.get(name, 0))
    m = rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)
    s = rng.uniform(0.5, 2.0, C)
    z = rng.standard_normal((n, C))
    gamma = rng.uniform(0.5, 1.5, C)
    beta = rng.normal(0.0, 0.3, C)
    relu = 1
    if kind == "gamma_mixed":
        gamma *= rng.choice([-1.0, 1.0], C)
        gamma[::5] = 0.0
    if kind == "no_relu":
        relu = 0
    if kind.startswith("offset"):
        ratio = float(kind.split("_")[1])
        if ratio >= 1e4:  # keep the rows 0.3 std away from v = 0
            z0 = -beta / gamma
            d = z - z0
            z = np.where(np.abs(d) < 0.3, z0 + np.where(d < 0, -1.0, 1.0) * (0.3 + np.abs(d)), z)
        x = s * (ratio + z)
    else:
        x = m + s * z
    if kind == "sorted":
        x = np.sort(x, axis=0)
    if kind == "constant":
        x[:, C // 3] = 1.2345
    if kind == "outlier":
        x[n // 2] = m + 1e4 * s
    if kind == "tie":
        rows = rng.choice(np.arange(1, n), n // 4, replace=False)
        x[rows] = x[0]
    x = np.ascontiguousarray(x, F)
    if kind == "tie":
        mean, _, invstd = _stats(x)
        beta = -(x[0].astype(np.float64) - mean) * invstd * gamma
    out = dict(x=x, dy=rng.standard_normal((n, C)).astype(F), gamma=gamma.astype(F), beta=beta.astype(F), eps=EPS, relu=relu,
               momentum=opt.get("momentum", 0.01), kind=kind, n=n, C=C,
               r_mean=rng.normal(0.0, 0.5, C).astype(F) if opt.get("running", True) else None,
               r_var=rng.uniform(0.5, 3.0, C).astype(F) if opt.get("running", True) else None,
               nbt=41 if opt.get("counter", True) else None)
    return _freeze(out)


@functools.lru_cache(maxsize=4)
def sparse_reference(name):
    """float64: the forward, its bars, the running statistics and theirs"""
    c = sparse_case(name)
    fw = ref.bn_forward(c["x"], c["gamma"], c["beta"], c["eps"], c["relu"])
    bars = ref.sparse_forward_bars(c["x"], c["gamma"], c["beta"], c["eps"], fw)
    if c["r_mean"] is not None:
        fw["running_mean"], fw["running_var"] = ref.bn_running(c["r_mean"], c["r_var"], fw["mean"], fw["var_unbiased"], c["momentum"])
        bars["running_mean"] = ref.running_bar(c["r_mean"], fw["mean"], bars["mean"], c["momentum"])
        bars["running_var"] = ref.running_bar(c["r_var"], fw["var_unbiased"], bars["var_unbiased"], c["momentum"])
    fw["near"] = ref.near_zero(fw["v"], bars["v"]) if c["relu"] else np.zeros(fw["v"].shape, bool)
    for d in (fw, bars):
        _freeze(d)
    return fw, bars


# ------------------------------------------------------------------------------------------------------------------ dense
FINALIZE_TILES = [1, 31, 32, 33, 64, 275, 1025]
APPLY_M = [1, 15, 16, 17, 432, 65535, 65536, 65537]
BWD_M = [1, 15, 16, 17, 8191, 8192, 8193, 8208, 8209, 35200]
BWD_KINDS = ["iid", "offset_1e2", "gamma_mixed", "tie"]
KIND_M = 8209
TIE_M = 4096
FINALIZE_RUNS = [(t, k, b) for t in FINALIZE_TILES for k in ("iid", "offset") for b in ("full", "below")] + [(1, "iid", "one")]
APPLY_RUNS = [(M, relu) for M in APPLY_M for relu in (1, 0)]
BWD_RUNS = ([(M, relu, "iid") for M in BWD_M for relu in (1, 0)] + [(KIND_M, 1, k) for k in BWD_KINDS[1:]] + [(TIE_M, 1, "tie")])


def run_id(run):
    return "-".join(str(p) for p in run)


def bf16_round(a):
    """float32 -> the float32 value of its bf16 rounding (to nearest, ties to even)"""
    b = np.ascontiguousarray(a, F).view(np.uint32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) & np.uint32(0xFFFF0000)).view(F)


def bf16_bits(a):
    """the 16 stored bits of bf16-valued float32 data"""
    b = np.ascontiguousarray(a, F).view(np.uint32)
    assert not (b & 0xFFFF).any(), "not a bf16 value"
    return (b >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(F)


def _dense_x(rng, M, kind):
    s = rng.uniform(0.5, 2.0, ref.DT_C).astype(F)
    m = (rng.uniform(0.5, 1.5, ref.DT_C) * rng.choice([-1.0, 1.0], ref.DT_C)).astype(F)
    z = rng.standard_normal((M, ref.DT_C), dtype=F)
    if kind.startswith("offset"):
        return bf16_round(s * (F(100.0) + z))
    return bf16_round(m + s * z)


@functools.lru_cache(maxsize=2)
def _finalize_data(tiles, kind):
    x = _dense_x(_rng("finalize", tiles, kind), tiles * 128, kind)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def finalize_case(tiles, kind, below):
    """-> dict(partial (tiles, 2, 128) f32 built in fp32 tile by tile, count, true_var: float64 variance of the pixels themselves)"""
    x = _finalize_data(tiles, kind)
    count = {"full": tiles * 128, "below": tiles * 128 - 77, "one": 1}[below]
    x = x[:count]
    pad = np.zeros((tiles * 128, ref.DT_C), F)
    pad[:count] = x
    pad = pad.reshape(tiles, 128, ref.DT_C)
    partial = np.stack([pad.sum(1, dtype=F), (pad * pad).sum(1, dtype=F)], 1)
    rng = _rng("finalize-running", tiles, kind, below)
    xd = x.astype(np.float64)
    return _freeze(dict(partial=np.ascontiguousarray(partial, F), count=count, tiles=tiles, eps=EPS, momentum=0.1 if kind == "offset" else 0.01,
                        r_mean=rng.normal(0.0, 0.5, ref.DT_C).astype(F), r_var=rng.uniform(0.5, 3.0, ref.DT_C).astype(F), nbt=7,
                        true_mean=xd.mean(0), true_var=xd.var(0)))


def _dense_case(rng, M, relu, kind):
    x = _dense_x(rng, M, kind)
    gamma = rng.uniform(0.5, 1.5, ref.DT_C)
    beta = rng.normal(0.0, 0.2, ref.DT_C)
    if kind == "gamma_mixed":
        gamma *= rng.choice([-1.0, 1.0], ref.DT_C)
        gamma[::5] = 0.0
    if kind == "tie":
        rows = rng.choice(np.arange(1, M), M // 4, replace=False)
        x[rows] = x[0]
    mean, _, invstd = _stats(x)
    mean, invstd = mean.astype(F), invstd.astype(F)  # what the kernels are handed
    if kind == "tie":
        beta = -(x[0].astype(np.float64) - mean) * invstd * gamma
    return dict(x=x, mean=mean, invstd=invstd, gamma=gamma.astype(F), beta=beta.astype(F), relu=relu, M=M, kind=kind)


@functools.lru_cache(maxsize=2)
def apply_case(M, relu):
    rng = _rng("apply", M)  # relu on and off share the input
    c = _dense_case(rng, M, relu, "iid")
    c.update(ref.dense_apply_reference(c["x"], c["mean"], c["invstd"], c["gamma"], c["beta"], relu))
    return _freeze(c)


@functools.lru_cache(maxsize=2)
def bwd_case(M, relu, kind):
    rng = _rng("bwd", M, kind)
    c = _dense_case(rng, M, relu, kind)
    c["dy"] = bf16_round(rng.standard_normal((M, ref.DT_C), dtype=F))
    c.update(ref.dense_apply_reference(c["x"], c["mean"], c["invstd"], c["gamma"], c["beta"], relu))
    c["near"] = ref.near_zero(c["v"], c["bar_v"]) if relu else np.zeros(c["v"].shape, bool)
    return _freeze(c)


# ------------------------------------------------------------------------------------------------------------------ judging a run
def sparse_fractions(name, got):
    """every output of a sparse run (the model's here, the GPU's in tests/test_gpu_bn_edges.py) in units of its bar -> dict; the
    backward against bn_backward on the run's OWN save_mean / save_invstd with mask = (y > 0): nothing is left out"""
    c = sparse_case(name)
    fw, bars = sparse_reference(name)
    out = dict(y=ref.in_bars(got["y"], fw["y"], bars["y"]), save_mean=ref.in_bars(got["save_mean"], fw["mean"], bars["mean"]),
               save_invstd=ref.in_bars(got["save_invstd"], fw["invstd"], bars["invstd"]),
               var_unbiased=ref.in_bars(got["var_unbiased"], fw["var_unbiased"], bars["var_unbiased"]))
    if c["r_mean"] is not None:
        out["running_mean"] = ref.in_bars(got["running_mean"], fw["running_mean"], bars["running_mean"])
        out["running_var"] = ref.in_bars(got["running_var"], fw["running_var"], bars["running_var"])
    mask = (got["y"] > 0) if c["relu"] else None
    bw = ref.bn_backward(c["x"], c["dy"], got["save_mean"], got["save_invstd"], c["gamma"], c["beta"], c["relu"], mask=mask)
    bb = ref.backward_bars(bw, c["gamma"], got["save_invstd"], ref.sbn_geometry(c["n"], c["C"])["k_bwd"])
    for k in ("dx", "dgamma", "dbeta"):
        out[k] = ref.in_bars(got[k], bw[k], bb[k])
    return out


def sparse_float64_mask_fractions(name, got):
    """the same backward against the FLOAT64 mask: the near-zero elements left out of dx, their |dy|, |dy xhat| in the bars of the sums;
    also: (y > 0) equals the float64 mask off the near-zero set"""
    c = sparse_case(name)
    fw, _ = sparse_reference(name)
    near = fw["near"]
    bw = ref.bn_backward(c["x"], c["dy"], got["save_mean"], got["save_invstd"], c["gamma"], c["beta"], c["relu"])
    bb = ref.backward_bars(bw, c["gamma"], got["save_invstd"], ref.sbn_geometry(c["n"], c["C"])["k_bwd"], near=near, dy=c["dy"])
    if c["relu"]:
        assert np.array_equal((got["y"] > 0)[~near], (fw["v"] > 0)[~near]), f"{name}: y > 0 against the float64 mask"
    return dict(dx=ref.in_bars(got["dx"][~near], bw["dx"][~near], bb["dx"][~near]), dgamma=ref.in_bars(got["dgamma"], bw["dgamma"], bb["dgamma"]),
                dbeta=ref.in_bars(got["dbeta"], bw["dbeta"], bb["dbeta"]))


def dense_bwd_fractions(c, got, y):
    """a dense backward run in units of its bars, against bn_backward with mask = (y > 0), y the forward's stored output: nothing is
    left out"""
    bw = ref.bn_backward(c["x"], c["dy"], c["mean"], c["invstd"], c["gamma"], c["beta"], c["relu"], mask=(y > 0) if c["relu"] else None)
    bb = ref.backward_bars(bw, c["gamma"], c["invstd"], ref.dense_geometry(c["M"])["k_bwd"], bf16=True)
    return {("dx_bf16" if k == "dx" else k): ref.in_bars(got[k], bw[k], bb[k]) for k in ("dx", "dgamma", "dbeta")}


def dense_finalize_fractions(c, got):
    fin = ref.dense_finalize(c["partial"], c["count"], c["eps"])
    bars = ref.dense_finalize_bars(c["partial"], c["count"], c["eps"], fin, c["momentum"], c["r_mean"], c["r_var"])
    fin["running_mean"], fin["running_var"] = ref.bn_running(c["r_mean"], c["r_var"], fin["mean"], fin["var_unbiased"], c["momentum"])
    return {k: ref.in_bars(got[k], fin[k], bars[k]) for k in ("mean", "invstd", "running_mean", "running_var")}

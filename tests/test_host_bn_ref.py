"""Host: tests/bn_ref.py against torch's float64 BatchNorm autograd, every case of tests/bn_cases.py against the property it is named for,
and a plain numpy float32 MODEL of each kernel's arithmetic and summation order against the bars.  What this file establishes for
tests/test_gpu_bn_edges.py:
  * bn_ref is torch.nn.BatchNorm1d / 2d (+ ReLU) in float64: outputs, the three gradients, the running statistics;
  * every case is well-posed: its chunk geometry is the hand-worked one (the cap cases have ONE empty chunk), "sorted" has its variance
    between the chunks, the offsets have their |mean| / std, and -- the tie kind apart -- at most 0.1 % of the float64 pre-activations
    lie within their own bar of 0 (those elements are left out of the dx / mask comparisons against the float64 mask; their |dy| and
    |dy xhat| join the bars of dbeta / dgamma);
  * the bars are neither too tight nor idle: the fp32 model of the kernels (sparse: row-lane partials in the unrolled order, lane sum,
    chunk mean, second pass, float64 merge in group order, the elementwise passes, the backward sums and merge; dense: 32-part column
    sums, the folded apply, sweep / row-group / column sums of the backward) stays within HALF of every bar on every case, and each of
    these mistakes, made in the model, breaks a bar on the named cases (no mutated library is built or run on a GPU):
      sparse   between-chunk term dropped        kind-sorted-*                fp32 E[x^2] - mean^2      kind-offset_1e4-*
               biased / unbiased swapped         unroll-c{4,8}-n{2,3}         last chunk counted full   chunks-c*-n{257,511}
               tail rows skipped                 unroll-c*-n{4RL+1,2RL+1}     empty chunk counted       cap-c*-n{131073,140000}
               mask from xhat > 0                kind-iid-*, chunks-*         dgamma from x             kind-iid-*, kind-offset_1e2-*
               dx without its mean terms         kind-iid-*                   momentum reversed         book-mom_1, book-mom_0
      dense    count = 128 tiles                 every "below" run            rows past 32 dropped      tiles 33, 64, 275, 1025
               no stride in the reduction        M = 8193, 8208, 8209, 35200  no stride in the apply    M = 65537
               1 / M of the padded M             M = 15, 17                   (mask from xhat: the tie runs -- counted, see below)
The dense tie runs also COUNT, in the model, how many masks the backward's former expression fmaf(xhat, gamma, beta) > 0 decides
differently from the forward's fmaf(x, sc, sh) > 0 (printed; the kernels now share the forward's).
"""
import numpy as np
import pytest
import torch

import bn_cases as cases
import bn_ref as ref
from bn_cases import dense_bwd_fractions, dense_finalize_fractions, sparse_float64_mask_fractions, sparse_fractions

F = np.float32
HALF = 0.5
NEAR_SHARE = 1e-3


# ------------------------------------------------------------------------------------------------------------------ the sparse model
def sparse_model(c, mut=None, bwd_stats=None):
    """csrc/sparse_bn.hip in numpy float32, operation by operation (the library is compiled without contraction) -> dict of the outputs.
    `mut` names one deliberate mistake."""
    x, dy, ga, be = c["x"], c["dy"], c["gamma"], c["beta"]
    n, C = x.shape
    geo = ref.sbn_geometry(n, C)
    G, rows, RL, Q, cnt = geo["G"], geo["rows"], geo["RL"], geo["Q"], geo["counts"]
    K = -(-rows // RL)
    K4 = -(-K // 4) * 4

    def lanes(a):  # (n, C) -> (G, K4, RL, C): row b * rows + k * RL + rl of chunk b, zeros where there is none
        flat = np.zeros((G * rows, C), F)
        flat[:n] = a
        pad = np.zeros((G, K4 * RL, C), F)
        pad[:, :rows] = flat.reshape(G, rows, C)
        return pad.reshape(G, K4, RL, C)

    valid = np.arange(K4 * RL).reshape(K4, RL)[None] < cnt[:, None, None]
    cnt_l = valid.sum(1)  # rows of lane rl in chunk b

    def unrolled(v):  # s += (a + b) + (c + d) while four rows remain, then s += a
        s = np.zeros((G, RL, C), F)
        for t in range(K4 // 4):
            a, b, c_, d = v[:, 4 * t], v[:, 4 * t + 1], v[:, 4 * t + 2], v[:, 4 * t + 3]
            full = (cnt_l >= 4 * t + 4)[..., None]
            tail = s if mut == "skip_tail" else (((s + a) + b) + c_) + d
            s = np.where(full, s + ((a + b) + (c_ + d)), tail)
        return s

    def lane_sum(s):
        t = np.zeros((G, C), F)
        for q in range(RL):
            t = t + s[:, q]
        return t

    def grouped(a):  # float64: thread (q, c) adds chunks q, q + Q, ...; then the Q groups in order
        Gp = -(-G // Q) * Q
        pad = np.zeros((Gp, C))
        pad[:G] = a
        pad = pad.reshape(Gp // Q, Q, C)
        acc = np.zeros((Q, C))
        for i in range(Gp // Q):
            acc = acc + pad[i]
        t = np.zeros(C)
        for j in range(Q):
            t = t + acc[j]
        return t

    xl = lanes(x)
    cnt_div = np.where(cnt > 0, rows, 0) if mut == "last_full" else cnt
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_b = np.where(cnt[:, None] > 0, lane_sum(unrolled(xl)) / cnt_div[:, None].astype(F), F(0))
    dv = xl - mean_b[:, None, None, :]
    m2_b = lane_sum(unrolled(np.where(valid[..., None], dv * dv, F(0))))
    p0 = (np.where(cnt == 0, rows, cnt_div) if mut == "empty_counted" else cnt_div).astype(F).astype(np.float64)[:, None]
    pm, pm2 = mean_b.astype(np.float64), m2_b.astype(np.float64)
    mean = grouped(p0 * pm) / n
    d = pm - mean
    m2 = grouped(pm2 if mut == "no_between" else pm2 + p0 * d * d)
    var_b = (m2 / n).astype(F)
    var_u = (m2 / (n - 1)).astype(F) if n > 1 else var_b
    save_mean = mean.astype(F)
    if mut == "e2_fp32":
        save_mean = x.sum(0, dtype=F) / F(n)
        var_b = np.maximum((x * x).sum(0, dtype=F) / F(n) - save_mean * save_mean, F(0))
        var_u = var_b * F(n) / F(max(n - 1, 1))
    if mut == "swap_var":
        var_b, var_u = var_u, var_b
    invstd = F(1) / np.sqrt(var_b + F(c["eps"]))
    out = dict(save_mean=save_mean, save_invstd=invstd, var_unbiased=var_u)
    if c["r_mean"] is not None:
        mom = F(c["momentum"])
        a, b = (mom, F(1) - mom) if mut == "mom_rev" else (F(1) - mom, mom)
        out["running_mean"] = a * c["r_mean"] + b * save_mean
        out["running_var"] = a * c["r_var"] + b * var_u
    v = (x - save_mean) * invstd * ga + be
    out["y"] = np.maximum(v, F(0)) if c["relu"] else v
    # backward, from the forward's own statistics (or the ones handed in)
    m_, is_ = bwd_stats if bwd_stats is not None else (save_mean, invstd)
    xhat = (x - m_) * is_
    keep = (xhat > 0) if mut == "mask_xhat" else (xhat * ga + be > 0)
    dz = np.where(keep, dy, F(0)) if c["relu"] else dy
    dzl, hl = lanes(dz), lanes(x if mut == "dgamma_x" else xhat)
    s0, s1 = np.zeros((G, RL, C), F), np.zeros((G, RL, C), F)
    for k in range(K):  # two rows per trip while two remain, then one: the sums stay sequential
        if mut == "skip_tail":
            live = (k < 2 * (cnt_l // 2))[..., None]
            s0, s1 = np.where(live, s0 + dzl[:, k], s0), np.where(live, s1 + dzl[:, k] * hl[:, k], s1)
        else:
            s0, s1 = s0 + dzl[:, k], s1 + dzl[:, k] * hl[:, k]
    dbeta = grouped(lane_sum(s0).astype(np.float64)).astype(F)
    dgamma = grouped(lane_sum(s1).astype(np.float64)).astype(F)
    inv_n = F(1) / F(n)
    out["dx"] = ga * is_ * dz if mut == "dx_no_mean" else ga * is_ * (dz - dbeta * inv_n - xhat * dgamma * inv_n)
    out["dbeta"], out["dgamma"] = dbeta, dgamma
    assert all(v_.dtype == F for v_ in out.values())
    return out


# ------------------------------------------------------------------------------------------------------------------ the dense model
def fma32(a, b, c_):
    """fmaf for a bf16-valued or float32 `a`, b float32: the product is exact in float64 (at most 48 bits), one float64 rounding of the
    sum precedes the float32 one (it can differ from fmaf only on a 2^-29 sliver next to a float32 midpoint)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c_.astype(np.float64)).astype(F)


def colsum32(partial, first32=False):
    """(rows, ...) float32 -> float64 column sums in dt_colsum32's order: part p adds rows p, p + 32, ...; then the 32 parts"""
    rows = partial.shape[0]
    Rp = -(-rows // 32) * 32
    pad = np.zeros((Rp,) + partial.shape[1:])
    pad[:rows] = partial
    pad = pad.reshape((Rp // 32, 32) + partial.shape[1:])
    acc = np.zeros(pad.shape[1:])
    for i in range(1 if first32 else Rp // 32):
        acc = acc + pad[i]
    t = np.zeros(pad.shape[2:])
    for q in range(32):
        t = t + acc[q]
    return t


def dense_finalize_model(c, mut=None):
    tot = colsum32(c["partial"], first32=mut == "first32")
    count = c["tiles"] * 128 if mut == "count_tiles" else c["count"]
    mom, eps = float(F(c["momentum"])), float(F(c["eps"]))
    mu = tot[0] / count
    var = np.maximum(tot[1] / count - mu * mu, 0.0)
    unb = var * count / (count - 1) if count > 1 else var
    return dict(mean=mu.astype(F), invstd=(1.0 / np.sqrt(var + eps)).astype(F),
                running_mean=((1.0 - mom) * c["r_mean"].astype(np.float64) + mom * mu).astype(F),
                running_var=((1.0 - mom) * c["r_var"].astype(np.float64) + mom * unb).astype(F))


def dense_fold(c):
    sc = c["invstd"] * c["gamma"]
    return sc, c["beta"] - c["mean"] * sc


def dense_apply_model(c, mut=None):
    sc, sh = dense_fold(c)
    v = fma32(c["x"], sc, sh)
    y = cases.bf16_round(np.maximum(v, F(0)) if c["relu"] else v)
    if mut == "apply_no_stride":
        y[ref.DT_APPLY_BLOCKS * ref.DT_ROWS:] = 0
    return dict(v=v, y=y)


def dense_bwd_model(c, mut=None):
    x, dy, M = c["x"], c["dy"], c["M"]
    geo = ref.dense_geometry(M)
    blocks, J = geo["blocks"], geo["sweeps"]
    mu, is_, ga, be = c["mean"], c["invstd"], c["gamma"], c["beta"]
    sc, sh = dense_fold(c)
    xh = (x - mu) * is_
    keep = fma32(xh, ga, be) > 0 if mut == "old_mask" else fma32(x, sc, sh) > 0
    g = np.where(keep, dy, F(0)) if c["relu"] else dy

    def sweeps(a):  # pixel m = (j * blocks + block) * 16 + rg
        pad = np.zeros((J * blocks * 16, ref.DT_C), F)
        pad[:M] = a
        return pad.reshape(J, blocks, 16, ref.DT_C)

    gl, hl = sweeps(g), sweeps(xh)
    s1, s2 = np.zeros((blocks, 16, ref.DT_C), F), np.zeros((blocks, 16, ref.DT_C), F)
    for j in range(1 if mut == "reduce_no_stride" else J):
        s1, s2 = s1 + gl[j], fma32(gl[j], hl[j], s2)
    p1, p2 = np.zeros((blocks, ref.DT_C), F), np.zeros((blocks, ref.DT_C), F)
    for rg in range(16):
        p1, p2 = p1 + s1[:, rg], p2 + s2[:, rg]
    dbeta, dgamma = colsum32(p1).astype(F), colsum32(p2).astype(F)
    inv_m = F(1) / F(-(-M // 16) * 16 if mut == "wrong_M" else M)
    k0, k1 = dbeta * inv_m, dgamma * inv_m
    return dict(dx=cases.bf16_round(ga * is_ * (g - k0 - xh * k1)), dbeta=dbeta, dgamma=dgamma, mask=keep)


# the sparse running pair; all four outputs of the dense finalize; the dense kernels' bf16 outputs ("y_bf16", "dx_bf16")
FEW_ROUNDINGS = ("running_mean", "running_var", "mean", "invstd", "y_bf16", "dx_bf16")


def worst(fr):
    """the largest fraction of a bar, those of FEW_ROUNDINGS halved.  Half a bar is the rule for every output whose bar is a chain bound
    (tens of roundings: a model in the kernel's own order sits far inside).  The sparse running update is FOUR roundings on top of a
    statistic that carries next to nothing of its bar times a momentum of 0.01, and the dense finalize is float64 up to ONE cast: such a
    bar is attained, not approached -- three aligned half-ulps of r' exceed half of 3 u |r'| in one channel out of seven just above a
    power of two (P(|U1 + U2 + U3| > 1.5) = 0.14; observed at once: 0.51 on unroll-c64-n15), a single cast reaches u |r'| itself, and
    a bf16 output's bar is its one final rounding, half a bf16 ulp, which a value next to a midpoint uses up entirely.  No term is
    missing there and none may be invented: these outputs are held to their whole bar."""
    return max(v / 2 if k in FEW_ROUNDINGS else v for k, v in fr.items())


def broken(fr):
    return max(fr.values()) > 1


# ------------------------------------------------------------------------------------------------------------------ bn_ref is torch's
TORCH_SPARSE = ["unroll-c16-n65", "chunks-c128-n513", "kind-sorted-n5000", "kind-gamma_mixed-n513", "kind-no_relu-n5000", "book-mom_1",
                "kind-offset_1e2-n513"]


@pytest.mark.parametrize("name", TORCH_SPARSE)
def test_the_reference_is_torch_batchnorm1d_in_float64(name):
    c = cases.sparse_case(name)
    fw, _ = cases.sparse_reference(name)
    bn = torch.nn.BatchNorm1d(c["C"], eps=float(F(c["eps"])), momentum=float(F(c["momentum"]))).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(c["gamma"].astype(np.float64)))
        bn.bias.copy_(torch.from_numpy(c["beta"].astype(np.float64)))
        bn.running_mean.copy_(torch.from_numpy(c["r_mean"].astype(np.float64)))
        bn.running_var.copy_(torch.from_numpy(c["r_var"].astype(np.float64)))
    xt = torch.from_numpy(c["x"].astype(np.float64)).requires_grad_(True)
    y = bn(xt)
    y = torch.relu(y) if c["relu"] else y
    y.backward(torch.from_numpy(c["dy"].astype(np.float64)))
    scale = np.abs(fw["v"]).max()
    np.testing.assert_allclose(y.detach().numpy(), fw["y"], rtol=0, atol=1e-11 * scale)
    np.testing.assert_allclose(bn.running_mean.numpy(), fw["running_mean"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(bn.running_var.numpy(), fw["running_var"], rtol=1e-12, atol=1e-13)
    bw = ref.bn_backward(c["x"], c["dy"], fw["mean"], fw["invstd"], c["gamma"], c["beta"], c["relu"])
    assert np.array_equal(bw["v"] > 0, y.detach().numpy() > 0) or not c["relu"]
    for got, want in ((xt.grad, bw["dx"]), (bn.weight.grad, bw["dgamma"]), (bn.bias.grad, bw["dbeta"])):
        np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=1e-10 * max(np.abs(want).max(), 1.0))


@pytest.mark.parametrize("run", [(432, 1, "iid"), (17, 0, "iid"), (cases.KIND_M, 1, "gamma_mixed")], ids=cases.run_id)
def test_the_reference_is_torch_batchnorm2d_in_float64(run):
    c = cases.bwd_case(*run)
    M = c["M"]
    fw = ref.bn_forward(c["x"], c["gamma"], c["beta"], cases.EPS, c["relu"])
    bn = torch.nn.BatchNorm2d(128, eps=float(F(cases.EPS))).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(c["gamma"].astype(np.float64)))
        bn.bias.copy_(torch.from_numpy(c["beta"].astype(np.float64)))
    xt = torch.from_numpy(c["x"].astype(np.float64).reshape(1, M, 1, 128)).permute(0, 3, 1, 2).requires_grad_(True)
    y = bn(xt)
    y = torch.relu(y) if c["relu"] else y
    y.backward(torch.from_numpy(c["dy"].astype(np.float64).reshape(1, M, 1, 128)).permute(0, 3, 1, 2))
    back = lambda t: t.detach().permute(0, 2, 3, 1).reshape(M, 128).numpy()
    np.testing.assert_allclose(back(y), fw["y"], rtol=0, atol=1e-11 * np.abs(fw["v"]).max())
    bw = ref.bn_backward(c["x"], c["dy"], fw["mean"], fw["invstd"], c["gamma"], c["beta"], c["relu"])
    for got, want in ((back(xt.grad), bw["dx"]), (bn.weight.grad.numpy(), bw["dgamma"]), (bn.bias.grad.numpy(), bw["dbeta"])):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-10 * max(np.abs(want).max(), 1.0))
    new_mean, new_var = ref.bn_running(np.zeros(128), np.ones(128), fw["mean"], fw["var_unbiased"], 0.1)
    np.testing.assert_allclose(bn.running_mean.numpy(), new_mean, rtol=1e-7, atol=1e-9)  # momentum: the float32 0.1 on our side
    np.testing.assert_allclose(bn.running_var.numpy(), new_var, rtol=1e-7, atol=1e-9)
    # dense_finalize on exact float64 "partials" is the same statistics
    x64 = c["x"].astype(np.float64)
    fin = ref.dense_finalize(np.stack([x64.sum(0), (x64 * x64).sum(0)])[None], M, cases.EPS)
    np.testing.assert_allclose(fin["mean"], fw["mean"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(fin["var_unbiased"], fw["var_unbiased"], rtol=1e-9)


def test_one_row_by_hand():
    c = cases.sparse_case("one_row")
    fw, _ = cases.sparse_reference("one_row")
    assert (fw["var"] == 0).all() and (fw["var_unbiased"] == 0).all() and (fw["xhat"] == 0).all()
    assert np.array_equal(fw["y"][0], np.maximum(c["beta"].astype(np.float64), 0))
    bw = ref.bn_backward(c["x"], c["dy"], fw["mean"], fw["invstd"], c["gamma"], c["beta"], 1)
    assert (bw["dx"] == 0).all() and (bw["dgamma"] == 0).all()
    m = sparse_model(c)
    assert np.array_equal(m["y"][0], np.maximum(c["beta"], 0)) and (m["dx"] == 0).all() and (m["var_unbiased"] == 0).all()
    assert np.array_equal(m["save_mean"], c["x"][0]) and np.array_equal(m["save_invstd"], F(1) / np.sqrt(np.zeros(16, F) + F(1e-3)))


# ------------------------------------------------------------------------------------------------------------------ well-posed; the model
@pytest.mark.parametrize("name", cases.SPARSE_IDS)
def test_a_sparse_case_is_what_it_is_named_for_and_the_model_keeps_half_the_bars(name):
    c = cases.sparse_case(name)
    fw, bars = cases.sparse_reference(name)
    n, C, kind = c["n"], c["C"], c["kind"]
    geo = ref.sbn_geometry(n, C)
    assert geo["counts"].sum() == n and (np.diff(geo["counts"]) <= 0).all()
    if n in cases.GEOMETRY:
        assert (geo["G"], geo["rows"], geo["empty"]) == cases.GEOMETRY[n], (geo["G"], geo["rows"], geo["empty"])
    else:
        assert geo["G"] == 1 and geo["rows"] == n and geo["empty"] == 0
    family = name.split("-")[0]
    if family == "unroll":
        lane_rows = -(-n // geo["RL"])  # of lane 0
        if C in cases.SMALL_C:
            assert lane_rows < 4, "no unrolled statistics trip at this width"
        else:
            assert n in cases.unroll_sizes(C)
    if family == "cap":
        assert geo["G"] == 512 and geo["empty"] == (1 if n > 131072 else 0) and (geo["counts"][-1] == 0) == (n > 131072)
    if family == "merge":
        assert {4: {65280: 255, 65536: 256, 65537: 257}, 256: {768: 3, 1024: 4, 1025: 5}}[C][n] == geo["G"] and geo["Q"] == 1024 // C
    x = c["x"].astype(np.float64)
    std = np.sqrt(fw["var"])
    # the share of the variance that lies BETWEEN the chunks
    pad = np.full((geo["G"] * geo["rows"], C), np.nan)
    pad[:n] = x
    with np.errstate(invalid="ignore"), np.testing.suppress_warnings() as sup:
        sup.filter(RuntimeWarning)
        mb = np.nanmean(pad.reshape(geo["G"], geo["rows"], C), 1)
    between = np.nansum(geo["counts"][:, None] * (mb - fw["mean"]) ** 2, 0) / n / np.maximum(fw["var"], 1e-300)
    if kind == "sorted":
        assert between.min() > (0.95 if geo["G"] >= 20 else 0.7), between.min()  # three chunks of a sorted normal sample: 0.79
    elif kind == "iid" and geo["G"] > 1 and n >= 5000:
        assert between.max() < 0.05
    if kind.startswith("offset"):
        want = float(kind.split("_")[1])
        assert ((np.abs(fw["mean"]) / std > 0.8 * want) & (np.abs(fw["mean"]) / std < 1.25 * want)).all()
    if kind == "constant":
        assert fw["var"][C // 3] == 0 and (np.delete(fw["var"], C // 3) > 0.1).all()
    if kind == "outlier":
        assert ((x[n // 2] - np.delete(x, n // 2, 0).mean(0)) / np.delete(x, n // 2, 0).std(0) > 0.9e4).all()
    if kind == "gamma_mixed":
        assert (c["gamma"] > 0).any() and (c["gamma"] < 0).any() and (c["gamma"] == 0).sum() >= C // 5
    if kind == "tie":
        assert (np.abs(fw["v"]) <= bars["v"]).mean() >= 0.25, "a quarter of the rows sit on the ReLU's edge"
        assert ((x == x[0]).all(1)).sum() == n // 4 + 1
    else:
        share = float(fw["near"].mean())
        assert share <= NEAR_SHARE, f"{share:.2%} of the pre-activations lie within their bar of 0: choose another seed"
    if c["relu"] and n > 1 and kind not in ("tie",):
        assert 0.2 < (fw["v"] > 0).mean() < 0.8, "both sides of the ReLU are populated"
    # the fp32 model of the kernels
    got = sparse_model(c)
    fr = sparse_fractions(name, got)
    print(f"{name}: model, in units of the bars: " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()))
    assert worst(fr) <= HALF, fr
    if kind != "tie":
        fr64 = sparse_float64_mask_fractions(name, got)
        assert worst(fr64) <= HALF, fr64


SPARSE_MUTATIONS = [
    ("no_between", ["kind-sorted-n5000", "kind-sorted-n513"]),
    ("e2_fp32", ["kind-offset_1e4-n5000", "kind-offset_1e4-n513"]),
    ("swap_var", ["unroll-c4-n2", "unroll-c4-n3", "unroll-c8-n2", "unroll-c8-n3"]),
    ("last_full", ["chunks-c16-n257", "chunks-c16-n511", "chunks-c128-n257", "chunks-c128-n511"]),  # 513 = 3 x 171: no short chunk
    ("skip_tail", ["unroll-c64-n65", "unroll-c256-n17", "unroll-c16-n129", "unroll-c64-n33", "unroll-c256-n9"]),  # 4 RL + 1, 2 RL + 1
    ("empty_counted", ["cap-c4-n131073", "cap-c16-n131073", "cap-c4-n140000", "cap-c16-n140000"]),
    ("mask_xhat", ["kind-iid-n5000", "kind-iid-n513", "chunks-c16-n1025"]),
    ("dgamma_x", ["kind-iid-n5000", "kind-offset_1e2-n513"]),
    ("dx_no_mean", ["kind-iid-n5000", "kind-iid-n513"]),
    ("mom_rev", ["book-mom_1", "book-mom_0"]),
]


@pytest.mark.parametrize("mut,names", SPARSE_MUTATIONS, ids=[m for m, _ in SPARSE_MUTATIONS])
def test_a_mistake_in_the_sparse_model_breaks_a_bar(mut, names):
    for name in names:
        fr = sparse_fractions(name, sparse_model(cases.sparse_case(name), mut=mut))
        broken = {k: round(v, 1) for k, v in fr.items() if v > 1}
        print(f"{mut} on {name}: {broken}")
        assert broken, (mut, name, fr)


def test_the_cap_mistake_is_invisible_below_the_cap_and_the_tail_one_at_a_multiple():
    """the counterparts: what the named cases add over their neighbours"""
    assert worst(sparse_fractions("cap-c16-n131072", sparse_model(cases.sparse_case("cap-c16-n131072"), mut="empty_counted"))) <= HALF
    assert worst(sparse_fractions("chunks-c16-n512", sparse_model(cases.sparse_case("chunks-c16-n512"), mut="last_full"))) <= HALF
    assert worst(sparse_fractions("chunks-c16-n513", sparse_model(cases.sparse_case("chunks-c16-n513"), mut="last_full"))) <= HALF  # 3 x 171
    assert worst(sparse_fractions("unroll-c64-n64", sparse_model(cases.sparse_case("unroll-c64-n64"), mut="skip_tail"))) <= HALF


# ------------------------------------------------------------------------------------------------------------------ dense
@pytest.mark.parametrize("run", cases.FINALIZE_RUNS, ids=cases.run_id)
def test_a_finalize_run_and_its_model(run):
    c = cases.finalize_case(*run)
    tiles, kind, below = run
    assert c["partial"].shape == (tiles, 2, 128) and c["partial"].dtype == F
    assert c["count"] == {"full": tiles * 128, "below": tiles * 128 - 77, "one": 1}[below] and (tiles - 1) * 128 < c["count"] or below == "one"
    if kind == "offset":
        ratio = np.abs(c["true_mean"]) / np.sqrt(c["true_var"])  # 128 pixels a tile, bf16 steps of 0.5 - 1 at 100 - 200: roughly 100
        assert ((ratio > 50) & (ratio < 200)).all()
    fin = ref.dense_finalize(c["partial"], c["count"], c["eps"])
    if below != "one":  # what the input has lost already: reported, not asserted (it is the convolution's epilogue that forms these sums)
        loss = np.abs(fin["var"] - c["true_var"]) / c["true_var"]
        print(f"finalize {cases.run_id(run)}: E[x^2] - mean^2 from the fp32 partials against the pixels' float64 variance: "
              f"largest relative difference {loss.max():.3e}, median {np.median(loss):.3e}")
    else:
        assert (fin["var"] == 0).all() and (fin["var_unbiased"] == 0).all()
    fr = dense_finalize_fractions(c, dense_finalize_model(c))
    assert worst(fr) <= HALF, fr
    if below == "below":
        assert broken(dense_finalize_fractions(c, dense_finalize_model(c, mut="count_tiles")))
    if tiles >= 33:
        assert broken(dense_finalize_fractions(c, dense_finalize_model(c, mut="first32")))
    else:
        assert worst(dense_finalize_fractions(c, dense_finalize_model(c, mut="first32"))) <= HALF


def apply_fractions(c, y):
    return ref.in_bars(y, c["y"], c["bar_y"])


@pytest.mark.parametrize("run", cases.APPLY_RUNS, ids=cases.run_id)
def test_an_apply_run_and_its_model(run):
    c = cases.apply_case(*run)
    M = c["M"]
    geo = ref.dense_geometry(M)
    assert geo["apply_blocks"] == min(-(-M // 16), 4096) and (M > 65536) == (-(-M // 16) > 4096)
    near = ref.near_zero(c["v"], c["bar_v"])
    assert near.mean() <= NEAR_SHARE
    m = dense_apply_model(c)
    assert apply_fractions(c, m["y"]) <= 1, "one bf16 rounding: the whole bar (see `worst`)"
    assert ref.in_bars(m["v"], c["v"], c["bar_v"]) <= 1  # four roundings: the whole bar
    if c["relu"]:
        assert np.array_equal((m["y"] > 0)[~near], (c["v"] > 0)[~near])
    stale = apply_fractions(c, dense_apply_model(c, mut="apply_no_stride")["y"])
    assert (stale > 1) == (M > 65536), "only the run past 4096 blocks notices a missing stride"


@pytest.mark.parametrize("run", cases.BWD_RUNS, ids=cases.run_id)
def test_a_backward_run_and_its_model(run):
    c = cases.bwd_case(*run)
    M, relu, kind = run
    geo = ref.dense_geometry(M)
    assert geo["blocks"] == min(-(-M // 16), 512) and (geo["sweeps"] > 1) == (M > 8192)
    if kind == "tie":
        assert c["near"].mean() >= 0.25
    else:
        assert c["near"].mean() <= NEAR_SHARE, f"{c['near'].mean():.2%} near zero: choose another seed"
    if kind == "offset_1e2":
        x = c["x"].astype(np.float64)
        assert ((np.abs(x.mean(0)) / x.std(0) > 50) & (np.abs(x.mean(0)) / x.std(0) < 200)).all()
    y = dense_apply_model(c)["y"]
    m = dense_bwd_model(c)
    assert np.array_equal(m["mask"], y > 0) or not relu, "the backward's mask is the stored output's"
    fr = dense_bwd_fractions(c, m, y)
    print(f"bwd {cases.run_id(run)}: model, in units of the bars: {fr}")
    assert worst(fr) <= HALF, fr
    if kind != "tie":  # against the float64 mask, the near-zero elements left out
        near = c["near"]
        bw = ref.bn_backward(c["x"], c["dy"], c["mean"], c["invstd"], c["gamma"], c["beta"], relu)
        bb = ref.backward_bars(bw, c["gamma"], c["invstd"], geo["k_bwd"], bf16=True, near=near, dy=c["dy"])
        assert ref.in_bars(m["dx"][~near], bw["dx"][~near], bb["dx"][~near]) <= 1
        assert ref.in_bars(m["dbeta"], bw["dbeta"], bb["dbeta"]) <= HALF and ref.in_bars(m["dgamma"], bw["dgamma"], bb["dgamma"]) <= HALF
        if relu:
            assert np.array_equal(m["mask"][~near], bw["mask"][~near])
    else:
        old = dense_bwd_model(c, mut="old_mask")
        tied = (c["x"] == c["x"][0]).all(1)
        differ = old["mask"] != (y > 0)
        print(f"bwd {cases.run_id(run)}: fmaf(xhat, gamma, beta) > 0 differs from y > 0 on {int(differ.sum())} of {int(tied.sum()) * 128} tie elements "
              f"({int(differ[~tied].sum())} elsewhere)")
        assert differ.sum() > 1000, "the tie kind separates the two expressions"
        assert broken(dense_bwd_fractions(c, old, y)), "and the former mask misses the bars"
    # the mistakes
    no_stride = broken(dense_bwd_fractions(c, dense_bwd_model(c, mut="reduce_no_stride"), y))
    assert no_stride == (M > 8192), "a reduction without its stride is noticed from 8193 pixels on, and only there"
    if M in (15, 17):
        assert broken(dense_bwd_fractions(c, dense_bwd_model(c, mut="wrong_M"), y))
    if M == 16:
        assert worst(dense_bwd_fractions(c, dense_bwd_model(c, mut="wrong_M"), y)) <= HALF

"""Training-mode BatchNorm (+ ReLU), forward and backward, restated in float64 numpy, with the error bar of every output of the two HIP
implementations: csrc/sparse_bn.hip (fp32 rows (n, C)) and the dt_bn_* kernels of csrc/dense_train.hip (bf16 NHWC, 128 channels).
Reads nothing from vision3d_amd.

  bn_forward   mean, biased and unbiased variance, invstd = 1 / sqrt(var + eps), xhat, the pre-activation v = xhat gamma + beta, y.
  bn_running   r <- (1 - momentum) r + momentum * statistic, momentum read as the float32 the C ABI receives.
  bn_backward  dz = dy [v > 0];  dbeta = sum dz;  dgamma = sum dz xhat;  dx = gamma invstd (dz - dbeta / n - xhat dgamma / n).  mean and
               invstd are INPUTS: both backward entries and the dense apply are pure functions of the float32 mean / invstd they are
               handed, so the yardstick is float64 arithmetic on those same float32 values.  `mask` replaces [v > 0]: the mask the
               forward under test produced (y > 0).
  dense_finalize  mean / variance / invstd from (tiles, 2, 128) float32 partial sums, in float64 ON THOSE PARTIALS: what E[x^2] - mean^2
               loses when it is formed from float32 partials is a property of the input, not of the kernel that adds them.

THE BARS.  u = 2^-24.  A sum of float32 terms t_i whose longest chain of additions has k links is off by at most k u sum|t_i| (first order;
k u < 2e-5 here).  The library is compiled without contraction, so every operator of the source rounds once; fmaf rounds once.  Every bar
is evaluated on the case's own float64 magnitudes; none is tuned.  The one final rounding of a bf16 output costs half a bf16 ulp of the
value's binade, h(r) = 2^-8 2^floor(log2 |r|): between 2^-9 |r| (top of the binade) and 2^-8 |r| (bottom).  2^-9 |r| itself is NOT a bound
for round-to-nearest: r = 1 + 2^-8 lies midway between the bf16 neighbours 1 and 1 + 2^-7, and either is 2^-8 away.

sparse_bn.hip, forward.  A workgroup owns a chunk of n_b rows; a thread (row lane, channel quad) adds its rows four at a time,
s += (a + b) + (c + d), then one at a time; the RL = 1024 / C lanes are added in lane order; one division.  Longest chain:
K = 2 + ceil(rows / RL) + RL + 1 (sbn_geometry: k_stats).  So the chunk mean m~_b is off by at most
    d_b = K u sum_b|x| / n_b                                                                  (K u times the chunk's mean |x|)
and NOTHING in fp32 can do better than u |x|: the forward multiplies that by invstd, so every sparse forward bar grows with |mean| / std.
The merge is float64 (its own rounding, ~G 2^-53, is far below u and is covered by the "+ u" cast terms):
    save_mean      D + u |mean|,                       D = sum_b n_b d_b / n = K u mean|x|
The second pass sums (x - m~_b)^2 about the COMPUTED chunk mean and the merge treats m~_b as the chunk's mean.  With e_b = m~_b - m_b and
mu~ = sum n_b m~_b / n, expanding about mu~ gives exactly
    M2~ = M2 + n (mu~ - mu)^2 - 2 sum_b n_b e_b (m~_b - mu~),        |m~_b - mu~| <= |m_b - mu| + d_b + D,
and the fp32 evaluation of sum_b sum_i (x_i - m~_b)^2 (= within-chunk M2 + sum n_b e_b^2; a term carries 3 u: one subtraction squared, one
product; the chain K - 1 links) adds (K + 3) u of it.  Hence
    var (biased)   B = D^2 + 2 sum_b n_b d_b (|m_b - mu| + d_b + D) / n + (K + 3) u (var + sum_b n_b d_b^2 / n) + u var
    var_unbiased   B n / (n - 1)
    save_invstd    invstd (r / (2 (1 - r)) + 4 u),  r = B / (var + eps)      (one addition, sqrtf, one division; 4 u covers a 1-ulp sqrtf)
    y, and v       |gamma| (invstd bar(mean) + |x - mean| bar(invstd)) + u (4 |xhat gamma| + |beta|)         (sub, mul, mul, add)
    running pair   |momentum| bar(statistic) + u (3 |(1 - momentum) r| + 2 |momentum statistic|)
The first term of B is why a sorted input (chunk means far apart) and a large |mean| / std are the hard cases, and why a kernel that
dropped n_b (m_b - mu)^2 or formed E[x^2] - mean^2 in fp32 lands far outside it.

sparse_bn.hip, backward.  A thread adds its rows in order (two per trip, the sums still sequential), lanes in order, chunks in float64:
chain Kb = ceil(rows / RL) + RL + 1 (k_bwd).  xhat = (x - mean) invstd carries 2 u, the product dz xhat one more:
    dbeta          Kb u sum|dz|
    dgamma         (Kb + 3) u sum|dz xhat|
    dx             |gamma invstd| [ (bar(dbeta) + |xhat| bar(dgamma)) / n + u (4 |dz| + 6 |dbeta| / n + 8 |xhat dgamma| / n) ]
(1 / n rounds once; dbeta / n: 2 u; xhat dgamma / n: 5 u; two subtractions and two products of the bracket: 4 u of |dz| + |..| + |..|.)
With mask = (y_gpu > 0) nothing is left out: forward and backward evaluate ONE fp32 expression.  Against the float64 mask (mask=None)
the elements whose float64 v lies within bar(v) of 0 may fall either way: they are left out of the dx comparison and their |dy| and
|dy xhat| are added to the dbeta / dgamma bars (`near`).

dense_train.hip.  finalize: float64 sums of the partials in a fixed order (chain ceil(tiles / 32) + 32), so against float64 on the same
partials only the cast to float32 and 2^-53-sized terms remain; they matter for the variance alone, where E[x^2] - mean^2 cancels:
    mean u |mean| + s;  invstd: invstd (u + V / (var + eps));  running pair: u |r'| + |momentum| (s or V n / (n - 1))
with s = 2 kd 2^-53 sum|partial_0| / count, V = 2 kd 2^-53 sum|partial_1| / count + 2 |mean| s + 4 2^-53 mean^2, kd = ceil(tiles / 32) + 36.
apply: sc = invstd gamma, sh = beta - mean sc, v = fmaf(x, sc, sh), one rounding to bf16:
    v              u (|x sc| + 3 |mean sc| + |beta| + |v|)       -- the folded shift: it grows with |mean invstd gamma| + |beta|
    y              bar(v) + h(|y| + bar(v))
backward: a thread adds its pixel of every sweep of the grid (ceil(M / (blocks 16)) sweeps), the 16 pixel rows of a block in order, the
blocks in float64: chain Kd = sweeps + 16 + 1; the rest as for the sparse kernels, then one rounding of dx to bf16:
    dbeta Kd u sum|dz|;  dgamma (Kd + 3) u sum|dz xhat|;  dx: the sparse bracket + h(|dx| + that).
"""
import numpy as np

U = 2.0 ** -24
D64 = 2.0 ** -53
SBN_MIN_ROWS, SBN_MAX_CHUNKS, SBN_THREADS = 256, 512, 1024  # rows per chunk at least; chunks at most; RL * C = Q * C
DT_C, DT_RED_BLOCKS, DT_APPLY_BLOCKS, DT_ROWS = 128, 512, 4096, 16  # dense: channels, grids of the reduction / the apply, pixels a block


def f64(a):
    return np.asarray(a, np.float64)


def bf16_half_ulp(a):
    """half a bf16 ulp (8 significant bits) of the binade of |a|; 0 at 0"""
    a = np.abs(f64(a))
    with np.errstate(divide="ignore"):
        return np.where(a > 0, 2.0 ** -8 * 2.0 ** np.floor(np.log2(np.where(a > 0, a, 1.0))), 0.0)


def sbn_geometry(n, C):
    """the chunking every sparse kernel derives from n: G chunks of `rows` rows (the last live one shorter, the rest empty)"""
    G = min(max(-(-n // SBN_MIN_ROWS), 1), SBN_MAX_CHUNKS)
    rows, RL = -(-n // G), SBN_THREADS // C
    counts = np.clip(n - np.arange(G) * rows, 0, rows)
    trips = -(-rows // RL)
    return dict(G=G, rows=rows, RL=RL, Q=SBN_THREADS // C, counts=counts, empty=int((counts == 0).sum()), k_stats=3 + trips + RL,
                k_bwd=1 + trips + RL)


def dense_geometry(M):
    blocks = min(-(-M // DT_ROWS), DT_RED_BLOCKS)
    sweeps = -(-M // (blocks * DT_ROWS))
    return dict(blocks=blocks, sweeps=sweeps, apply_blocks=min(-(-M // DT_ROWS), DT_APPLY_BLOCKS), k_bwd=sweeps + DT_ROWS + 1)


# ------------------------------------------------------------------------------------------------------------------ the statement
def bn_forward(x, gamma, beta, eps, relu):
    x, gamma, beta, eps = f64(x), f64(gamma), f64(beta), float(np.float32(eps))
    n = x.shape[0]
    mean = x.mean(0)
    d = x - mean
    var = (d * d).mean(0)
    var_unbiased = var * n / (n - 1) if n > 1 else var.copy()
    invstd = 1.0 / np.sqrt(var + eps)
    xhat = d * invstd
    v = xhat * gamma + beta
    return dict(mean=mean, var=var, var_unbiased=var_unbiased, invstd=invstd, xhat=xhat, v=v, y=np.maximum(v, 0.0) if relu else v)


def bn_running(r_mean, r_var, mean, var_unbiased, momentum):
    m = float(np.float32(momentum))
    return (1.0 - m) * f64(r_mean) + m * f64(mean), (1.0 - m) * f64(r_var) + m * f64(var_unbiased)


def bn_backward(x, dy, mean, invstd, gamma, beta, relu, mask=None):
    x, dy, mean, invstd, gamma, beta = f64(x), f64(dy), f64(mean), f64(invstd), f64(gamma), f64(beta)
    n = x.shape[0]
    xhat = (x - mean) * invstd
    v = xhat * gamma + beta
    if mask is None:
        mask = v > 0 if relu else np.ones(x.shape, bool)
    dz = np.where(mask, dy, 0.0)
    dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
    dx = gamma * invstd * (dz - dbeta / n - xhat * dgamma / n)
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, xhat=xhat, v=v, dz=dz, mask=mask, n=n)


def dense_finalize(partial, count, eps):
    p, eps = f64(partial), float(np.float32(eps))
    tot = p.sum(0)
    mean = tot[0] / count
    var = np.maximum(tot[1] / count - mean * mean, 0.0)
    var_unbiased = var * count / (count - 1) if count > 1 else var.copy()
    return dict(mean=mean, var=var, var_unbiased=var_unbiased, invstd=1.0 / np.sqrt(var + eps))


# ------------------------------------------------------------------------------------------------------------------ the bars
def sparse_forward_bars(x, gamma, beta, eps, fw):
    """bars of save_mean, var, var_unbiased, save_invstd and v (= y's) for sbn_stats / sbn_merge / sbn_apply; fw = bn_forward(...)"""
    x, gamma, beta, eps = f64(x), f64(gamma), f64(beta), float(np.float32(eps))
    n, C = x.shape
    geo = sbn_geometry(n, C)
    G, rows, K = geo["G"], geo["rows"], geo["k_stats"]
    pad = np.zeros((G * rows, C))
    pad[:n] = x
    pad = pad.reshape(G, rows, C)
    nb = geo["counts"][:, None].astype(np.float64)
    nb1 = np.maximum(nb, 1.0)
    mb = pad.sum(1) / nb1
    db = K * U * np.abs(pad).sum(1) / nb1  # 0 for an empty chunk
    D = (nb * db).sum(0) / n
    mean, var = fw["mean"], fw["var"]
    b_mean = D + U * np.abs(mean)
    b_var = (D * D + 2.0 * (nb * db * (np.abs(mb - mean) + db + D)).sum(0) / n + (K + 3) * U * (var + (nb * db * db).sum(0) / n) + U * var)
    r = b_var / (var + eps)
    assert (r < 0.5).all(), "the variance bar is no small perturbation: the case is beyond fp32"
    b_invstd = fw["invstd"] * (r / (2.0 * (1.0 - r)) + 4 * U)
    b_v = np.abs(gamma) * (fw["invstd"] * b_mean + np.abs(x - mean) * b_invstd) + U * (4 * np.abs(fw["xhat"] * gamma) + np.abs(beta))
    return dict(mean=b_mean, var=b_var, var_unbiased=b_var * (n / (n - 1.0) if n > 1 else 1.0), invstd=b_invstd, v=b_v, y=b_v)


def running_bar(r, stat, bar_stat, momentum):
    """fp32 r' = (1.f - momentum) * r + momentum * stat, of a statistic known to bar_stat"""
    m = float(np.float32(momentum))
    return abs(m) * f64(bar_stat) + U * (3 * np.abs((1.0 - m) * f64(r)) + 2 * np.abs(m * f64(stat)))


def backward_bars(bw, gamma, invstd, k_sum, bf16=False, near=None, dy=None):
    """bars of dbeta, dgamma, dx for a two-level sum whose longest chain has k_sum links; `near` (bool mask): the elements left to either
    side of the ReLU -- their |dy| and |dy xhat| join the bars of the sums"""
    gamma, invstd, n = f64(gamma), f64(invstd), bw["n"]
    xhat, dz = bw["xhat"], bw["dz"]
    b_dbeta = k_sum * U * np.abs(dz).sum(0)
    b_dgamma = (k_sum + 3) * U * np.abs(dz * xhat).sum(0)
    if near is not None:
        stray = np.where(near, np.abs(f64(dy)), 0.0)
        b_dbeta = b_dbeta + stray.sum(0)
        b_dgamma = b_dgamma + (stray * np.abs(xhat)).sum(0)
    b_dx = np.abs(gamma * invstd) * ((b_dbeta + np.abs(xhat) * b_dgamma) / n
                                     + U * (4 * np.abs(dz) + 6 * np.abs(bw["dbeta"]) / n + 8 * np.abs(xhat * bw["dgamma"]) / n))
    if bf16:
        b_dx = b_dx + bf16_half_ulp(np.abs(bw["dx"]) + b_dx)
    return dict(dbeta=b_dbeta, dgamma=b_dgamma, dx=b_dx)


def dense_finalize_bars(partial, count, eps, fin, momentum=None, r_mean=None, r_var=None):
    p, eps = f64(partial), float(np.float32(eps))
    kd = -(-p.shape[0] // 32) + 36
    s = 2 * kd * D64 * np.abs(p[:, 0]).sum(0) / count
    V = 2 * kd * D64 * np.abs(p[:, 1]).sum(0) / count + 2 * np.abs(fin["mean"]) * s + 4 * D64 * fin["mean"] ** 2
    out = dict(mean=U * np.abs(fin["mean"]) + s, invstd=fin["invstd"] * (U + V / (fin["var"] + eps)))
    if momentum is not None:
        m = abs(float(np.float32(momentum)))
        new_mean, new_var = bn_running(r_mean, r_var, fin["mean"], fin["var_unbiased"], momentum)
        out["running_mean"] = U * np.abs(new_mean) + m * s
        out["running_var"] = U * np.abs(new_var) + m * V * (count / (count - 1.0) if count > 1 else 1.0)
    return out


def dense_apply_reference(x, mean, invstd, gamma, beta, relu):
    """float64 on the float32 mean / invstd handed to the kernel -> v, y, bar(v), bar(y)"""
    x, mean, invstd, gamma, beta = f64(x), f64(mean), f64(invstd), f64(gamma), f64(beta)
    v = (x - mean) * invstd * gamma + beta
    y = np.maximum(v, 0.0) if relu else v
    sc = invstd * gamma
    b_v = U * (np.abs(x * sc) + 3 * np.abs(mean * sc) + np.abs(beta) + np.abs(v))
    return dict(v=v, y=y, bar_v=b_v, bar_y=b_v + bf16_half_ulp(np.abs(y) + b_v))


# ------------------------------------------------------------------------------------------------------------------ comparing
def in_bars(got, want, bar):
    """the largest |got - want| in units of the bar (0 where both are equal, inf where a zero bar is missed)"""
    err, bar = np.abs(f64(got) - f64(want)), np.broadcast_to(f64(bar), np.shape(want))
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bar)
    return float(np.nanmax(np.where(np.isnan(f64(got) + q), np.inf, q)))


def near_zero(v, bar_v):
    """the elements whose float64 pre-activation lies within its own bar of 0: a correct fp32 forward may put them on either side"""
    return np.abs(v) <= bar_v

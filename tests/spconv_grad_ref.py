"""Float64 statements of the two gradients of the sparse convolution, written from the FORWARD rulebook alone, and the bar the
real-valued weight gradient is held to.  numpy only.

forward      out[o] = sum_k X[nbr[k][o]] @ W[k]                     over the live pairs (i = nbr[k][o] >= 0, o < n)
dw           dW[k]  = sum over the live pairs of column k of X[i]^T dY[o]
dx           dX[i] += dY[o] @ W[k]^T for every live pair: a SCATTER over the forward table.  It never forms a transposed table and never
             reverses the offsets, so it is independent of the two things SparseConvFunction.backward assumes (a submanifold table is its
             own transpose with the offsets reversed; v3d_rulebook_transpose for the strided ones).
tests/test_host_spconv_grad_ref.py shows that both are torch's float64 autograd of the dense F.conv3d.

The bar of a real-valued dW (csrc/spconv.hip, spconv_bwd_weight_tiles + spconv_bwd_weight_reduce_kernel).  One element dW[k][ci][co] is a
sum of products x_i dy_o, one per live pair of column k.  The kernel adds them in this structure:
  * the n = min(*n_ptr, cap) rows are cut into slabs of R = bw_rows_per_block(n) rows (the multiple of 256 at or above ceil(n / 64), at
    least 256); S = ceil(n / R) <= 64 of them are live;
  * a slab is cut into four sub-slabs of R / 4 rows, one per wave.  A wave adds the products of ITS live pairs into one fp32 accumulator
    (v_mfma_f32_16x16x4_f32, four pairs per instruction in an order the hardware does not promise): a chain of at most P additions, P the
    number of live pairs of that sub-slab in column k, whatever the order inside an instruction, plus ONE rounding for each product (a fused
    product would round less);
  * the four wave accumulators are added in wave order: 3 additions;
  * the S slab partials are added in slab order, starting from 0: S additions.
Every term therefore passes through at most L = max_subslab P + 1 + 3 + S roundings, each of relative size u = 2^-24, and the standard
bound for a sum whose every term sees at most L roundings gives
      |dW_gpu - dW| <= gamma_L * sum |x_i| |dy_o|,     gamma_L = L u / (1 - L u)
per element, with the sum over the live pairs of that element.  L is read off the table (`dw_chain`), not measured.  It does not depend on
how the queue batches the pairs (16 at a time, leftovers moved to the front): batching changes which instruction adds a pair, not how many
additions lie above it.
The bar of a real-valued dX is the project's own: gpu_util.assert_features_close against float64 (the route is bf16x3: floor 1e-4).
"""
import numpy as np

U = 2.0 ** -24
BW_MAX_SPLITS = 64  # csrc/spconv.hip
BW_Q = 128
BW_BATCH = 16       # pairs per consume()


def rows_per_block(n):
    """bw_rows_per_block: rows per slab from the live row count"""
    r = (-(-n // BW_MAX_SPLITS) + 255) & ~255
    return max(r, 256)


def geometry(n):
    """-> dict(R rows per slab, sub rows per wave, slabs live)"""
    R = rows_per_block(n)
    return dict(R=R, sub=R // 4, slabs=-(-n // R))


def dw(nbr, n, X, dY):
    """nbr (K, cap) int32, n live output rows, X (n_in, Cin), dY (>= n, Cout) -> dW (K, Cin, Cout) float64"""
    nbr = np.asarray(nbr)
    X, dY = np.asarray(X, np.float64), np.asarray(dY, np.float64)
    out = np.zeros((nbr.shape[0], X.shape[1], dY.shape[1]))
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k, :n] >= 0)[0]
        out[k] = X[nbr[k, o]].T @ dY[o]
    return out


def dw_abs(nbr, n, X, dY):
    """sum |x_i| |dy_o| over the live pairs, per element"""
    return dw(nbr, n, np.abs(np.asarray(X, np.float64)), np.abs(np.asarray(dY, np.float64)))


def dx(nbr, n, n_in, dY, W):
    """nbr (K, cap) int32 FORWARD table, dY (>= n, Cout), W (K, Cin, Cout) -> dX (n_in, Cin) float64"""
    nbr = np.asarray(nbr)
    dY, W = np.asarray(dY, np.float64), np.asarray(W, np.float64)
    out = np.zeros((n_in, W.shape[1]))
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k, :n] >= 0)[0]
        np.add.at(out, nbr[k, o], dY[o] @ W[k].T)
    return out


def fed_rows(nbr, n, n_in):
    """(n_in,) bool: the input rows that feed at least one output"""
    nbr = np.asarray(nbr)[:, :n]
    fed = np.zeros(n_in, bool)
    fed[nbr[nbr >= 0]] = True
    return fed


def dw_chain(nbr, n):
    """(K,) int: L of the module docstring, per column"""
    nbr = np.asarray(nbr)
    g = geometry(max(n, 1))
    K = nbr.shape[0]
    subs = g["slabs"] * 4
    live = np.zeros((K, subs * g["sub"]), np.int64)
    live[:, :n] = nbr[:, :n] >= 0
    P = live.reshape(K, subs, g["sub"]).sum(2).max(1)
    return P + 1 + 3 + g["slabs"]


def dw_bar(nbr, n, X, dY):
    """(K, Cin, Cout) float64: gamma_L * sum |x_i| |dy_o|"""
    L = dw_chain(nbr, n).astype(np.float64)
    gamma = L * U / (1.0 - L * U)
    return gamma[:, None, None] * dw_abs(nbr, n, X, dY)


def in_bars(got, ref, bar):
    """largest |got - ref| / bar; 0 where both the error and the bar are 0, inf where an error meets a bar of 0"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bar)
    return float(q.max()) if q.size else 0.0

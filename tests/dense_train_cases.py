"""Seeded cases of the dense half of the train step (csrc/dense_train.hip: dt_conv3_kernel, dt_conv_kernel<1>, dt_wgrad_kernel +
dt_wgrad_reduce_kernel, the three dt_head_* kernels), shared by tests/test_host_dense_train_cases.py and
tests/test_gpu_dense_train_edges.py.  numpy operands, no GPU needed; every case names the tile arithmetic it is meant to hit (`*_arith`,
restated here from the launch code and compared with the library on the GPU), and the reference of every case is torch's float64
conv2d / conv_transpose2d and its autograd on the same operands (`*_reference`; `device` = "cpu", or the GPU for the two largest).

Layouts are the kernels': activations (B, H, W, 128) holding bf16-representable float32 values, weights (128, 128, k, k), the head's
maps and their gradient (B, O, H, W).

Three operand kinds.
  "int"     x, dY, feat, dmaps in {-1, 0, 1}, x non-zero on every image border and tile seam (rows / columns 0, 7, 8, 15 mod 16 and the
            image's last); convolution weights in {-1, 0, 1} with 1/16 of them set, so that |y| <= 256 and the bf16 output is exact;
            every other output is an fp32 sum of integers whose absolute values add up to less than 2^24, exact in ANY order.  These
            are conditions (tests/test_host_dense_train_cases.py asserts them), and the GPU result must EQUAL float64.
  "onehot"  (convolution, small shapes) one non-zero pixel at each image corner, at (15, 15) and (16, 16) across the tile seam (value 2
            at the latter) and at the last pixel of the last image, on channels CI and CO; weights tap + 1 on the one pair
            w[CO, CI, tap].  The output spells out tap order, tap flip (data gradient) and channel swap, exactly.
  "real"    standard normal values rounded to bf16 (head weights, bias and dmaps stay fp32: the head kernels take them so), judged
            ELEMENTWISE by the bars below; they watch the arithmetic.
  "x_lo", "dy_lo", "both"  (split weight gradient) planes hi = 16 a with a in {-2, -1, 1, 2} and lo in {-1, 1}, or a zero lo plane for
            the tensor that carries none.  The reference is the float64 value of hi*hi + hi*lo + lo*hi: the exact product of the two
            split tensors MINUS lo*lo.  Every term is a multiple of 16 and at most 1024 + 2 * 32: sums over all pixels, in units of 16,
            stay below 2^24 (asserted), so fp32 is exact in any order, across the three terms too.

Bars of the real-valued cases (u = 2^-24; n = the number of products of one output element; `mag` = the same torch operation on
the operands' absolute values, float64).  Nothing else goes into a bar.
  bf16 output (convolution, the head's dfeat)      half a bf16 ulp of the reference's binade + n u mag
  fp32 output (dW, maps, the head's dW and db)     n u mag: the any-order summation bound (tests/spconv_grad_ref.py dw_bar)
  statistics                                       rows of sums of the ROUNDED outputs the kernel itself wrote: n u sum|terms| with n
                                                   the pixels of the workgroup (the squares of bf16 values are exact in fp32)
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

C = 128
U = 2.0 ** -24
CI, CO = 5, 77  # the one-hot channel pair

CONV_SHAPES = [(1, 1, 1), (1, 1, 4), (1, 3, 3), (1, 15, 15), (1, 16, 16), (1, 16, 17), (1, 17, 16), (1, 17, 17), (3, 17, 33), (1, 1, 4113),
               (1, 17, 2049)]
ONEHOT_SHAPES = CONV_SHAPES[:9]
CONV_ON_DEVICE = [(1, 17, 2049)]  # float64 reference built on the GPU in the GPU tests
WGRAD_SHAPES = [(1, 1, 1), (1, 3, 3), (1, 8, 16), (1, 9, 17), (3, 9, 17), (1, 8, 1008), (1, 8, 1024), (1, 8, 1040), (1, 8, 2064)]
SPLIT_KINDS = ["x_lo", "dy_lo", "both"]
HEAD_O = [8, 16, 24, 32, 48, 64]
HEAD_M = [1, 63, 64, 65, 255, 256, 257]
# (O, B, H, W).  M = B H W.  The small ones: every M of HEAD_M as ONE image (the total is M) and as B = 2 images of M pixels (odd M: the
# image boundary inside a 64-pixel chunk and a 256-pixel block).  65 601 = 3 x 21 867: the weight kernel's second trip starts at pixel
# 1024 x 64 = 65 536 and its last chunk holds one pixel.  2 x 5 x 52 459 = 524 590 = 2048 x 256 + 302: the second trip of the forward
# and data kernels (an odd total, 524 589, has no B = 2 form).
HEAD_SMALL = [(o, b, 1, m) for o in HEAD_O for m in HEAD_M for b in (1, 2)]
HEAD_TRIP_W = (16, 3, 1, 21867)
HEAD_TRIP_FD = (8, 2, 5, 52459)
HEAD_ON_DEVICE = [HEAD_TRIP_FD]
HEAD_CASES = HEAD_SMALL + [HEAD_TRIP_W, HEAD_TRIP_FD]


def _cdiv(a, b):
    return -(-a // b)


def _rng(name):
    return np.random.default_rng([20263, sum(ord(ch) * (i + 1) for i, ch in enumerate(name))])


def bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------------ tile arithmetic
def conv_arith(B, H, W):
    """v3d_dense_train_conv's launch: 16 x 16 tiles (3x3), runs of 128 pixels (1x1), one persistent grid for both"""
    tiles, runs = B * _cdiv(H, 16) * _cdiv(W, 16), _cdiv(B * H * W, 128)
    wg = min(tiles, runs, 256)
    return dict(tiles=tiles, runs=runs, workgroups=wg, wg0_tiles=(tiles - 1) // wg + 1, wg0_runs=(runs - 1) // wg + 1,
                two_tile_wgs=max(0, min(wg, tiles - wg)), two_run_wgs=max(0, min(wg, runs - wg)))


# what the cases are meant to hit: compared with conv_arith by the host test
CONV_CLAIMS = {
    (1, 1, 1): dict(tiles=1, runs=1, workgroups=1), (1, 1, 4): dict(tiles=1, workgroups=1), (1, 3, 3): dict(tiles=1, workgroups=1),
    (1, 15, 15): dict(tiles=1, runs=2, workgroups=1, wg0_runs=2), (1, 16, 16): dict(tiles=1, runs=2, workgroups=1),
    (1, 16, 17): dict(tiles=2, workgroups=2), (1, 17, 16): dict(tiles=2, workgroups=2),
    (1, 17, 17): dict(tiles=4, runs=3, workgroups=3, wg0_tiles=2, two_tile_wgs=1),
    (3, 17, 33): dict(tiles=18, runs=14, workgroups=14, wg0_tiles=2, two_tile_wgs=4),
    (1, 1, 4113): dict(tiles=258, runs=33, workgroups=33, wg0_tiles=8, wg0_runs=1),
    (1, 17, 2049): dict(tiles=258, runs=273, workgroups=256, wg0_tiles=2, wg0_runs=2, two_tile_wgs=2, two_run_wgs=17),
}


def conv_owner(B, H, W, ksize):
    """(B, H, W) int: the workgroup (= row of `stats`) that computes each output pixel"""
    a = conv_arith(B, H, W)
    b, h, w = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    if ksize == 3:
        tile = (b * _cdiv(H, 16) + h // 16) * _cdiv(W, 16) + w // 16
    else:
        tile = ((b * H + h) * W + w) // 128
    return tile % a["workgroups"], tile


def wgrad_arith(B, H, W):
    """dt_wgrad: 8 x 16 tiles dealt to min(tiles, 64) slabs, slab s takes tiles s, s + slabs, ..."""
    tiles = B * _cdiv(H, 8) * _cdiv(W, 16)
    slabs = min(tiles, 64)
    return dict(tiles=tiles, slabs=slabs, slab0_tiles=(tiles - 1) // slabs + 1)


WGRAD_CLAIMS = {
    (1, 1, 1): dict(tiles=1, slabs=1), (1, 3, 3): dict(tiles=1, slabs=1), (1, 8, 16): dict(tiles=1, slabs=1), (1, 9, 17): dict(tiles=4, slabs=4),
    (3, 9, 17): dict(tiles=12, slabs=12), (1, 8, 1008): dict(tiles=63, slabs=63, slab0_tiles=1),
    (1, 8, 1024): dict(tiles=64, slabs=64, slab0_tiles=1), (1, 8, 1040): dict(tiles=65, slabs=64, slab0_tiles=2),
    (1, 8, 2064): dict(tiles=129, slabs=64, slab0_tiles=3),
}


def head_arith(B, H, W):
    """dt_head_*: forward / data gradient 256 pixels per block on at most 2048 blocks; weight gradient 64-pixel chunks on at most 1024"""
    M = B * H * W
    fd_blocks, w_blocks = min(_cdiv(M, 256), 2048), min(_cdiv(M, 64), 1024)
    return dict(M=M, fd_blocks=fd_blocks, fd_trips=_cdiv(M, 256 * fd_blocks), w_blocks=w_blocks, w_trips=_cdiv(_cdiv(M, 64), w_blocks),
                last_chunk=(M - 1) % 64 + 1)


HEAD_CLAIMS = {HEAD_TRIP_W: dict(M=65601, w_blocks=1024, w_trips=2, last_chunk=1, fd_trips=1),
               HEAD_TRIP_FD: dict(M=524590, fd_blocks=2048, fd_trips=2)}


# ------------------------------------------------------------------------------------------------ operands
def seam_mask(B, H, W):
    """(B, H, W, 1) bool: image borders and the seams of the 16 x 16 and 8 x 16 tiles"""
    h, w = np.arange(H), np.arange(W)
    hs = np.isin(h % 16, (0, 7, 8, 15)) | (h == H - 1)
    ws = np.isin(w % 16, (0, 15)) | (w == W - 1)
    return np.broadcast_to((hs[:, None] | ws[None, :])[None, :, :, None], (B, H, W, 1))


def _act(kind, rng, shape):
    B, H, W = shape
    if kind == "real":
        return bf16(rng.standard_normal((B, H, W, C)))
    x = rng.integers(-1, 2, (B, H, W, C))
    pm = rng.integers(0, 2, (B, H, W, C)) * 2 - 1
    return np.where(seam_mask(B, H, W) & (x == 0), pm, x).astype(np.float32)


def onehot_pixels(B, H, W):
    px = {(b, h, w): 1.0 for b in range(B) for h in (0, H - 1) for w in (0, W - 1)}
    if H > 15 and W > 15:
        px[(0, 15, 15)] = 1.0
    if H > 16 and W > 16:
        px[(0, 16, 16)] = 2.0
    px.setdefault((B - 1, H - 1, W - 1), 1.0)
    return px


@functools.lru_cache(maxsize=None)
def conv_case(shape, ksize, kind):
    """-> dict(name, shape, ksize, kind, x (B, H, W, 128), w (128, 128, k, k), arith)"""
    B, H, W = shape
    rng = _rng(f"conv {shape} {ksize} {kind}")
    if kind == "onehot":
        x = np.zeros((B, H, W, C), np.float32)
        for p, v in onehot_pixels(B, H, W).items():
            x[p][[CI, CO]] = v
        w = np.zeros((C, C, ksize, ksize), np.float32)
        w[CO, CI] = np.arange(1, ksize * ksize + 1).reshape(ksize, ksize)
    elif kind == "int":
        x = _act(kind, rng, shape)
        w = ((rng.integers(0, 2, (C, C, ksize, ksize)) * 2 - 1) * (rng.random((C, C, ksize, ksize)) < 1 / 16)).astype(np.float32)
    else:
        x = _act(kind, rng, shape)
        w = bf16(rng.standard_normal((C, C, ksize, ksize)) / np.sqrt(C * ksize * ksize))
    frozen(x, w)
    return dict(name=f"conv-{B}x{H}x{W}-k{ksize}-{kind}", shape=shape, ksize=ksize, kind=kind, x=x, w=w, arith=conv_arith(*shape))


@functools.lru_cache(maxsize=None)
def wgrad_case(shape, kind):
    """-> dict(name, shape, kind, x, dy (B, H, W, 128), arith); the split kinds: x_hi, x_lo, dy_hi, dy_lo"""
    B, H, W = shape
    rng = _rng(f"wgrad {shape} {kind}")
    c = dict(name=f"wgrad-{B}x{H}x{W}-{kind}", shape=shape, kind=kind, arith=wgrad_arith(*shape))
    if kind in SPLIT_KINDS:
        def planes(with_lo):
            a = rng.integers(0, 4, (B, H, W, C))
            hi = (16 * np.array([-2, -1, 1, 2])[a]).astype(np.float32)
            lo = (rng.integers(0, 2, (B, H, W, C)) * 2 - 1).astype(np.float32) if with_lo else np.zeros((B, H, W, C), np.float32)
            return frozen(hi, lo)
        c["x_hi"], c["x_lo"] = planes(kind != "dy_lo")
        c["dy_hi"], c["dy_lo"] = planes(kind != "x_lo")
    else:
        c["x"], c["dy"] = frozen(_act(kind, rng, shape), _act(kind, rng, shape))
    return c


@functools.lru_cache(maxsize=None)
def head_case(spec, kind):
    """-> dict(name, O, shape, kind, feat (B, H, W, 128), w (O, 128), bias (O), dmaps (B, O, H, W), arith)"""
    O, B, H, W = spec
    rng = _rng(f"head {spec} {kind}")
    if kind == "int":
        feat = rng.integers(-1, 2, (B, H, W, C), dtype=np.int8).astype(np.float32)
        w = rng.integers(-1, 2, (O, C)).astype(np.float32)
        bias = rng.integers(-2, 3, O).astype(np.float32)
        dmaps = rng.integers(-1, 2, (B, O, H, W), dtype=np.int8).astype(np.float32)
    else:
        feat = bf16(rng.standard_normal((B, H, W, C), dtype=np.float32))
        w = (rng.standard_normal((O, C)) * 0.05).astype(np.float32)
        bias = (rng.standard_normal(O) * 0.1).astype(np.float32)
        dmaps = rng.standard_normal((B, O, H, W), dtype=np.float32)
    frozen(feat, w, bias, dmaps)
    return dict(name=f"head-O{O}-{B}x{H}x{W}-{kind}", O=O, shape=(B, H, W), kind=kind, feat=feat, w=w, bias=bias, dmaps=dmaps,
                arith=head_arith(B, H, W))


# ------------------------------------------------------------------------------------------------ references (torch, float64)
def _nchw(a, device):
    return torch.tensor(a).to(device).double().permute(0, 3, 1, 2)


def _nhwc_out(t):
    return t.permute(0, 2, 3, 1).contiguous().cpu().numpy()


def conv_reference(x, w, transpose, device="cpu", dtype=torch.float64):
    """-> (y, mag) (B, H, W, 128): torch's conv2d (transpose = 0) / conv_transpose2d (1: the data gradient of the layer with weights w, x in
    the role of dY), and the same on the absolute values"""
    k = w.shape[-1]
    f = F.conv_transpose2d if transpose else F.conv2d
    xt, wt = _nchw(x, device).to(dtype), torch.tensor(w).to(device).to(dtype)
    return _nhwc_out(f(xt, wt, padding=k // 2)), _nhwc_out(f(xt.abs(), wt.abs(), padding=k // 2))


def _wgrad(xt, dyt, ksize):
    w = torch.zeros((C, C, ksize, ksize), dtype=xt.dtype, device=xt.device, requires_grad=True)
    F.conv2d(xt, w, padding=ksize // 2).backward(dyt)
    return w.grad


def wgrad_reference(x, dy, ksize, device="cpu", dtype=torch.float64):
    """-> (dW, mag) (128, 128, k, k): autograd's weight gradient of conv2d(x, W, padding = k / 2) under the output gradient dy"""
    xt, dyt = _nchw(x, device).to(dtype), _nchw(dy, device).to(dtype)
    return _wgrad(xt, dyt, ksize).cpu().numpy(), _wgrad(xt.abs(), dyt.abs(), ksize).cpu().numpy()


def wgrad_split_terms(c, ksize, device="cpu"):
    """-> the three terms (x_hi, dy_hi), (x_hi, dy_lo), (x_lo, dy_hi) of the split weight gradient, float64 each"""
    p = {k: _nchw(c[k], device) for k in ("x_hi", "x_lo", "dy_hi", "dy_lo")}
    return [_wgrad(p[a], p[b], ksize).cpu().numpy() for a, b in (("x_hi", "dy_hi"), ("x_hi", "dy_lo"), ("x_lo", "dy_hi"))]


def head_reference(c, device="cpu", dtype=torch.float64):
    """-> dict of (value, mag) for maps (B, O, H, W), dfeat (B, H, W, 128), dw (O, 128), db (O): conv2d with bias and its autograd"""
    O = c["O"]

    def run(feat, w, bias, dm):
        feat, w, bias = feat.requires_grad_(True), w.requires_grad_(True), bias.requires_grad_(True)
        maps = F.conv2d(feat, w.view(O, C, 1, 1), bias)
        maps.backward(dm)
        return maps.detach().cpu().numpy(), _nhwc_out(feat.grad), w.grad.cpu().numpy(), bias.grad.cpu().numpy()
    t = [_nchw(c["feat"], device).to(dtype)] + [torch.tensor(c[k]).to(device).to(dtype) for k in ("w", "bias", "dmaps")]
    val = run(*[a.clone() for a in t])
    mag = run(*[a.abs() for a in t])
    return {k: (v, m) for k, v, m in zip(("maps", "dfeat", "dw", "db"), val, mag)}


# ------------------------------------------------------------------------------------------------ bars
def half_ulp_bf16(ref):
    """half a bf16 ulp (8 significant bits) of the binade of each reference value; 0 at 0"""
    _, e = np.frexp(ref)  # |ref| = m 2^e, m in [0.5, 1): the binade starts at 2^(e - 1), its ulp is 2^(e - 8)
    return np.where(ref != 0, np.ldexp(1.0, e - 9), 0.0)


def bf16_bar(ref, mag, n):
    return half_ulp_bf16(ref) + n * U * mag


def fp32_bar(mag, n):
    return n * U * mag


def fraction(got, want, bar):
    """the largest |got - want| in units of the elementwise bar (0 / 0 counts as 0, x / 0 as infinity)"""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        fr = np.where(err == 0, 0.0, err / bar)
    return float(fr.max()) if fr.size else 0.0


def stats_rows(y, owner, rows):
    """(rows, 2, 128) float64: per-workgroup channel sums and sums of squares of y (B, H, W, 128), and the same of |y| for the bar"""
    out, mag = np.zeros((rows, 2, C)), np.zeros((rows, 2, C))
    y2 = y.reshape(-1, C).astype(np.float64)
    o = owner.reshape(-1)
    np.add.at(out[:, 0], o, y2)
    np.add.at(out[:, 1], o, y2 * y2)
    np.add.at(mag[:, 0], o, np.abs(y2))
    mag[:, 1] = out[:, 1]
    return out, mag, np.bincount(o, minlength=rows)

"""The dense training kernels of csrc/dense_train.hip -- dt_conv3_kernel, dt_conv_kernel<1>, dt_wgrad_kernel<9|1> + dt_wgrad_reduce_kernel
(both arithmetics), the three dt_head_* kernels -- through raw C-ABI calls on the cases of tests/dense_train_cases.py, against torch's
float64 conv2d / conv_transpose2d and its autograd.  Integer, one-hot and split cases must EQUAL float64, element for element; real-valued
cases keep the elementwise bars derived in dense_train_cases.  tests/test_host_dense_train_cases.py shows on the host that the cases hit the
tile arithmetic they claim, that the exactness conditions hold, that a float32 torch model keeps half of every bar, and which case notices
which planted mistake.

Every raw call: outputs pre-filled with NaN with GUARD elements on both sides, workspaces of 0xFF bytes with a guard behind them, inputs
compared with their copies afterwards, every call made twice with bit-equal results; a workspace one byte short returns V3D_EWORKSPACE and
writes nothing; `stats` has v3d_dense_train_conv_tiles rows (= the Python arithmetic), every one written and nothing behind them.

Which case reaches what (dense_train_cases.CONV_CLAIMS / WGRAD_CLAIMS / HEAD_CLAIMS, asserted on the host):
  conv  1x1x1, 1x1x4, 1x3x3     below one tile (W = 1, 3, 4: below the W >= 4 gate of dense_train.why_unsupported)
        1x15x15 .. 1x17x17      one full 16 x 16 tile and one over; 17 x 17: 3 workgroups for 4 tiles, workgroup 0 owns tiles 0 and 3
        3x17x33                 18 tiles on 14 workgroups, image boundaries inside a workgroup's tile list and inside a 128-pixel run
        1x1x4113                258 tiles on 33 workgroups, 8 or 7 each;  1x17x2049: both kernels at the 256-workgroup cap
  dW    1x1x1, 1x3x3            W = 1 and 3 again;  3x9x17: 12 tiles, batch boundaries between the slabs
        1x8x1008 / 1024 / 1040  63 / 64 / 65 tiles: slab 0's second tile;  1x8x2064: 129 tiles, slab 0 takes three, both LDS buffers reused
        the split form on every shape: x carries a lo plane, dY does, both -- 192 partials at 64 and 65 tiles
  head  every O at M in {1, 63, 64, 65, 255, 256, 257} as one image and as two images of M pixels; O = 16 at M = 65 601 (the weight
        kernel's second trip, a one-pixel chunk); O = 8 at M = 524 590 (the second trip of the forward and data kernels)
  step  v3d_dense_train_forward_split / _backward_split, 1 and 2 layers, 3x3 and 1x1, on 1x17x17, 3x17x33, 1x8x1040 against float64 torch
        modules: this is what pins the split data gradient (dt_wt_flip_kernel + v3d_conv2d_pack_weights) at tile edges.

Observed on the MI355X.  Every integer, one-hot and split case equals float64, the statistics rows included; no kernel had to change.
Largest |error| in units of the elementwise bar, per group (every test prints its own line, `OBSERVED ...`):
  conv y      3x3 0.935 forward / 0.931 data gradient (1x1x4113), 1x1 0.996 (1x17x2049) / 0.995 (3x17x33): a bf16 output's bar is its own
              rounding, half an ulp, plus an accumulation term a tenth of that -- the largest of 10^5 .. 10^6 roundings comes close to it
  conv stats  0.248 (3x3) and 0.318 (1x1), both at 1x1x4: four pixels against a bar of four u
  dW          0.138 / 0.125 (1x3x3, nine pixels), 0.011 (1x8x16); 0.000 from 63 tiles on: n u sum|x||dY| grows with the pixels, the
              error of the two-level sum does not -- the exact cases are what watches the large shapes
  head        maps 0.049 (M = 524 590); dfeat 1.000 to three digits (bf16 output, as conv y); dW 0.996 and db 0.496 at M = 1 and 2 (ONE or
              two roundings against a bar of one or two u), 0.002 and 0.001 from M = 63 on
  split step  relative L2 against float64 (the fp32 torch modules' own in brackets), worst over the twelve runs: maps 9.8e-6 (4.0e-7),
              d(input) 8.4e-6 (8.7e-7), dW 3.8e-5 (8.3e-6), dgamma 3.8e-5 (2.2e-6), dbeta 2.5e-5 (5.7e-6), head dW 7.7e-6 (1.1e-6), head db
              2.5e-7 (2.0e-6) -- all under the 2e-4 floor of the bar.  One tensor has no meaningful figure: dbeta of layer 0 of the
              two-layer 1x1 stacks is mathematically ZERO (a channel offset in front of a 1x1 convolution is removed by the next
              BatchNorm; the 3x3 stacks keep a border term): all three computations return their own rounding noise, and the
              figures "2.0e+9 .. 3.5e+9 (3.0e+8 .. 5.1e+8)" are one noise relative to another, inside the rule's 256 x.
The file's 254 tests run in 12 s.
"""
import numpy as np
import pytest
import torch

import dense_train_cases as dc

pytestmark = pytest.mark.gpu

EINVAL, EWORKSPACE = -1, -2
GUARD = 4096      # elements in front of and behind every output
WS_GUARD = 4096   # bytes behind a workspace
NAN = float("nan")


def _lib():
    from vision3d_amd import _lib as L
    return L, L.lib()


def dev(a, dtype=None):
    t = torch.tensor(a).cuda()
    return t if dtype is None else t.to(dtype)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Out(object):
    """an output of n elements pre-filled with NaN between two guards"""

    def __init__(self, n, dtype=torch.float32):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), NAN, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]

    def intact(self):
        return bool(self.buf[:GUARD].isnan().all() and self.buf[GUARD + self.n:].isnan().all())

    def untouched(self):
        return bool(self.buf.isnan().all())

    def numpy(self, *shape):
        return self.t.float().cpu().numpy().reshape(shape)


class Inputs(object):
    def __init__(self, **tensors):
        self.t = tensors
        self.copies = {k: v.clone() for k, v in tensors.items()}

    def check(self, what):
        for k, v in self.copies.items():
            assert torch.equal(bits(self.t[k]), bits(v)), f"{what}: input {k} was written"


def workspace(nbytes):
    return torch.full((nbytes + WS_GUARD,), 0xFF, dtype=torch.uint8, device="cuda")


def ref_device(on_device):
    return "cuda" if on_device else "cpu"


# ------------------------------------------------------------------------------------------------------------------ convolution
def raw_conv(c, transpose):
    """one v3d_dense_train_conv call with statistics -> (y Out, stats Out, rows)"""
    L, lib = _lib()
    B, H, W = c["shape"]
    k = c["ksize"]
    w = dev(c["w"])
    img = torch.empty(int(lib.v3d_dense_train_weight_image_bytes(k)) // 4, dtype=torch.int32, device="cuda")
    L.check(lib.v3d_dense_train_pack_weights(L.ptr(w), k, transpose, L.ptr(img), L.stream_ptr()), "pack")
    inp = Inputs(x=dev(c["x"], torch.bfloat16), w=w, img=img)
    rows = int(lib.v3d_dense_train_conv_tiles(B, H, W))
    y, stats = Out(B * H * W * dc.C, torch.bfloat16), Out(rows * 2 * dc.C)
    code = lib.v3d_dense_train_conv(L.ptr(inp.t["x"]), L.ptr(img), B, H, W, k, L.ptr(y.t), L.ptr(stats.t), L.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0
    inp.check(c["name"])
    assert y.intact() and stats.intact(), f"{c['name']}: written outside y or behind the {rows} rows of stats"
    assert not y.t.isnan().any(), f"{c['name']}: {int(y.t.isnan().sum())} elements of y not written"
    assert not stats.t.isnan().any(), f"{c['name']}: a row of stats not written"
    return y, stats, rows


CONV_PARAMS = [(s, k, kind) for s in dc.CONV_SHAPES for k in (3, 1) for kind in ("int", "real")] + \
              [(s, k, "onehot") for s in dc.ONEHOT_SHAPES for k in (3, 1)]


@pytest.mark.parametrize("shape,ksize,kind", CONV_PARAMS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_the_convolution_and_its_data_gradient_form(shape, ksize, kind):
    c = dc.conv_case(shape, ksize, kind)
    B, H, W = shape
    owner, _ = dc.conv_owner(B, H, W, ksize)
    for transpose in (0, 1):
        y, stats, rows = raw_conv(c, transpose)
        assert rows == c["arith"]["workgroups"], "v3d_dense_train_conv_tiles against the Python arithmetic"
        want, mag = dc.conv_reference(c["x"], c["w"], transpose, ref_device(shape in dc.CONV_ON_DEVICE))
        got, st = y.numpy(B, H, W, dc.C), stats.numpy(rows, 2, dc.C)
        what = f"{c['name']} transpose {transpose}"
        if kind == "real":
            fr = dc.fraction(got, want, dc.bf16_bar(want, mag, dc.C * ksize * ksize))
            sw, sm, cnt = dc.stats_rows(got, owner, rows)  # sums of the values the kernel itself stored
            fs = dc.fraction(st, sw, dc.fp32_bar(sm, cnt[:, None, None]))
            print(f"OBSERVED conv {what}: y at {fr:.3f} of the bar, stats at {fs:.3f}")
            assert fr <= 1 and fs <= 1, (what, fr, fs)
        else:
            bad = (got != want).any(-1)
            assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ from float64, first at (b, h, w) = {tuple(np.argwhere(bad)[0])}"
            sw, sm, _ = dc.stats_rows(want, owner, rows)
            assert sm.max() < 2 ** 24
            assert np.array_equal(st, sw), f"{what}: statistics rows {np.unique(np.argwhere(st != sw)[:, 0]).tolist()} differ"
        y2, stats2, _ = raw_conv(c, transpose)
        assert torch.equal(bits(y.t), bits(y2.t)) and torch.equal(bits(stats.t), bits(stats2.t)), f"{what}: two runs differ"


# ------------------------------------------------------------------------------------------------------------------ weight gradient
def raw_wgrad(c, ksize, short=0):
    """one v3d_dense_train_wgrad[_split] call -> (code, dW Out, workspace, its size)"""
    L, lib = _lib()
    B, H, W = c["shape"]
    split = c["kind"] in dc.SPLIT_KINDS
    names = ("x_hi", "x_lo", "dy_hi", "dy_lo") if split else ("x", "dy")
    inp = Inputs(**{k: dev(c[k], torch.bfloat16) for k in names})
    nbytes = int(lib.v3d_dense_train_wgrad_workspace(ksize)) * (3 if split else 1)
    ws, dw = workspace(nbytes), Out(dc.C * dc.C * ksize * ksize)
    fn = lib.v3d_dense_train_wgrad_split if split else lib.v3d_dense_train_wgrad
    code = fn(*[L.ptr(inp.t[k]) for k in names], B, H, W, ksize, L.ptr(dw.t), L.ptr(ws), nbytes - short, L.stream_ptr())
    torch.cuda.synchronize()
    inp.check(c["name"])
    assert dw.intact(), f"{c['name']}: written outside dW"
    assert bool((ws[nbytes:] == 0xFF).all()), f"{c['name']}: written behind the workspace"
    return code, dw, ws


def check_wgrad(c, ksize, want, bar):
    code, dw, _ = raw_wgrad(c, ksize)
    assert code == 0 and not dw.t.isnan().any(), "every element written"
    got = dw.numpy(dc.C, dc.C, ksize, ksize)
    what = f"{c['name']} k{ksize}"
    if bar is None:
        bad = got != want
        assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} elements differ from float64, first at (co, ci, ky, kx) = " \
                              f"{tuple(np.argwhere(bad)[0])}: {got[bad][0]} for {want[bad][0]}"
    else:
        fr = dc.fraction(got, want, bar)
        print(f"OBSERVED dW {what}: at {fr:.3f} of the bar")
        assert fr <= 1, (what, fr)
    code, again, _ = raw_wgrad(c, ksize)
    assert code == 0 and torch.equal(bits(dw.t), bits(again.t)), f"{what}: two runs differ"
    code, none, ws = raw_wgrad(c, ksize, short=1)
    assert code == EWORKSPACE and none.untouched() and bool((ws == 0xFF).all()), f"{what}: a short workspace must write nothing"


@pytest.mark.parametrize("ksize", [3, 1])
@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("shape", dc.WGRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_weight_gradient(shape, kind, ksize):
    c = dc.wgrad_case(shape, kind)
    want, mag = dc.wgrad_reference(c["x"], c["dy"], ksize)
    check_wgrad(c, ksize, want, dc.fp32_bar(mag, shape[0] * shape[1] * shape[2]) if kind == "real" else None)


@pytest.mark.parametrize("ksize", [3, 1])
@pytest.mark.parametrize("kind", dc.SPLIT_KINDS)
@pytest.mark.parametrize("shape", dc.WGRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_split_weight_gradient_is_three_terms_exactly(shape, kind, ksize):
    """hi*hi + hi*lo + lo*hi, each once: the exact product of the split tensors minus lo*lo"""
    c = dc.wgrad_case(shape, kind)
    check_wgrad(c, ksize, sum(dc.wgrad_split_terms(c, ksize)), None)


def test_the_weight_gradient_return_codes():
    L, lib = _lib()
    c = dc.wgrad_case((1, 9, 17), "both")
    t = {k: dev(c[k], torch.bfloat16) for k in ("x_hi", "x_lo", "dy_hi", "dy_lo")}
    nbytes = 3 * int(lib.v3d_dense_train_wgrad_workspace(3))
    ws, dw = workspace(nbytes), Out(dc.C * dc.C * 9)
    good = [L.ptr(t["x_hi"]), L.ptr(t["x_lo"]), L.ptr(t["dy_hi"]), L.ptr(t["dy_lo"]), 1, 9, 17, 3, L.ptr(dw.t), L.ptr(ws), nbytes, L.stream_ptr()]
    for i, v in [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (7, 2), (8, 0), (9, 0)]:
        args = list(good)
        args[i] = v
        assert lib.v3d_dense_train_wgrad_split(*args) == EINVAL, i
    args = list(good)
    args[10] = 2 * int(lib.v3d_dense_train_wgrad_workspace(3))  # enough for the bf16 form, not for three terms
    assert lib.v3d_dense_train_wgrad_split(*args) == EWORKSPACE
    torch.cuda.synchronize()
    assert dw.untouched() and bool((ws == 0xFF).all())


# ------------------------------------------------------------------------------------------------------------------ head
def raw_head(c, short=0):
    """v3d_dense_train_head_fwd + _bwd -> (code of the backward, dict of Outs, workspace)"""
    L, lib = _lib()
    B, H, W = c["shape"]
    O, M = c["O"], c["arith"]["M"]
    inp = Inputs(feat=dev(c["feat"], torch.bfloat16), w=dev(c["w"]), bias=dev(c["bias"]), dmaps=dev(c["dmaps"]))
    o = dict(maps=Out(M * O), dfeat=Out(M * dc.C, torch.bfloat16), dw=Out(O * dc.C), db=Out(O))
    p = {k: L.ptr(v) for k, v in inp.t.items()}
    code = lib.v3d_dense_train_head_fwd(p["feat"], B, H, W, p["w"], p["bias"], O, L.ptr(o["maps"].t), L.stream_ptr())
    assert code == 0
    nbytes = int(lib.v3d_dense_train_head_workspace(O))
    ws = workspace(nbytes)
    code = lib.v3d_dense_train_head_bwd(p["feat"], p["dmaps"], B, H, W, p["w"], O, L.ptr(o["dfeat"].t), L.ptr(o["dw"].t), L.ptr(o["db"].t),
                                        L.ptr(ws), nbytes - short, L.stream_ptr())
    torch.cuda.synchronize()
    inp.check(c["name"])
    for k, v in o.items():
        assert v.intact(), f"{c['name']}: written outside {k}"
    assert bool((ws[nbytes:] == 0xFF).all()), f"{c['name']}: written behind the workspace"
    return code, o, ws


def head_shapes(c):
    B, H, W = c["shape"]
    return dict(maps=(B, c["O"], H, W), dfeat=(B, H, W, dc.C), dw=(c["O"], dc.C), db=(c["O"],))


def check_head(spec, kind):
    c = dc.head_case(spec, kind)
    code, o, _ = raw_head(c)
    assert code == 0
    ref = dc.head_reference(c, ref_device(spec in dc.HEAD_ON_DEVICE))
    M, O = c["arith"]["M"], c["O"]
    n = dict(maps=dc.C + 1, dfeat=O, dw=M, db=M)
    frs = {}
    for k, shp in head_shapes(c).items():
        assert not o[k].t.isnan().any(), f"{c['name']}: {k} not written everywhere"
        got, (want, mag) = o[k].numpy(*shp), ref[k]
        if kind == "int":
            bad = got != want
            assert not bad.any(), f"{c['name']}: {k} differs from float64 in {int(bad.sum())} elements, first at {tuple(np.argwhere(bad)[0])}"
        else:
            bar = dc.bf16_bar(want, mag, n[k]) if k == "dfeat" else dc.fp32_bar(mag, n[k])
            frs[k] = dc.fraction(got, want, bar)
            assert frs[k] <= 1, (c["name"], k, frs[k])
    if frs:
        print(f"OBSERVED head {c['name']}: " + ", ".join(f"{k} at {v:.3f}" for k, v in frs.items()) + " of the bar")
    code, again, _ = raw_head(c)
    assert code == 0 and all(torch.equal(bits(o[k].t), bits(again[k].t)) for k in o), f"{c['name']}: two runs differ"
    return c


@pytest.mark.parametrize("spec", dc.HEAD_SMALL, ids=lambda s: "O%d-%dx%dx%d" % s)
def test_the_head_at_every_width_around_its_chunk_and_block_edges(spec):
    check_head(spec, "int")
    check_head(spec, "real")


@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("spec", [dc.HEAD_TRIP_W, dc.HEAD_TRIP_FD], ids=lambda s: "O%d-%dx%dx%d" % s)
def test_the_heads_grid_stride_loops(spec, kind):
    check_head(spec, kind)


def test_the_head_return_codes():
    c = dc.head_case((16, 2, 1, 65), "int")
    code, o, ws = raw_head(c, short=1)
    assert code == EWORKSPACE
    assert all(o[k].untouched() for k in ("dfeat", "dw", "db")) and bool((ws == 0xFF).all()), "a short workspace must write nothing"


# ------------------------------------------------------------------------------------------------------------------ the split step
def l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("ksize", [3, 1])
@pytest.mark.parametrize("n_layers", [1, 2])
@pytest.mark.parametrize("shape", [(1, 17, 17), (3, 17, 33), (1, 8, 1040)], ids=lambda s: "x".join(map(str, s)))
def test_the_split_step_through_its_public_entry(shape, n_layers, ksize):
    """n x (conv + BatchNorm(batch statistics, offsets of +8: no ReLU decision near zero) + ReLU) + a 16-wide head in the fp32-class
    arithmetic against float64 torch modules; the bar per tensor is tests/test_gpu_dense_train.py's for this arithmetic"""
    from torch import nn
    L, lib = _lib()
    B, H, W = shape
    O, eps, mom = 16, 1e-3, 0.01
    g = torch.Generator().manual_seed(1000 * n_layers + 10 * ksize + H + W)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x32 = r(B, H, W, dc.C).cuda()
    hi = x32.bfloat16()
    lo = (x32 - hi.float()).bfloat16()
    xin = (hi.float() + lo.float()).permute(0, 3, 1, 2).cpu()  # the value the planes hold
    ws = [r(dc.C, dc.C, ksize, ksize) / (dc.C * ksize * ksize) ** 0.5 for _ in range(n_layers)]
    gammas = [torch.rand(dc.C, generator=g) * 0.8 + 0.6 for _ in range(n_layers)]
    betas = [torch.rand(dc.C, generator=g) * 0.4 - 0.2 + 8.0 for _ in range(n_layers)]
    hw, hb, gmap = r(O, dc.C) * 0.05, r(O) * 0.1, r(B, O, H, W)

    def torch_run(dtype):
        mods = []
        for l in range(n_layers):
            conv, bn = nn.Conv2d(dc.C, dc.C, ksize, padding=ksize // 2, bias=False), nn.BatchNorm2d(dc.C, eps=eps, momentum=mom)
            with torch.no_grad():
                conv.weight.copy_(ws[l]), bn.weight.copy_(gammas[l]), bn.bias.copy_(betas[l])
            mods += [conv, bn, nn.ReLU()]
        head = nn.Conv2d(dc.C, O, 1)
        with torch.no_grad():
            head.weight.copy_(hw.view(O, dc.C, 1, 1)), head.bias.copy_(hb)
        net = nn.Sequential(*mods, head).to(dtype).train()
        xi = xin.to(dtype).requires_grad_(True)
        out = net(xi)
        (out * gmap.to(dtype)).sum().backward()
        res = {"maps": out.detach(), "d(input)": xi.grad}
        for l in range(n_layers):
            res[f"dW{l}"], res[f"dgamma{l}"], res[f"dbeta{l}"] = mods[3 * l].weight.grad, mods[3 * l + 1].weight.grad, mods[3 * l + 1].bias.grad
        res["head dW"], res["head db"] = head.weight.grad.view(O, dc.C), head.bias.grad
        return res

    d = {k: [t.cuda().contiguous() for t in v] for k, v in dict(w=ws, gamma=gammas, beta=betas).items()}
    rm, rv = [torch.zeros(dc.C, device="cuda") for _ in ws], [torch.ones(dc.C, device="cuda") for _ in ws]
    nbt = [torch.zeros((), dtype=torch.int64, device="cuda") for _ in ws]
    gw = [torch.full((dc.C, dc.C, ksize, ksize), NAN, device="cuda") for _ in ws]
    gg, gb = [torch.full((dc.C,), NAN, device="cuda") for _ in ws], [torch.full((dc.C,), NAN, device="cuda") for _ in ws]
    io = (L.DenseTrainLayer * n_layers)()
    for l, s in enumerate(io):
        s.weight, s.gamma, s.beta = L.ptr(d["w"][l]), L.ptr(d["gamma"][l]), L.ptr(d["beta"][l])
        s.running_mean, s.running_var, s.num_batches_tracked = L.ptr(rm[l]), L.ptr(rv[l]), L.ptr(nbt[l])
        s.eps, s.momentum, s.ksize = eps, mom, ksize
        s.grad_weight, s.grad_gamma, s.grad_beta = L.ptr(gw[l]), L.ptr(gg[l]), L.ptr(gb[l])
    hwd, hbd, gmd = hw.cuda().contiguous(), hb.cuda(), gmap.cuda().contiguous()
    arena = torch.empty(int(lib.v3d_dense_train_arena_bytes_split(B, H, W, n_layers, O)), dtype=torch.uint8, device="cuda")
    maps = torch.full((B, O, H, W), NAN, device="cuda")
    dhw, dhb = torch.full((O, dc.C), NAN, device="cuda"), torch.full((O,), NAN, device="cuda")
    dx = torch.full((2, B, H, W, dc.C), NAN, dtype=torch.bfloat16, device="cuda")
    L.check(lib.v3d_dense_train_forward_split(L.ptr(hi), L.ptr(lo), B, H, W, io, n_layers, L.ptr(hwd), L.ptr(hbd), O, L.ptr(arena), L.ptr(maps),
                                              L.stream_ptr()), "forward_split")
    L.check(lib.v3d_dense_train_backward_split(L.ptr(hi), L.ptr(lo), L.ptr(gmd), B, H, W, io, n_layers, L.ptr(hwd), O, L.ptr(arena), L.ptr(dhw),
                                               L.ptr(dhb), L.ptr(dx[0]), L.ptr(dx[1]), L.stream_ptr()), "backward_split")
    torch.cuda.synchronize()
    mine = {"maps": maps, "d(input)": (dx[0].float() + dx[1].float()).permute(0, 3, 1, 2), "head dW": dhw, "head db": dhb}
    for l in range(n_layers):
        mine[f"dW{l}"], mine[f"dgamma{l}"], mine[f"dbeta{l}"] = gw[l], gg[l], gb[l]
        assert int(nbt[l]) == 1
    r64, r32 = torch_run(torch.float64), torch_run(torch.float32)
    line = []
    for k, want in r64.items():
        assert torch.isfinite(mine[k]).all(), k
        e, own = l2(mine[k], want), l2(r32[k], want)
        line.append(f"{k} {e:.1e} ({own:.1e})")
        assert e < max(2e-4, 256 * own), (k, e, own)
    print(f"OBSERVED step {B}x{H}x{W} layers {n_layers} k{ksize}: " + ", ".join(line))

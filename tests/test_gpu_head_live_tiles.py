"""GPU: the fused RPN tail + head over the LIVE tiles only (v3d_conv2d_1x1_head_fused_tiles, csrc/dense_conv.hip) against the
every-pixel entry on the planes a frame holds -- computed values in the tiles the last 3x3 layer convolved, that layer's empty-map
response in the others -- bit for bit, in both arithmetics; then through DenseHeadPlan with a persistent state, eagerly and from a
captured graph."""
import numpy as np
import pytest
import torch

from gpu_util import randomize_bn
from vision3d_amd.core.config import second_car_cfg

pytestmark = pytest.mark.gpu

TH, TW = 5, 16  # the tile of the 3x3 layers' tile kernel (D2_TH x D2_TW), tiles in (b, ty, tx) order
NAN16 = 0x7FFF  # a NaN in bf16 and in f16


def _tiles(b, h, w):
    return b, (h + TH - 1) // TH, (w + TW - 1) // TW


def _pixel_mask(state, b, h, w):
    """(n_tiles,) 0 / 1 -> bool (b, h, w): the pixels of the live tiles"""
    nb, ty, tx = _tiles(b, h, w)
    m = state[:nb * ty * tx].reshape(nb, ty, tx).bool()
    return m.repeat_interleave(TH, 1).repeat_interleave(TW, 2)[:, :h, :w].contiguous()


def _patterns(n, seed):
    g = torch.Generator().manual_seed(seed)
    first, last = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    first[0], last[n - 1] = 1, 1
    return {"all live": torch.ones(n, dtype=torch.int32), "all dead": torch.zeros(n, dtype=torch.int32), "first": first, "last": last,
            "checkerboard": (torch.arange(n) % 2).to(torch.int32), "random": (torch.rand(n, generator=g) < 0.4).to(torch.int32)}


class _Tail(object):
    """Weights of a 1x1 128 -> 128 (+ ReLU) layer and a head of cout2 channels, random input planes for b images and one image of
    "background" planes under one scale entry, and the two entry points."""

    def __init__(self, b, h, w, cout2, precision, push=None):
        from vision3d_amd import _lib as L
        from vision3d_amd.runtime import pack_conv_weight, scale_entry_from_max, to_split_nhwc
        self.L, self.b, self.h, self.w, self.cout2 = L, b, h, w, cout2
        self.f16s = precision == "fp32"
        g = torch.Generator().manual_seed(b * 1000 + h * 10 + w + cout2)
        x = torch.randn(b + 1, 128, h, w, generator=g)
        x[b] = x[b].abs() * 0.5  # the last image plays the feeding layer's empty-map response
        w1 = torch.randn(128, 128, 1, 1, generator=g) / 128 ** 0.5
        s1 = torch.rand(128, generator=g) + 0.5
        self.b1 = (torch.randn(128, generator=g) * 0.2).cuda()
        w2 = torch.randn(cout2, 128, 1, 1, generator=g) / 128 ** 0.5
        self.b2 = (torch.randn(cout2, generator=g) * 0.2).cuda()
        mid = torch.relu(torch.nn.functional.conv2d(x.double(), (w1 * s1.view(-1, 1, 1, 1)).double(), self.b1.cpu().double()))
        self.mid_entry = scale_entry_from_max(mid.abs().max().float().cuda(), 1) if self.f16s else None
        if push is not None:  # (after the entry: these values leave the intermediate tensor's range)
            bb, ys, xs, factor = push
            x[bb, :, ys, xs] *= factor
        hi, lo = to_split_nhwc(x.cuda(), precision)
        self.in_entry = hi.v3d_entry if self.f16s else None
        self.hi, self.lo, self.bg_hi, self.bg_lo = hi[:b], lo[:b], hi[b:], lo[b:]
        self.img1, self.img2 = pack_conv_weight(w1.cuda(), s1.cuda(), precision), pack_conv_weight(w2.cuda(), None, precision)
        self.bg_maps = self.every_pixel(self.bg_hi, self.bg_lo)

    def _args(self, hi, lo, out, flag):
        from vision3d_amd.runtime import _prec_struct
        L = self.L
        ref, keep = _prec_struct((self.in_entry, self.mid_entry, flag) if self.f16s else None)
        return (L.ptr(hi), L.ptr(lo), L.ptr(self.img1), L.ptr(self.b1), 1, L.ptr(self.img2), L.ptr(self.b2), 0, hi.shape[0], self.h,
                self.w, 128, self.cout2, L.ptr(out), ref), keep

    def every_pixel(self, hi, lo, flag=None):
        L = self.L
        out = torch.full((hi.shape[0], self.cout2, self.h, self.w), float("nan"), device="cuda")
        args, keep = self._args(hi, lo, out, flag)
        L.check(L.lib().v3d_conv2d_1x1_head_fused(*args, L.stream_ptr()), "head_fused")
        torch.cuda.synchronize()
        return out

    def live_tiles(self, hi, lo, state, max_workgroups=0, flag=None):
        L = self.L
        out = torch.full((hi.shape[0], self.cout2, self.h, self.w), float("nan"), device="cuda")
        args, keep = self._args(hi, lo, out, flag)
        L.check(L.lib().v3d_conv2d_1x1_head_fused_tiles(*args, L.ptr(state), L.ptr(self.bg_maps), int(max_workgroups),
                                                         L.stream_ptr()), "head_fused_tiles")
        torch.cuda.synchronize()
        return out

    def frame(self, mask):
        """the planes a frame holds: random values in the live tiles, the background planes in the dead ones"""
        m = mask[..., None]
        return torch.where(m, self.hi, self.bg_hi.expand_as(self.hi)).contiguous(), torch.where(m, self.lo, self.bg_lo.expand_as(self.lo)).contiguous()


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("cout2", [16, 14])
@pytest.mark.parametrize("b,h,w,max_wg", [(1, 5, 16, 0), (1, 10, 32, 0), (2, 7, 20, 0), (2, 10, 48, 1), (2, 10, 48, 2)])
def test_live_tiles_equal_every_pixel_and_dead_inputs_are_unread(b, h, w, max_wg, cout2, precision):
    """One tile, 2 x 2 whole tiles, a partial tile in both directions with a second image, and 60 live row tiles against 9 and 18 wave
    slots (second and later passes); every state pattern.  The live-tiles entry equals the every-pixel entry on the frame's planes;
    with the dead tiles' input planes overwritten by NaNs it still does, and the dead tiles hold the background tensor."""
    from vision3d_amd import _lib as L
    t = _Tail(b, h, w, cout2, precision)
    nb, ty, tx = _tiles(b, h, w)
    n_words = int(L.lib().v3d_conv2d_bg_tiles(b, h, w))
    assert n_words >= nb * ty * tx
    for name, pat in _patterns(nb * ty * tx, b * 100 + h + w).items():
        state = torch.zeros(n_words, dtype=torch.int32)
        state[:nb * ty * tx] = pat
        state = state.cuda()
        mask = _pixel_mask(state, b, h, w)
        f_hi, f_lo = t.frame(mask)
        ref = t.every_pixel(f_hi, f_lo)
        got = t.live_tiles(f_hi, f_lo, state, max_wg)
        assert torch.equal(got, ref), name
        nan = torch.full_like(f_hi, NAN16)
        n_hi, n_lo = torch.where(mask[..., None], f_hi, nan), torch.where(mask[..., None], f_lo, nan)
        got = t.live_tiles(n_hi, n_lo, state, max_wg)
        assert torch.equal(got, ref), name + " (dead inputs NaN)"
        dead = ~mask[:, None].expand_as(got)
        assert torch.equal(got[dead], t.bg_maps.expand_as(got)[dead]), name + " (dead tiles = the background tensor)"


def test_range_flag_covers_the_computed_tiles_only():
    """f16s: values that push the intermediate tensor beyond its entry's limit raise the range flag when their tile is live and not
    when it is dead -- a dead tile's planes are never read."""
    b, h, w = 1, 10, 32
    t = _Tail(b, h, w, 16, "fp32", push=(0, slice(5, 10), slice(16, 32), 64.0))  # tile (ty 1, tx 1) = tile 3
    n_words = int(t.L.lib().v3d_conv2d_bg_tiles(b, h, w))
    for live3, want in ((1, 2), (0, 0)):
        state = torch.zeros(n_words, dtype=torch.int32)
        state[:4] = torch.tensor([1, 1, 1, live3])
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        t.live_tiles(t.hi, t.lo, state.cuda(), flag=flag)
        assert int(flag) == want, (live3, int(flag))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    t.every_pixel(t.hi, t.lo, flag=flag)
    assert int(flag) == 2  # (the every-pixel entry reads the tile whatever its state)


def _model(seed):
    from vision3d_amd.detector import Second
    torch.manual_seed(seed)
    model = Second(second_car_cfg())
    randomize_bn(model, seed)
    with torch.no_grad():
        model.head.conv_cls.weight.normal_(0, 0.05)
        model.head.conv_reg.weight.normal_(0, 0.02)
    return model.cuda().eval()


def _sparse_bev(b, h, w, pixels, seed):
    """fp32 (b, 128, h, w) BEV map with a few occupied pixels, and its inverted occupancy bitmap"""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(b, 128, h, w)
    occ = np.full((b * h, (w + 31) // 32), 0xFFFFFFFF, dtype=np.uint32)
    for bb, yy, xx in pixels:
        x[bb, :, yy, xx] = torch.randn(128, generator=g)
        occ[bb * h + yy, xx // 32] &= ~np.uint32(1 << (xx % 32))
    return x.cuda(), torch.from_numpy(occ.view(np.int32)).cuda()


FRAME_A = [(0, 2, 3), (1, 17, 44)]
FRAME_B = [(0, 18, 40), (1, 1, 1), (1, 9, 30)]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_through_the_plan_frames_graph_and_weight_change(precision):
    """DenseHeadPlan.forward(occ=..., work=state) on a small sparse BEV map (20 x 48: 12 tiles per image, most of them background behind
    six 3x3 layers) equals the same call with fuse_tail = False, frame after frame A, B, A on one state (tiles that die are
    rewritten), replayed from a captured graph, and again after a head bias changed (the background tensor is rebuilt in place)."""
    from vision3d_amd.runtime import DenseHeadPlan, to_split_nhwc
    b, h, w = 2, 20, 48
    model = _model(7)
    fused, plain = DenseHeadPlan(model.rpn, model.head, precision), DenseHeadPlan(model.rpn, model.head, precision)
    plain.fuse_tail = False
    dev = torch.device("cuda")
    frames = {}
    for name, pixels in (("A", FRAME_A), ("B", FRAME_B)):
        x, occ = _sparse_bev(b, h, w, pixels, len(pixels))
        frames[name] = (x, occ)
    # one scale entry for both frames' planes (f16s): split them as one tensor
    hi, lo = to_split_nhwc(torch.cat([frames["A"][0], frames["B"][0]]), precision)
    entry = getattr(hi, "v3d_entry", None)
    planes = {"A": (hi[:b], lo[:b], frames["A"][1]), "B": (hi[b:], lo[b:], frames["B"][1])}
    with torch.no_grad():
        st_f, st_p = fused.new_state(dev), plain.new_state(dev)
        want = {}
        for name in ("A", "B", "A"):
            p_hi, p_lo, occ = planes[name]
            ref = plain.forward(p_hi, p_lo, occ=occ, work=st_p, in_entry=entry)
            got = fused.forward(p_hi, p_lo, occ=occ, work=st_f, in_entry=entry)
            assert torch.equal(got, ref), name
            assert torch.equal(got, fused.forward(p_hi, p_lo, in_entry=entry)), name + " (every pixel)"
            live = st_f.tiles[len(fused.layers) - 3][:b * 4 * 3]  # the layer that feeds the tail
            assert 0 < int(live.sum()) < live.numel()
            want[name] = ref.clone()
        bg_head = fused.background_head(h, w, dev)
        assert bg_head is not None and tuple(bg_head.shape) == (1, fused.layers[-1]["cout"], h, w)

        # the same from a captured graph on a state of its own
        s_hi, s_lo, s_occ = planes["A"][0].clone(), planes["A"][1].clone(), planes["A"][2].clone()
        st_g = fused.new_state(dev)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fused.forward(s_hi, s_lo, occ=s_occ, work=st_g, in_entry=entry)  # (warm-up: allocations, the background)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = fused.forward(s_hi, s_lo, occ=s_occ, work=st_g, in_entry=entry)
        for name in ("A", "B", "A"):
            for dst, src in zip((s_hi, s_lo, s_occ), planes[name]):
                dst.copy_(src)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want[name]), name + " (graph replay)"
        del graph

        # a head bias changes: both plans repack, the background tensor is rebuilt where it was
        where = bg_head.data_ptr()
        before = bg_head.clone()
        model.head.conv_cls.bias.add_(0.25)
        for name in ("B", "A"):
            p_hi, p_lo, occ = planes[name]
            ref = plain.forward(p_hi, p_lo, occ=occ, work=st_p, in_entry=entry)
            got = fused.forward(p_hi, p_lo, occ=occ, work=st_f, in_entry=entry)
            assert torch.equal(got, ref), name + " (after the weight change)"
            assert not torch.equal(ref, want[name])
        after = fused.background_head(h, w, dev)
        assert after.data_ptr() == where and not torch.equal(after, before)

"""tests/dense_train_cases.py on the host: every case hits the tile arithmetic it claims; the integer, one-hot and split cases meet the
conditions under which the kernels' bf16 / fp32 results are exact; a float32 torch model of every operation keeps half of the accumulation
part of every real-valued bar; and a table of planted mistakes -- each written as an alternative CPU result -- shows which named case rejects
which mistake.  A planted mistake that no case notices means a case is missing.  No GPU."""
import numpy as np
import pytest
import torch

import dense_train_cases as dc

C = dc.C
sid = lambda s: "x".join(map(str, s))  # noqa: E731


# ------------------------------------------------------------------------------------------------ the claimed tile arithmetic
def test_every_case_hits_the_tile_arithmetic_it_claims():
    assert set(dc.CONV_CLAIMS) == set(dc.CONV_SHAPES) and set(dc.WGRAD_CLAIMS) == set(dc.WGRAD_SHAPES)
    for claims, arith in ((dc.CONV_CLAIMS, dc.conv_arith), (dc.WGRAD_CLAIMS, dc.wgrad_arith)):
        for shape, claim in claims.items():
            got = arith(*shape)
            assert {k: got[k] for k in claim} == claim, (shape, got)
    for spec, claim in dc.HEAD_CLAIMS.items():
        got = dc.head_arith(*spec[1:])
        assert {k: got[k] for k in claim} == claim, (spec, got)
    # 17 x 17: workgroup 0 owns tiles 0 and 3; 3x17x33: an image boundary inside a workgroup's tile list and inside a 128-pixel run
    owner, tile = dc.conv_owner(1, 17, 17, 3)
    assert sorted(set(tile[owner == 0])) == [0, 3] and tile[0, 16, 16] == 3
    owner, tile = dc.conv_owner(3, 17, 33, 3)
    assert any(len({t // 6 for t in set(tile[owner == g])}) == 2 for g in range(14)), "a workgroup with tiles of two images"
    owner, run = dc.conv_owner(3, 17, 33, 1)
    assert any(len(set(np.nonzero(run == r)[0])) == 2 for r in range(14)), "a run with pixels of two images"
    a = dc.conv_arith(1, 1, 4113)
    assert sorted({(a["tiles"] - 1 - g) // a["workgroups"] + 1 for g in range(a["workgroups"])}) == [7, 8]
    # the small head cases put M one under, at and one over a 64-pixel chunk and a 256-pixel block, as one image and as two
    assert {dc.head_arith(b, h, w)["M"] for _, b, h, w in dc.HEAD_SMALL if b == 1} == set(dc.HEAD_M)
    assert {o for o, _, _, _ in dc.HEAD_SMALL} == {8, 16, 24, 32, 48, 64}
    assert dc.HEAD_CLAIMS[dc.HEAD_TRIP_W]["M"] == 1024 * 64 + 65 and dc.HEAD_CLAIMS[dc.HEAD_TRIP_FD]["M"] == 2048 * 256 + 302


# ------------------------------------------------------------------------------------------------ exactness conditions
@pytest.mark.parametrize("ksize", [3, 1])
@pytest.mark.parametrize("shape", dc.CONV_SHAPES, ids=sid)
def test_integer_convolution_cases_are_exact_in_bf16_and_fp32(shape, ksize):
    B, H, W = shape
    for kind in ("int", "onehot") if shape in dc.ONEHOT_SHAPES else ("int",):
        c = dc.conv_case(shape, ksize, kind)
        if kind == "int":
            assert (c["x"][np.broadcast_to(dc.seam_mask(B, H, W), c["x"].shape)] != 0).all(), "x dense at borders and seams"
            assert set(np.unique(c["x"])) <= {-1, 0, 1} and set(np.unique(c["w"])) == {-1, 0, 1}
            assert 1 / 20 < (c["w"] != 0).mean() < 1 / 13
        owner, _ = dc.conv_owner(B, H, W, ksize)
        for transpose in (0, 1):
            y, _ = dc.conv_reference(c["x"], c["w"], transpose)
            assert np.array_equal(y, np.rint(y)) and np.abs(y).max() <= 256, "an integer of at most 256: exact in bf16"
            assert np.array_equal(dc.bf16(y), y)
            assert y.any()
            _, mag, _ = dc.stats_rows(y, owner, c["arith"]["workgroups"])
            assert mag.max() < 2 ** 24, "the statistics are exact in fp32 in any order"


def test_the_one_hot_cases_spell_out_the_taps():
    c = dc.conv_case((1, 3, 3), 3, "onehot")
    y, _ = dc.conv_reference(c["x"], c["w"], 0)
    # the centre sees the four corners through taps 0, 2, 6, 8 (weights 1, 3, 7, 9); the pixel right of corner (0, 0) sees it through tap 3
    assert y[0, 1, 1, dc.CO] == 1 + 3 + 7 + 9 and y[0, 0, 1, dc.CO] == 4 + 6 and not np.delete(y, dc.CO, -1).any()
    yt, _ = dc.conv_reference(c["x"], c["w"], 1)
    assert yt[0, 0, 1, dc.CI] == 6 + 4 and yt[0, 1, 0, dc.CI] == 8 + 2 and y[0, 1, 0, dc.CO] == 2 + 8 and not np.delete(yt, dc.CI, -1).any()
    c = dc.conv_case((1, 1, 4), 3, "onehot")
    y, _ = dc.conv_reference(c["x"], c["w"], 0)
    yt, _ = dc.conv_reference(c["x"], c["w"], 1)
    assert y[0, 0, :, dc.CO].tolist() == [5, 4, 6, 5] and yt[0, 0, :, dc.CI].tolist() == [5, 6, 4, 5], "flipped taps"


@pytest.mark.parametrize("shape", dc.WGRAD_SHAPES, ids=sid)
def test_integer_and_split_weight_gradient_cases_are_exact_in_fp32(shape):
    pixels = shape[0] * shape[1] * shape[2]
    c = dc.wgrad_case(shape, "int")
    assert set(np.unique(c["x"])) <= {-1, 0, 1} and pixels < 2 ** 24, "every partial sum is an integer below 2^24"
    for kind in dc.SPLIT_KINDS:
        c = dc.wgrad_case(shape, kind)
        for t, has_lo in (("x", kind != "dy_lo"), ("dy", kind != "x_lo")):
            assert set(np.unique(c[t + "_hi"])) <= {-32, -16, 16, 32}
            assert set(np.unique(c[t + "_lo"])) <= ({-1, 1} if has_lo else {0})
        # every product of the three terms is a multiple of 16 of magnitude <= 32 * 32, 32 * 1, 1 * 32
        assert pixels * (32 * 32 + 32 + 32) // 16 < 2 ** 24, "the sum of all three terms over all pixels, in units of 16"
    for ksize in (3, 1):
        c = dc.wgrad_case(shape, "both")
        terms = dc.wgrad_split_terms(c, ksize)
        assert all(np.array_equal(t, 16 * np.rint(t / 16)) for t in terms)
        exact, _ = dc.wgrad_reference(c["x_hi"] + c["x_lo"], c["dy_hi"] + c["dy_lo"], ksize)
        lolo, _ = dc.wgrad_reference(c["x_lo"], c["dy_lo"], ksize)
        assert np.array_equal(sum(terms), exact - lolo) and lolo.any(), "the exact product minus lo * lo"


@pytest.mark.parametrize("spec", dc.HEAD_SMALL[::5] + [dc.HEAD_TRIP_W], ids=lambda s: "O%d-%dx%dx%d" % s)
def test_integer_head_cases_are_exact(spec):
    c = dc.head_case(spec, "int")
    ref = dc.head_reference(c)
    for k in ("maps", "dw", "db"):
        assert ref[k][1].max() < 2 ** 24
    assert np.abs(ref["dfeat"][0]).max() <= 256 and ref["dfeat"][1].max() < 2 ** 24


def test_the_largest_integer_head_case_is_exact_by_its_bounds():
    O, B, H, W = dc.HEAD_TRIP_FD
    c = dc.head_case(dc.HEAD_TRIP_FD, "int")
    for k in ("feat", "w", "dmaps"):
        assert np.abs(c[k]).max() == 1
    assert np.abs(c["bias"]).max() <= 2 and C + 2 < 2 ** 24 and O <= 256 and B * H * W < 2 ** 24


# ------------------------------------------------------------------------------------------------ a float32 model keeps half of each bar
def share(n):
    """the part of an n-term bar a float32 model may use: half of it -- from 8 terms on.  A pairwise fp32 sum of n terms rounds
    log2(n) + 1 times on any path, which is at most n / 2 from n = 8; below that (one pixel: ONE rounding against a bar of one u) the
    model may need the whole bar."""
    return 0.5 if n >= 8 else 1.0


@pytest.mark.parametrize("ksize", [3, 1])
@pytest.mark.parametrize("shape", dc.CONV_SHAPES, ids=sid)
def test_a_float32_convolution_keeps_half_of_the_accumulation_bar(shape, ksize):
    """(before its rounding to bf16: the rounding is the bar's other term, half an ulp by itself)"""
    c = dc.conv_case(shape, ksize, "real")
    for transpose in (0, 1):
        want, mag = dc.conv_reference(c["x"], c["w"], transpose)
        y32, _ = dc.conv_reference(c["x"], c["w"], transpose, dtype=torch.float32)
        assert dc.fraction(y32, want, dc.fp32_bar(mag, C * ksize * ksize)) <= 0.5
        # and the rounded result keeps the whole bar
        assert dc.fraction(dc.bf16(y32), want, dc.bf16_bar(want, mag, C * ksize * ksize)) <= 1


@pytest.mark.parametrize("shape", dc.WGRAD_SHAPES, ids=sid)
def test_a_float32_weight_gradient_keeps_half_of_the_bar(shape):
    c = dc.wgrad_case(shape, "real")
    for ksize in (3, 1):
        want, mag = dc.wgrad_reference(c["x"], c["dy"], ksize)
        got, _ = dc.wgrad_reference(c["x"], c["dy"], ksize, dtype=torch.float32)
        assert dc.fraction(got, want, dc.fp32_bar(mag, shape[0] * shape[1] * shape[2])) <= share(shape[0] * shape[1] * shape[2])


@pytest.mark.parametrize("spec", dc.HEAD_SMALL[::5] + [dc.HEAD_TRIP_W], ids=lambda s: "O%d-%dx%dx%d" % s)
def test_a_float32_head_keeps_half_of_the_bars(spec):
    c = dc.head_case(spec, "real")
    want, got = dc.head_reference(c), dc.head_reference(c, dtype=torch.float32)
    n = dict(maps=C + 1, dfeat=c["O"], dw=c["arith"]["M"], db=c["arith"]["M"])
    for k in n:
        assert dc.fraction(got[k][0], want[k][0], dc.fp32_bar(want[k][1], n[k])) <= share(n[k]), k


def test_the_bars():
    assert dc.half_ulp_bf16(np.array([1.0, 1.99, 2.0, -3.0, 0.0, 0.75])).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 0.0, 2.0 ** -9]
    assert dc.fraction(np.array([1.0, 0.0]), np.array([1.0, 0.0]), np.array([0.0, 0.0])) == 0
    assert dc.fraction(np.array([1.0]), np.array([1.5]), np.array([0.0])) == np.inf


# ------------------------------------------------------------------------------------------------ planted mistakes
def taps_conv(x, w, transpose, halo="checked", flip=True, swap=True):
    """the convolution tap by tap, ONLY to state mistakes with (it equals torch without one: asserted below).
    halo: "checked" | "row" (flattened m + dx with no column check) | "image" (rows taken from the neighbouring image)"""
    B, H, W, _ = x.shape
    k = w.shape[-1]
    b, h, wq = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    flat = np.concatenate([x.reshape(-1, C).astype(np.float64), np.zeros((1, C))])
    y = np.zeros((B, H, W, C))
    for ty in range(k):
        for tx in range(k):
            dy, dx = ty - k // 2, tx - k // 2
            if not transpose:
                m = w[:, :, ty, tx].T
            else:
                a = w[:, :, k - 1 - ty, k - 1 - tx] if flip else w[:, :, ty, tx]
                m = a if swap else a.T
            hh, ww = h + dy, wq + dx
            rows_ok = (hh >= 0) & (hh < H)
            if halo == "image":
                rows_ok = (b * H + hh >= 0) & (b * H + hh < B * H)
            ok = rows_ok & ((ww >= 0) & (ww < W) if halo != "row" else (hh * W + ww >= 0) & (hh * W + ww < H * W))
            src = np.where(ok, (b * H + hh) * W + ww, B * H * W)
            y += flat[src] @ m.astype(np.float64)
    return y


def _conv(shape, ksize, kind, transpose):
    c = dc.conv_case(shape, ksize, kind)
    return c, dc.conv_reference(c["x"], c["w"], transpose)[0]


def m_halo_row():
    c, want = _conv((1, 17, 17), 3, "int", 0)
    return c["name"], want, taps_conv(c["x"], c["w"], 0, halo="row")


def m_halo_image():
    c, want = _conv((3, 17, 33), 3, "int", 0)
    return c["name"], want, taps_conv(c["x"], c["w"], 0, halo="image")


def m_no_flip():
    c, want = _conv((1, 1, 4), 3, "onehot", 1)  # (3 x 3 with its four corners set is symmetric under the flip: it would not notice)
    return c["name"], want, taps_conv(c["x"], c["w"], 1, flip=False)


def m_no_swap():
    c, want = _conv((1, 1, 4), 1, "onehot", 1)
    return c["name"], want, taps_conv(c["x"], c["w"], 1, swap=False)


def m_no_swap_int():
    c, want = _conv((1, 16, 17), 3, "int", 1)
    return c["name"], want, taps_conv(c["x"], c["w"], 1, swap=False)


def m_second_tile_at_first_origin():
    c, want = _conv((1, 17, 17), 3, "int", 0)
    alt = want.copy()
    alt[0, 16:17, 16:17] = want[0, 0:1, 0:1]  # tile 3 (origin 16, 16, one valid pixel) computed at tile 0's origin
    return c["name"], want, alt


def m_last_ragged_tile_dropped():
    c, want = _conv((1, 17, 17), 3, "int", 0)
    alt = want.copy()
    alt[0, 16:, 16:] = 0
    return c["name"], want, alt


def m_last_run_dropped():
    c, want = _conv((3, 17, 33), 1, "int", 0)
    alt = want.reshape(-1, C).copy()
    alt[13 * 128:] = 0
    return c["name"], want.reshape(-1, C), alt


def _stats(c, y, ksize):
    B, H, W = c["shape"]
    return dc.stats_rows(y, dc.conv_owner(B, H, W, ksize)[0], c["arith"]["workgroups"])[0]


def m_stats_with_invalid_pixels():
    c, want = _conv((1, 17, 17), 3, "int", 0)
    xe = np.zeros((1, 32, 32, C), np.float32)
    xe[:, :17, :17] = c["x"]
    ye, _ = dc.conv_reference(xe, c["w"], 0)  # what the kernel's accumulators hold for the pixels outside the image
    h, w = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    owner = ((h // 16) * 2 + w // 16)[None] % 3
    return c["name"], _stats(c, want, 3), dc.stats_rows(ye, owner, 3)[0]


def m_stats_without_last_tile():
    c, want = _conv((1, 17, 17), 3, "int", 0)
    cut = want.copy()
    cut[0, 16:, 16:] = 0
    return c["name"], _stats(c, want, 3), _stats(c, cut, 3)


def m_slab_64_tile_dropped():
    c = dc.wgrad_case((1, 8, 1040), "int")
    want, _ = dc.wgrad_reference(c["x"], c["dy"], 3)
    dy = c["dy"].copy()
    dy[:, :, 1024:] = 0  # tile 64, the second tile of slab 0
    return c["name"], want, dc.wgrad_reference(c["x"], dy, 3)[0]


def _split_without(term):
    c = dc.wgrad_case((1, 8, 1040), "both")
    terms = dc.wgrad_split_terms(c, 3)
    return c["name"], sum(terms), sum(terms) - terms[term]


def _split_term_twice():
    c = dc.wgrad_case((1, 8, 1040), "both")
    t = dc.wgrad_split_terms(c, 3)
    return c["name"], sum(t), t[0] + 2 * t[1]  # hi*lo in the place of lo*hi: a wrong term offset in the partials


def m_split_one_sided(kind, term):
    """the cases with ONE lo plane: the term that carries it, dropped"""
    c = dc.wgrad_case((3, 9, 17), kind)
    terms = dc.wgrad_split_terms(c, 1)
    return c["name"], sum(terms), sum(terms) - terms[term]


def _head_dw_without(spec, first_dropped):
    c = dc.head_case(spec, "int")
    ref = dc.head_reference(c)
    B, H, W = c["shape"]
    g = c["dmaps"].transpose(0, 2, 3, 1).reshape(-1, c["O"])[first_dropped:].astype(np.float64)
    f = c["feat"].reshape(-1, C)[first_dropped:].astype(np.float64)
    return c["name"], (ref["dw"][0], ref["db"][0]), (ref["dw"][0] - g.T @ f, ref["db"][0] - g.sum(0))


def m_head_short_chunk_dropped(which):
    name, want, alt = _head_dw_without((16, 1, 1, 65), 64)
    return name, want[which], alt[which]


def m_head_weight_second_trip_dropped(which):
    name, want, alt = _head_dw_without(dc.HEAD_TRIP_W, 65536)
    return name, want[which], alt[which]


def m_head_second_trip_dropped(which):
    """per pixel: only the pixels of the second trip need a reference"""
    c = dc.head_case(dc.HEAD_TRIP_FD, "int")
    O, first = c["O"], 2048 * 256
    if which == "maps":
        want = c["feat"].reshape(-1, C)[first:].astype(np.float64) @ c["w"].T.astype(np.float64) + c["bias"]
    else:
        want = c["dmaps"].transpose(0, 2, 3, 1).reshape(-1, O)[first:].astype(np.float64) @ c["w"].astype(np.float64)
    return c["name"], want, np.zeros_like(want)


MISTAKES = {
    "halo taken from the neighbouring row (flattened m + dx, no column check)": m_halo_row,
    "halo taken from the previous image": m_halo_image,
    "tap flip omitted in the data gradient": m_no_flip,
    "channel swap omitted in the data gradient (one-hot)": m_no_swap,
    "channel swap omitted in the data gradient (integer)": m_no_swap_int,
    "a workgroup's second tile computed at the first tile's origin": m_second_tile_at_first_origin,
    "the last ragged tile dropped": m_last_ragged_tile_dropped,
    "the last ragged run of the 1x1 kernel dropped": m_last_run_dropped,
    "statistics that include the invalid pixels of a ragged tile": m_stats_with_invalid_pixels,
    "statistics that omit the last tile": m_stats_without_last_tile,
    "slab 64's tile dropped": m_slab_64_tile_dropped,
    "split term hi*hi dropped": lambda: _split_without(0),
    "split term hi*lo dropped": lambda: _split_without(1),
    "split term lo*hi dropped": lambda: _split_without(2),
    "split term hi*lo taken twice in the place of lo*hi": _split_term_twice,
    "split term hi*lo dropped where only dY carries a lo plane": lambda: m_split_one_sided("dy_lo", 1),
    "split term lo*hi dropped where only x carries a lo plane": lambda: m_split_one_sided("x_lo", 2),
    "the head's last short chunk dropped from dW": lambda: m_head_short_chunk_dropped(0),
    "the head's last short chunk dropped from db": lambda: m_head_short_chunk_dropped(1),
    "the head's weight kernel's second trip dropped from dW": lambda: m_head_weight_second_trip_dropped(0),
    "the head's weight kernel's second trip dropped from db": lambda: m_head_weight_second_trip_dropped(1),
    "the head's second trip dropped from the maps": lambda: m_head_second_trip_dropped("maps"),
    "the head's second trip dropped from dfeat": lambda: m_head_second_trip_dropped("dfeat"),
}


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_a_named_case_rejects_every_planted_mistake(mistake):
    name, want, alt = MISTAKES[mistake]()
    assert want.shape == alt.shape
    assert not np.array_equal(want, alt), f"{mistake}: {name} does not notice it"
    print(f"{mistake}: rejected by {name}, {int((want != alt).sum())} of {want.size} elements differ")


@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("shape,ksize", [((1, 17, 17), 3), ((3, 17, 33), 3), ((1, 3, 3), 3), ((1, 1, 4), 1)], ids=str)
def test_the_mistake_free_tap_model_is_torchs_convolution(shape, ksize, transpose):
    for kind in ("int", "onehot"):
        c, want = _conv(shape, ksize, kind, transpose)
        assert np.array_equal(taps_conv(c["x"], c["w"], transpose), want)


def test_the_w_gate_of_why_unsupported_is_stated():
    """W in {1, 3} run through the raw bf16 calls (conv shapes 1x1x1, 1x3x3 on the GPU): the gate's reason is in the docstring"""
    from vision3d_amd import dense_train
    assert "W >= 4" in dense_train.why_unsupported.__doc__

"""The dense RPN's per-frame tile schedule, restated in numpy (csrc/dense_conv.hip: d2_tile_near, d2_build_schedule).
A 5 x 16 tile of a layer with cumulative reach R is LIVE when an occupied BEV pixel lies within R (Chebyshev) of one of its pixels:
dilate the occupancy by R, clipped to the image, and take any-per-tile.  Tiles are numbered (b, ty, tx).  A dead tile whose state
word is still nonzero is STALE: it holds an earlier frame's computed values and gets the background copy."""
import numpy as np

TH, TW = 5, 16


def n_tiles(b, h, w):
    return b * ((h + TH - 1) // TH) * ((w + TW - 1) // TW)


def dilate(occ, reach):
    """bool (b, h, w) -> bool (b, h, w): pixels within `reach` (Chebyshev) of an occupied one, clipped to the image"""
    b, h, w = occ.shape
    out = np.zeros_like(occ)
    for dy in range(-reach, reach + 1):
        for dx in range(-reach, reach + 1):
            ys, yd = slice(max(0, -dy), min(h, h - dy)), slice(max(0, dy), min(h, h + dy))
            xs, xd = slice(max(0, -dx), min(w, w - dx)), slice(max(0, dx), min(w, w + dx))
            out[:, yd, xd] |= occ[:, ys, xs]
    return out


def live_tiles(occ, reach):
    """bool (b, h, w) -> bool (n_tiles,): any-per-tile of the dilated map"""
    b, h, w = occ.shape
    near = dilate(occ, reach)
    ty, tx = (h + TH - 1) // TH, (w + TW - 1) // TW
    pad = np.zeros((b, ty * TH, tx * TW), dtype=bool)
    pad[:, :h, :w] = near
    return pad.reshape(b, ty, TH, tx, TW).any(axis=(2, 4)).reshape(-1)


def schedule(occ, reach, state):
    """-> (live[], stale[]) as the builder writes them: increasing tile index; `state`: the layer's words before the frame"""
    live = live_tiles(occ, reach)
    stale = ~live & (np.asarray(state[:live.size]) != 0)
    return np.flatnonzero(live), np.flatnonzero(stale)


def occupancy_words(occ):
    """bool (b, h, w) -> the inverted bitmap (b * h, ceil(w / 32)) uint32: bit x % 32 of word x // 32 is 0 where occupied"""
    b, h, w = occ.shape
    words = np.full((b * h, (w + 31) // 32), 0xFFFFFFFF, dtype=np.uint32)
    for bb, yy, xx in zip(*np.nonzero(occ)):
        words[bb * h + yy, xx // 32] &= ~np.uint32(1 << (xx % 32))
    return words


def live_tiles_brute(occ, reach):
    """the same by definition: per tile, per pixel of the tile, the Chebyshev distance to every occupied pixel"""
    b, h, w = occ.shape
    ty, tx = (h + TH - 1) // TH, (w + TW - 1) // TW
    out = np.zeros(b * ty * tx, dtype=bool)
    for bb in range(b):
        pts = np.argwhere(occ[bb])
        for t_y in range(ty):
            for t_x in range(tx):
                hit = False
                for yy in range(t_y * TH, min(t_y * TH + TH, h)):
                    for xx in range(t_x * TW, min(t_x * TW + TW, w)):
                        if len(pts) and (np.maximum(np.abs(pts[:, 0] - yy), np.abs(pts[:, 1] - xx)) <= reach).any():
                            hit = True
                out[(bb * ty + t_y) * tx + t_x] = hit
    return out

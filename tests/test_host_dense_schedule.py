"""Host: the numpy restatement of the dense RPN's tile schedule (dense_schedule_ref.py) against the definition -- a brute-force
per-pixel Chebyshev distance -- on a handful of tiny maps.  No GPU."""
import numpy as np
import pytest

import dense_schedule_ref as R


def _maps():
    rng = np.random.default_rng(3)
    out = {}
    out["empty"] = np.zeros((1, 12, 40), dtype=bool)
    out["full"] = np.ones((1, 7, 20), dtype=bool)
    c = np.zeros((2, 12, 40), dtype=bool)
    c[0, 0, 0] = c[0, 0, 39] = c[1, 11, 0] = c[1, 11, 39] = True
    out["corners"] = c
    for d in (1, 2, 3, 4):
        e = np.zeros((1, 12, 40), dtype=bool)
        e[0, 2, 15 + d] = True  # d cells right of tile (0, 0)'s last column
        out[f"edge x {d}"] = e
        e = np.zeros((1, 12, 40), dtype=bool)
        e[0, 4 + d, 3] = True   # d cells below tile (0, 0)'s last row
        out[f"edge y {d}"] = e
    out["random"] = rng.random((2, 11, 35)) < 0.03
    return out


@pytest.mark.parametrize("name", sorted(_maps()))
@pytest.mark.parametrize("reach", [0, 1, 2, 3, 6])
def test_restatement_is_the_definition(name, reach):
    occ = _maps()[name]
    assert np.array_equal(R.live_tiles(occ, reach), R.live_tiles_brute(occ, reach))


def test_the_liveness_edge():
    """a pixel d cells from tile 0's edge: the tile is live from reach d on"""
    for axis in ("x", "y"):
        for d in (1, 2, 3, 4):
            occ = _maps()[f"edge {axis} {d}"]
            for reach in (1, 2, 3):
                assert bool(R.live_tiles(occ, reach)[0]) == (reach >= d), (axis, d, reach)


def test_schedule_lists_and_bitmap():
    occ = np.zeros((1, 12, 40), dtype=bool)
    occ[0, 11, 39] = True
    state = np.array([1, 0, 1, 0, 1, 0, 1, 0, 1])
    live, stale = R.schedule(occ, 1, state)
    assert live.tolist() == [8] and stale.tolist() == [0, 2, 4, 6]  # (rows 10-11 are tile row 2, columns 38-39 tile column 2)
    live, _ = R.schedule(occ, 2, state)
    assert live.tolist() == [5, 8]                                   # (row 9 is tile row 1)
    live, _ = R.schedule(occ, 8, state)
    assert live.tolist() == [1, 2, 4, 5, 7, 8]                       # (rows 3-11, columns 31-39)
    words = R.occupancy_words(occ)
    assert words.shape == (12, 2) and words[11, 1] == 0xFFFFFFFF & ~(1 << 7) and (words[:11] == 0xFFFFFFFF).all() and words[11, 0] == 0xFFFFFFFF

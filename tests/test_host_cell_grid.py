"""CPU: the grid-shape rule and the cell coordinate of the cell grids (vision3d_amd/csrc/cell_grid_device.h) compiled for the host
with g++: the rule ends within its stated bound on every input (extents that overflow float32 included) with every key in range,
equals the rule the ball query had before (restated here in numpy float32) wherever that one ends, and two values less than a
radius apart lie at most one cell apart.  The GPU runs of the same header are tests/test_gpu_pointops.py (ball query) and
tests/test_gpu_vector_pool.py (VectorPool search)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32


@pytest.fixture(scope="module")
def cg():
    so = os.path.join(HERE, "host", "_build", "libcell_grid_host.so")
    src = os.path.join(HERE, "host", "cell_grid_host_shim.cpp")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-std=c++17", "-o", so, src])
    lib = C.CDLL(so)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    class Host:
        MAX_KEYS, SHAPE_STEPS = lib.host_cg_constants(0), lib.host_cg_constants(1)

        @staticmethod
        def shape(bounds, cell_min, n, max_chunks):
            """bounds (k, 4) = xlo, xhi, ylo, yhi -> dict of (k,) arrays: x0, y0, inv_c, nx, ny, nch, chunk, steps."""
            bounds = np.ascontiguousarray(bounds, F)
            k = len(bounds)
            cell_min, n, max_chunks = (np.ascontiguousarray(np.broadcast_to(a, (k,)), t) for a, t in ((cell_min, F), (n, np.int32), (max_chunks, np.int32)))
            hf, hi, steps = np.empty((k, 3), F), np.empty((k, 4), np.int32), np.empty(k, np.int32)
            lib.host_cg_shape(ptr(bounds), ptr(cell_min), ptr(n), ptr(max_chunks), k, ptr(hf), ptr(hi), ptr(steps))
            return dict(x0=hf[:, 0], y0=hf[:, 1], inv_c=hf[:, 2], nx=hi[:, 0], ny=hi[:, 1], nch=hi[:, 2], chunk=hi[:, 3], steps=steps)

        @staticmethod
        def cell(x, x0, inv_c):
            x = np.ascontiguousarray(x, F)
            x0, inv_c = (np.ascontiguousarray(np.broadcast_to(a, x.shape), F) for a in (x0, inv_c))
            out = np.empty(x.shape, F)
            lib.host_cg_cell(ptr(x), ptr(x0), ptr(inv_c), x.size, ptr(out))
            return out
    return Host


def _axis(rng, extent):
    """(lo, hi) of one axis as float32: hi - lo is `extent` up to rounding, inf for extent = inf."""
    if extent == np.inf:
        return F(-3e38), F(3e38)
    if extent >= 1e38:
        return F(-1e38), F(extent - 1e38)
    lo = F(rng.uniform(-100.0, 100.0))
    return lo, F(lo + F(extent))


def _sweep():
    """-> bounds (k, 4), cell_min (k,), N (k,), max_chunks (k,): every combination of the extents along x and y, 13 cell sizes a
    decade apart times a seeded factor in [1, 10), max_chunks and N."""
    rng = np.random.default_rng(2024)
    extents = (0.0, 1e-3, 100.0, 1e6, 3e38, np.inf)
    rows = []
    for ex, ey, e, mc, n in itertools.product(extents, extents, range(-6, 7), (1, 8), (1, 1000, 1 << 20)):
        cell_min = 10.0 ** e * (rng.uniform(1.0, 10.0) if e < 6 else 1.0)
        rows.append(_axis(rng, ex) + _axis(rng, ey) + (F(cell_min), n, mc))
    a = np.array(rows, np.float64)
    return a[:, :4].astype(F), a[:, 4].astype(F), a[:, 5].astype(np.int32), a[:, 6].astype(np.int32)


def _parent_rule(xlo, xhi, ylo, yhi, cell_min, n, limit=10000):
    """The rule of the ball query's build kernel before the shared header, float32 step for step: -> (inv_c, nx, ny, nch, chunk), or
    None where its loop has not ended after `limit` steps."""
    max_keys, max_chunks = 32768, 8
    c = F(cell_min)
    with np.errstate(all="ignore"):
        for _ in range(limit):
            inv_c = F(1.0) / c
            fx, fy = np.floor((xhi - xlo) * inv_c), np.floor((yhi - ylo) * inv_c)
            if fx < F(max_keys) and fy < F(max_keys) and (int(fx) + 1) * (int(fy) + 1) <= max_keys:
                nx, ny = int(fx) + 1, int(fy) + 1
                nch = min(max_chunks, max_keys // (nx * ny))
                return inv_c, nx, ny, nch, (n + nch - 1) // nch
            c = c * F(1.5)
    return None


def test_shape_rule_ends_with_every_key_in_range(cg):
    bounds, cell_min, n, mc = _sweep()
    h = cg.shape(bounds, cell_min, n, mc)
    assert cg.SHAPE_STEPS == 512 and cg.MAX_KEYS == 32768
    assert (h["steps"] >= 0).all() and (h["steps"] <= cg.SHAPE_STEPS).all()
    assert (h["nx"] >= 1).all() and (h["ny"] >= 1).all()
    assert (h["nx"].astype(np.int64) * h["ny"] * h["nch"] <= cg.MAX_KEYS).all()
    assert (h["nch"] >= 1).all() and (h["nch"] <= mc).all() and (h["nch"].astype(np.int64) * h["chunk"] >= n).all()
    assert np.array_equal(h["x0"].view(np.uint32), bounds[:, 0].view(np.uint32)) and np.array_equal(h["y0"].view(np.uint32), bounds[:, 2].view(np.uint32))
    # the largest and the smallest coordinate of each axis: the last and the first cell, so every key is in range
    assert np.array_equal(cg.cell(bounds[:, 1], h["x0"], h["inv_c"]), (h["nx"] - 1).astype(F))
    assert np.array_equal(cg.cell(bounds[:, 3], h["y0"], h["inv_c"]), (h["ny"] - 1).astype(F))
    assert (cg.cell(bounds[:, 0], h["x0"], h["inv_c"]) == 0).all() and (cg.cell(bounds[:, 2], h["y0"], h["inv_c"]) == 0).all()
    # cells no smaller than asked for (1 / c is monotone in c), unless the single cell was given
    single = h["inv_c"] == 0
    assert (h["inv_c"][~single] <= F(1.0) / cell_min[~single]).all() and (h["inv_c"] >= 0).all()
    # the single cell: exactly where an extent overflows, one cell and one chunk; every finite value lies in cell 0
    with np.errstate(over="ignore"):
        overflow = ~np.isfinite(bounds[:, 1] - bounds[:, 0]) | ~np.isfinite(bounds[:, 3] - bounds[:, 2])
    assert overflow.any() and np.array_equal(single, overflow)
    assert (h["nx"][single] == 1).all() and (h["ny"][single] == 1).all() and (h["nch"][single] == 1).all()
    assert np.array_equal(h["chunk"][single], n[single])
    probe = np.array([-3.4e38, -3e38, -1.0, 0.0, 1e-30, 70.4, 3e38, 3.4e38], F)
    assert (cg.cell(probe, F(-3e38), F(0.0)) == 0).all() and (cg.cell(probe, F(3e38), F(0.0)) == 0).all()


def test_shape_rule_of_a_frame_without_points_and_of_a_cell_that_cannot_grow(cg):
    inf = np.inf
    h = cg.shape([[inf, -inf, inf, -inf]], 0.4, 100, 8)
    assert (h["nx"][0], h["ny"][0], h["nch"][0], h["chunk"][0], h["inv_c"][0], h["steps"][0]) == (0, 0, 1, 100, 0.0, 0)
    # cells of 0, below 0 and NaN would never grow: the single cell at once
    h = cg.shape([[0.0, 50.0, 0.0, 50.0]] * 3, [0.0, -1.0, np.nan], 100, 8)
    assert (h["steps"] <= cg.SHAPE_STEPS).all() and (h["nx"] == 1).all() and (h["ny"] == 1).all() and (h["nch"] == 1).all() and (h["inv_c"] == 0).all()


def test_shape_rule_equals_the_ball_querys_earlier_rule(cg):
    bounds, cell_min, n, mc = _sweep()
    keep = mc == 8
    bounds, cell_min, n = bounds[keep], cell_min[keep], n[keep]
    h = cg.shape(bounds, cell_min, n, 8)
    ended = 0
    for i, (b, c, k) in enumerate(zip(bounds, cell_min, n)):
        want = _parent_rule(b[0], b[1], b[2], b[3], c, int(k))
        if want is None:
            continue
        ended += 1
        assert F(want[0]).view(np.uint32) == h["inv_c"][i].view(np.uint32), (b, c, k)
        assert want[1:] == (h["nx"][i], h["ny"][i], h["nch"][i], h["chunk"][i]), (b, c, k)
    with np.errstate(over="ignore"):
        finite = np.isfinite(bounds[:, 1] - bounds[:, 0]) & np.isfinite(bounds[:, 3] - bounds[:, 2])
    assert ended == finite.sum() > 0  # (the earlier rule ends on every finite extent, and on no other)


@pytest.mark.parametrize("lo,hi", [((0.0, -40.0), (70.4, 40.0)), ((-75.2, -75.2), (75.2, 75.2))], ids=["kitti", "waymo"])
def test_values_less_than_a_radius_apart_lie_at_most_one_cell_apart(cg, lo, hi):
    """What the 3 x 3 walk of the ball query rests on: cells of 1.01 r (grown where the range needs more than 32 768 of them), the
    bounds as the origin, pairs |a - b| < r anywhere in the range."""
    rng = np.random.default_rng(31)
    for r in (0.2, 0.4, 0.8, 1.2, 2.4, 4.8):
        cell_min = F(r) * F(1.01)  # (as v3d_ball_query_grid_build states it)
        bounds = np.array([[lo[0] + rng.uniform(0, 1), hi[0], lo[1] + rng.uniform(0, 1), hi[1]]], F)
        h = cg.shape(bounds, cell_min, 16384, 8)
        assert h["inv_c"][0] > 0
        for axis, (x0, n_cells) in enumerate(((h["x0"][0], h["nx"][0]), (h["y0"][0], h["ny"][0]))):
            a = rng.uniform(bounds[0, 2 * axis], bounds[0, 2 * axis + 1], 200000).astype(F)
            d = rng.uniform(-r, r, a.shape)
            d[::2] = np.sign(d[::2]) * r * (1.0 - rng.uniform(0, 1e-3, d[::2].shape))  # every other pair: just inside the radius
            b = np.clip((a + d).astype(F), bounds[0, 2 * axis], bounds[0, 2 * axis + 1])
            near = np.abs(a.astype(np.float64) - b.astype(np.float64)) < float(F(r))
            assert near.mean() > 0.9
            ca, cb = cg.cell(a[near], x0, h["inv_c"][0]), cg.cell(b[near], x0, h["inv_c"][0])
            assert (np.abs(ca - cb) <= 1).all() and ca.min() >= 0 and ca.max() <= n_cells - 1

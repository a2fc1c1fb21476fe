"""tests/geometry_ref.py (the plain numpy restatement the GPU edge tests compare against) checked three ways, without a GPU:
hand-worked cases whose expected tables are written out below, the C oracle on every case of tests/geometry_cases.py that it can
state, and each case builder for the property that gives it its name.

Left out of the oracle comparison: "bad_batch" (the oracle knows no batch limit; checked against the reference on the valid rows
alone) and the capped runs of the strided builder (the oracle has no cap_out; checked as a prefix of the uncapped tables).  No
stride-1 case is left out: oracle.sparse_rulebook holds 8 * n outputs and the densest case here creates fewer than 4 * n.
"""
import functools

import numpy as np
import pytest

import geometry_cases as cases
import geometry_ref as ref

eq = np.testing.assert_array_equal


# ------------------------------------------------------------------------------------------------ hand-worked cases
BLOCK = [[0, z, y, x] for z in (0, 1) for y in (0, 1) for x in (0, 1)]  # row i = 4 z + 2 y + x


def table(K, n_out, entries):
    """{output row: {kernel offset: input row}} -> (K, n_out), -1 elsewhere"""
    t = np.full((K, n_out), -1, np.int32)
    for o, col in entries.items():
        for k, i in col.items():
            t[k, o] = i
    return t


def test_hand_block_k3_s2_p1():
    """Per axis a site at 0 reaches output 0 through k = 1, a site at 1 output 1 through k = 0 and output 0 through k = 2; each site's
    smallest live offset leads to the output with the site's own coordinates, so output o is created by row o."""
    co, nbr, out_shape, overflow = ref.sparse_rulebook(BLOCK, 8, [4, 4, 4], 3, 2, 1)
    assert out_shape == [2, 2, 2] and not overflow
    eq(co, np.array(BLOCK, np.int32))
    eq(nbr, table(27, 8, {0: {13: 0, 14: 1, 16: 2, 17: 3, 22: 4, 23: 5, 25: 6, 26: 7},
                          1: {12: 1, 15: 3, 21: 5, 24: 7},
                          2: {10: 2, 11: 3, 19: 6, 20: 7},
                          3: {9: 3, 18: 7},
                          4: {4: 4, 5: 5, 7: 6, 8: 7},
                          5: {3: 5, 6: 7},
                          6: {1: 6, 2: 7},
                          7: {0: 7}}))
    eq(ref.transpose(nbr, 8, 8)[:, 7], [7, -1, 6, -1, -1, -1, 5, -1, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, 3, -1, 2, -1, -1, -1, 1, -1, 0])


def test_hand_block_k2_s2_p0():
    """The whole block is one output cell: site (z, y, x) feeds it through offset 4 z + 2 y + x."""
    co, nbr, out_shape, overflow = ref.sparse_rulebook(BLOCK, 8, [4, 4, 4], 2, 2, 0)
    assert out_shape == [2, 2, 2] and not overflow
    eq(co, [[0, 0, 0, 0]])
    eq(nbr, [[0], [1], [2], [3], [4], [5], [6], [7]])
    eq(ref.transpose(nbr, 1, 8), np.where(np.eye(8, dtype=bool), 0, -1))


def test_hand_low_corner_pad_0():
    """Without padding the corner site only has offset 0 (k > c reaches below the grid); (2, 2, 2) reaches all eight outputs, the far
    one first; (1, 0, 0) only reaches (0, 0, 0), through kz = 1."""
    rows = [[0, 0, 0, 0], [0, 2, 2, 2], [0, 1, 0, 0]]
    co, nbr, out_shape, overflow = ref.sparse_rulebook(rows, 3, [5, 5, 5], 3, 2, 0)
    assert out_shape == [2, 2, 2] and not overflow
    eq(co, [[0, 0, 0, 0], [0, 1, 1, 1], [0, 1, 1, 0], [0, 1, 0, 1], [0, 1, 0, 0], [0, 0, 1, 1], [0, 0, 1, 0], [0, 0, 0, 1]])
    eq(nbr, table(27, 8, {0: {0: 0, 26: 1, 9: 2}, 1: {0: 1}, 2: {2: 1}, 3: {6: 1}, 4: {8: 1}, 5: {18: 1}, 6: {20: 1}, 7: {24: 1}}))
    # capped at three outputs: the first three survive with their columns complete, and the flag is raised
    co3, nbr3, _, overflow3 = ref.sparse_rulebook(rows, 3, [5, 5, 5], 3, 2, 0, cap_out=3)
    assert overflow3
    eq(co3, co[:3])
    eq(nbr3, nbr[:, :3])


def test_hand_311_column():
    """A column z = 0, 1, 3 at (2, 2), a site in the next column and one in the next frame: only 0 and 1 are neighbours."""
    rows = [[0, 0, 2, 2], [0, 1, 2, 2], [0, 3, 2, 2], [0, 1, 2, 3], [1, 1, 2, 2]]
    eq(ref.subm_rulebook(rows, 5, [4, 4, 4], [3, 1, 1]), [[-1, 0, -1, -1, -1], [0, 1, 2, 3, 4], [1, -1, -1, -1, -1]])
    # the strided (3, 1, 1) / (2, 1, 1) layer: one output plane; z = 3 would reach plane 1, which out_shape cuts
    co, nbr, out_shape, overflow = ref.sparse_rulebook(rows, 5, [4, 4, 4], [3, 1, 1], [2, 1, 1], 0)
    assert out_shape == [1, 4, 4] and not overflow
    eq(co, [[0, 0, 2, 2], [0, 0, 2, 3], [1, 0, 2, 2]])
    eq(nbr, [[0, -1, -1], [1, 3, 4], [-1, -1, -1]])
    eq(ref.transpose(nbr, 3, 5), [[0, -1, -1, -1, -1], [-1, 0, -1, 1, 2], [-1, -1, -1, -1, -1]])
    # a row without a key: nobody's neighbour, finds none, keeps its centre tap; the strided builder flags it
    rows[0][0] = 64
    eq(ref.subm_rulebook(rows, 5, [4, 4, 4], [3, 1, 1]), [[-1, -1, -1, -1, -1], [0, 1, 2, 3, 4], [-1, -1, -1, -1, -1]])
    co, nbr, _, overflow = ref.sparse_rulebook(rows, 5, [4, 4, 4], [3, 1, 1], [2, 1, 1], 0)
    assert overflow
    eq(co, [[0, 0, 2, 2], [0, 0, 2, 3], [1, 0, 2, 2]])
    eq(nbr, [[-1, -1, -1], [1, 3, 4], [-1, -1, -1]])


def test_hand_two_frame_voxel_clip():
    """max_pts = 2, max_voxels = 2 on the small grid (cells of 0.1 x 0.1 x 4); every number is a binary fraction, so the means are exact.
    Frame 0 opens cells x = 0 and 1; cell 2 is a third voxel and is dropped with both its points; the third point of cell 0 is dropped
    by max_pts.  Frame 1 opens cells 2 and 3; cell 4 is dropped, 7.0 lies outside."""
    y = -3.96875
    f0 = np.array([[0.03125, y, -1, 0.5], [0.125, y, -1, 0.25], [0.0625, y, -2, 1.0], [0.25, y, -1, 0.75], [0.046875, y, 0, 0.125],
                   [0.25, y, -2, 0.5]], np.float32)
    f1 = np.array([[0.25, y, -1, 0.5], [7.0, y, -1, 0.5], [0.375, y, 0.5, 0.25], [0.4375, y, -1, 0.5], [0.25, y, -2, 1.0]], np.float32)
    vox, coords, occ, mean = ref.voxelize([f0, f1], cases.SMALL_VOXEL, cases.SMALL_BOUNDS, 2, 2)
    eq(coords, [[0, 0, 0, 0], [0, 0, 0, 1], [1, 0, 0, 2], [1, 0, 0, 3]])
    eq(occ, [2, 1, 2, 1])
    eq(vox, np.array([[[0.03125, y, -1, 0.5], [0.0625, y, -2, 1.0]],
                      [[0.125, y, -1, 0.25], [0, 0, 0, 0]],
                      [[0.25, y, -1, 0.5], [0.25, y, -2, 1.0]],
                      [[0.375, y, 0.5, 0.25], [0, 0, 0, 0]]], np.float32))
    eq(mean, np.array([[0.046875, y, -1.5, 0.75], [0.125, y, -1, 0.25], [0.25, y, -1.5, 0.75], [0.375, y, 0.5, 0.25]], np.float32))
    assert coords.dtype == np.int32 and occ.dtype == np.int32 and vox.dtype == np.float32 and mean.dtype == np.float32


# ------------------------------------------------------------------------------------------------ against the C oracle
@functools.lru_cache(maxsize=None)
def strided_ref(case, geom, cap_out=None):
    c = cases.build(case)
    n = c.get("n_live", len(c["coords"]))
    return ref.sparse_rulebook(c["coords"], n, c["shape"], *cases.STRIDED_GEOMETRIES[geom], cap_out=cap_out)


@pytest.mark.parametrize("run", cases.VOXEL_RUNS, ids=cases.VOXEL_RUN_IDS)
def test_voxelize_against_oracle(oracle, run):
    from oracle import second_cpu
    _, name, max_pts, max_voxels = run
    c = cases.build(name)
    vox, coords, occ, mean = ref.voxelize(c["frames"], c["voxel_size"], c["bounds"], max_pts, max_voxels)
    ovox, ocoords, oocc = second_cpu.voxelize_batch(c["frames"], c["voxel_size"], c["bounds"], max_pts, max_voxels)
    assert vox.shape == ovox.shape and len(coords)
    eq(vox, ovox)
    eq(coords, ocoords)
    eq(occ, oocc)
    eq(mean, oracle.vfe_mean(ovox, oocc))


@pytest.mark.parametrize("ks", cases.SUBM_KERNELS, ids=lambda ks: "k%d%d%d" % tuple(ks))
def test_subm_against_oracle(oracle, ks):
    c = cases.build("few_hundred")
    eq(ref.subm_rulebook(c["coords"], len(c["coords"]), c["shape"], ks), oracle.subm_rulebook(c["coords"], c["shape"], ks).T)


@pytest.mark.parametrize("name", ["kpt_40960", "key_range", "padded"])
def test_subm_333_against_oracle(oracle, name):
    c = cases.build(name)
    n = c.get("n_live", len(c["coords"]))
    eq(ref.subm_rulebook(c["coords"], n, c["shape"], 3), oracle.subm_rulebook(c["coords"][:n], c["shape"], 3).T)


STRIDED_RUNS = [("odd_grid", g) for g in cases.STRIDED_GEOMETRIES] + [(s, g) for s, g, _ in cases.CHUNK_RUNS] + \
               [("key_range", "k3s2p1"), ("padded", "k3s2p1")]


@pytest.mark.parametrize("case,geom", STRIDED_RUNS, ids=["%s-%s" % r for r in STRIDED_RUNS])
def test_strided_against_oracle(oracle, case, geom):
    c = cases.build(case)
    n = c.get("n_live", len(c["coords"]))
    co, nbr, out_shape, overflow = strided_ref(case, geom)
    assert len(co) <= 8 * n, "oracle.sparse_rulebook holds 8 * n outputs"
    oc, onbr, oshape = oracle.sparse_rulebook(c["coords"][:n], c["shape"], *cases.STRIDED_GEOMETRIES[geom])
    assert out_shape == oshape and not overflow
    eq(co, oc)
    eq(nbr, onbr.T)
    # the transposed table, stated entry by entry on the oracle's table
    t = ref.transpose(nbr, len(co), n)
    o, k = np.nonzero(onbr >= 0)
    assert (t >= 0).sum() == len(o)
    eq(t[k, onbr[o, k]], o)


# ------------------------------------------------------------------------------------------------ what the cases are named for
def first_touchers(c, frame=0):
    """index of the point that opens each voxel of a frame"""
    cells, kept = ref.cells_of(c["frames"][frame], c["voxel_size"], c["bounds"])
    src = np.nonzero(kept)[0]
    _, first = np.unique(cells[src], axis=0, return_index=True)
    return np.sort(src[first])


def test_voxel_case_sizes():
    for n in cases.ONE_FRAME_SIZES:
        c = cases.build(f"one_frame_{n}")
        assert [len(f) for f in c["frames"]] == [n]
        if n > 1:
            ft = first_touchers(c)
            assert ft[-1] == n - 1, "the last chunk opens a voxel"
            assert len(ft) < ref.cells_of(c["frames"][0], c["voxel_size"], c["bounds"])[1].sum(), "voxels with several points"
    c = cases.build("one_frame_66000")
    assert -(-66000 // cases.VOX_CHUNK) == 258 and (first_touchers(c) // cases.VOX_CHUNK >= 256).sum() > 10
    for name, sizes in cases.BATCH_SIZES.items():
        assert tuple(len(f) for f in cases.build(name)["frames"]) == sizes
    offs = np.cumsum(cases.BATCH_SIZES["batch_chunk_boundaries"])
    assert offs[0] % cases.VOX_CHUNK == 0 and offs[1] % cases.VOX_CHUNK == 0 and offs[3] == offs[2]
    sizes = [len(f) for f in cases.build("batch_64_frames")["frames"]]
    assert len(sizes) == 64 and min(sizes) >= 7 and max(sizes) <= 40
    xyz = cases.build("channels_4")["frames"][0][:, :3]
    for C in cases.CHANNELS:
        f = cases.build(f"channels_{C}")["frames"][0]
        assert f.shape == (700, C)
        eq(f[:, :3], xyz)


def test_voxel_clip_cases_clip():
    c = cases.build("one_frame_clip")
    ft = first_touchers(c)
    assert len(c["frames"][0]) == 2000 and len(ft) > 600
    eq(ft[:cases.CLIP_DISTINCT], np.arange(cases.CLIP_DISTINCT))  # the first chunk is all first touchers
    runs = {r[0]: r for r in cases.VOXEL_RUNS}
    assert [runs[f"one_frame_clip-mv{m}"][3] for m in (1, 255, 256, 257, 2000)] == [1, 255, 256, 257, 2000]
    for rid in ("batch_chunk_boundaries-mv3", "batch_64_frames-mv3"):
        c = cases.build(runs[rid][1])
        for b, f in enumerate(c["frames"]):
            assert len(f) < 7 or len(first_touchers(c, b)) > runs[rid][3], "every frame of at least 7 points is clipped"


def test_face_case_has_points_where_the_reciprocal_is_wrong():
    c = cases.build("face")
    pts = c["frames"][0]
    total = 0
    for axis in range(3):
        v = cases.face_candidates(axis)
        bad = v[cases.reciprocal_disagrees(v, axis)]
        total += len(bad)
        assert np.isin(bad, pts[:, axis]).all()
    assert total >= 10, total
    assert np.isin(bad, pts[:, 2]).all()
    lo, hi = np.float32(c["bounds"][:3]), np.float32(c["bounds"][3:])
    inf = np.float32(np.inf)
    for axis in range(3):  # both bounds, one ulp either side, and +-0.0 relative to lo
        for v in (lo[axis], hi[axis], np.nextafter(lo[axis], -inf), np.nextafter(lo[axis], inf), np.nextafter(hi[axis], -inf),
                  np.nextafter(hi[axis], inf)):
            assert (pts[:, axis] == v).any()
    assert (np.signbit(pts[:, 0]) & (pts[:, 0] == 0)).any() and (~np.signbit(pts[:, 0]) & (pts[:, 0] == 0)).any()
    cells, kept = ref.cells_of(pts, c["voxel_size"], c["bounds"])
    assert kept.any() and not kept.all()
    eq(ref.grid_of(c["voxel_size"], c["bounds"]), [1408, 1600, 40])
    # a voxelizer that GROUPS the points by the reciprocal's cells but labels every voxel with the quotient's cell of its first point
    # (the key wrong, the coordinates right) still gives other voxels: the companions see to it
    d = pts[:, :3] - lo
    vs = np.float32(c["voxel_size"])
    wrong, right = np.floor(d * (np.float32(1) / vs)), np.floor(d / vs).astype(np.int64)
    src = np.nonzero(np.all((wrong >= 0) & (wrong < np.float32([1408, 1600, 40])), 1))[0]
    _, first, counts = np.unique(wrong[src].astype(np.int64), axis=0, return_index=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    _, want_coords, want_occ, _ = ref.voxelize(c["frames"], c["voxel_size"], c["bounds"], 5, 60000)
    assert len(want_coords) < 60000, "the run's max_voxels does not clip"
    assert len(order) != len(want_coords) or (right[src[first[order]]][:, ::-1] != want_coords[:, 1:]).any() or \
        (np.minimum(counts[order], 5) != want_occ).any()


def test_big_grid_keys_pass_32_bits():
    c = cases.build("big_grid")
    grid = ref.grid_of(c["voxel_size"], c["bounds"])
    eq(grid, [4096, 4096, 512])
    assert len(c["frames"]) == 2 and 900 <= sum(len(f) for f in c["frames"]) <= 1100
    for b, f in enumerate(c["frames"]):
        cells, kept = ref.cells_of(f, c["voxel_size"], c["bounds"])
        assert kept.all()
        key = ((b * grid[2] + cells[:, 2]) * grid[1] + cells[:, 1]) * grid[0] + cells[:, 0]
        assert key.max() >= 2 ** 32 and len(np.unique(key)) < len(key)
        for cz in (0, 511):
            for cy in (0, 4095):
                for cx in (0, 4095):
                    assert (cells == [cx, cy, cz]).all(1).any(), "a corner cell"


def test_site_cases():
    for name, (shape, batch, n, _) in cases.SITE_CASES.items():
        c = cases.build(name)
        co = c["coords"]
        assert co.dtype == np.int32 and len(np.unique(co, axis=0)) == len(co)
        assert (co >= 0).all() and (co[:, 1:] < shape).all() and (co[:, 0] < batch).all()
        cells = batch * shape[0] * shape[1] * shape[2]
        assert len(co) == (round(0.3 * cells) if n is None else n)
        if len(co) >= 8 * batch:
            assert all((co == r).all(1).any() for r in cases.corners(shape, batch)), "all eight corners"
        assert not (np.diff(co[:, 0]) >= 0).all(), "rows in random order"
    assert len(cases.build("kpt_40959")["coords"]) + 1 == len(cases.build("kpt_40960")["coords"]) == cases.SUBM_KPT_MIN_ROWS
    assert 200 <= len(cases.build("few_hundred")["coords"]) <= 999


def test_chunk_cases_have_the_stated_ticket_counts():
    for case, geom, tickets in cases.CHUNK_RUNS:
        ks, st, _ = cases.STRIDED_GEOMETRIES[geom]
        kc = int(np.prod([-(-k // s) for k, s in zip(ks, st)]))
        assert len(cases.build(case)["coords"]) * kc == tickets
    assert [t for _, _, t in cases.CHUNK_RUNS] == [2040, 2048, 2056, 4096, 4104, 2048, 2050, 528000]
    assert -(-528000 // cases.SCAN_CHUNK) == 258
    # rows_66000: outputs are first touched behind the 256th chunk too (the creator of an output is its smallest input row)
    _, nbr, _, _ = strided_ref("rows_66000", "k3s2p1")
    creator = np.where(nbr >= 0, nbr, 1 << 30).min(0)
    assert ((creator * 8) // cases.SCAN_CHUNK >= 256).sum() > 10


def test_strided_geometries_hit_their_edges():
    c = cases.build("odd_grid")
    co = c["coords"].astype(np.int64)
    for geom, (ks, st, pd) in cases.STRIDED_GEOMETRIES.items():
        out, nbr, out_shape, _ = strided_ref("odd_grid", geom)
        assert geom != "k3s2p1" or len(out) <= len(co), "the clipped runs need a true count of at most cap_in"
        assert (out[:, 1:].max(0) == np.array(out_shape) - 1).all()
        reached = np.zeros(len(co), bool)
        reached[nbr[nbr >= 0]] = True
        if geom in ("k1s2p0", "k2s2p0", "k3s3p0"):
            assert not reached.all(), "sites that reach no output (odd coordinates, or cut by out_shape)"
        # a site on the last plane whose candidate output lies outside out_shape
        v = co[:, 1:] + pd
        cut = ((v % st == 0) & (v // st >= out_shape)).any()
        if geom in ("k3s2p0", "k2s2p0", "k3s3p0", "k3s2p011"):
            assert cut, "the high border cuts an output"
    out, nbr, _, _ = strided_ref("odd_grid", "k3s1p1")
    assert (ref.transpose(nbr, len(out), len(co)) >= 0).sum(0).max() == 27, "stride 1: an interior site reaches 27 outputs"


def test_padded_and_bad_batch_cases():
    c = cases.build("padded")
    assert len(c["coords"]) == c["n_live"] + cases.PAD_ROWS and len(np.unique(c["coords"], axis=0)) == len(c["coords"])
    live = ref.subm_rulebook(c["coords"], c["n_live"], c["shape"], 3)
    every = ref.subm_rulebook(c["coords"], len(c["coords"]), c["shape"], 3)
    assert (live != every[:, :c["n_live"]]).any(), "the rows behind the live count would be neighbours"
    c = cases.build("bad_batch")
    co, bad = c["coords"], c["bad_rows"]
    assert sorted(co[bad, 0].tolist()) == [-1, -1, -1, 64, 64, 64]
    # the reference on the valid rows alone, renumbered, is the reference's answer for them
    good = np.setdiff1d(np.arange(len(co)), bad)
    new = np.full(len(co) + 1, -1, np.int64)
    new[good] = np.arange(len(good))
    full = ref.subm_rulebook(co, len(co), c["shape"], 3)
    eq(new[full[:, good]], ref.subm_rulebook(co[good], len(good), c["shape"], 3))
    eq(np.delete(full[:, bad], 13, 0), -1)
    eq(full[13, bad], bad)
    ks, st, pd = cases.STRIDED_GEOMETRIES["k3s2p1"]
    oc, nbr, _, overflow = ref.sparse_rulebook(co, len(co), c["shape"], ks, st, pd)
    oc2, nbr2, _, overflow2 = ref.sparse_rulebook(co[good], len(good), c["shape"], ks, st, pd)
    assert overflow and not overflow2
    eq(oc, oc2)
    eq(new[nbr], nbr2)


def test_capped_tables_are_prefixes():
    co, nbr, _, _ = strided_ref("odd_grid", "k3s2p1")
    T = len(co)
    assert T - 257 > 1
    for cap in (T, T - 1, T - 257, 1):
        c2, n2, _, overflow = strided_ref("odd_grid", "k3s2p1", cap)
        assert overflow == (cap < T)
        eq(c2, co[:cap])
        eq(n2, nbr[:, :cap])


def test_key_range_case():
    c = cases.build("key_range")
    co = c["coords"].astype(np.int64)
    shape = c["shape"]
    assert shape[0] * shape[1] * shape[2] < 2 ** 34 <= np.prod(cases.REFUSED_SHAPE)
    assert sorted(np.unique(co[:, 0]).tolist()) == [0, 63]
    key = ((co[:, 0] * shape[0] + co[:, 1]) * shape[1] + co[:, 2]) * shape[2] + co[:, 3]
    assert key.min() == 0 and key.max() == 64 * shape[0] * shape[1] * shape[2] - 1 and 2 ** 40 - 2 ** 27 < key.max() < 2 ** 40
    nbr = ref.subm_rulebook(co, len(co), shape, 3)
    assert (np.delete(nbr, 13, 0) >= 0).sum() >= 2 * 40, "pairs of adjacent cells"

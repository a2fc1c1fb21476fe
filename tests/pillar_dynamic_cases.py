"""Seeded cases of the dynamic pillar encoder (vision3d_amd/detector/pillar.py DynamicPillarFeatureNet), shared by
tests/test_host_pillar_dynamic.py and tests/test_gpu_pillar_dynamic.py.  numpy only; nothing here computes an expected value
(`voxel_mean` is an INPUT of the encoder: the fp32 rounding of the float64 mean of a pillar's points, where the dynamic voxelizer
stands within 2^-25 + half an ulp).

The tiny grid of tests/pillar_cases.py: bounds [0, -4, -3, 6.4, 4, 1], pillars 0.4 x 0.4 x 4 -> a 20 x 16 map.  Every pillar sits in a
cell of its own, its points strictly inside; pillars are frame-major, the last cell of the last frame is occupied.  The flat point
array is the concatenation of the frames, SHUFFLED inside each frame -- a pillar's points are not contiguous --, with dropped points
(point_voxel = -1; in-grid values, as a point whose voxel max_voxels cut) scattered through it, the first and the last entry among
them.

Which case crosses which cap of csrc/pillar.hip:
  second_pass   M = 1029 = 4 * 256 + 5   pillar_dyn_bwd_kernel: 256 workgroups of four pillars leave partials -- every workgroup takes a
                                         second pass, the last one partial (five pillars)
  many_points   N_kept = 65 536 + 37     pillar_dyn_moments_kernel: 256 workgroups of 256 points leave partials -- a second pass whose
                                         tail is 37 points (+ the dropped ones); also 300 pillars of ~218 points: four chunks each
  encode_pass   M = 4101 = 4096 + 5      pillar_dyn_encode_kernel: 4096 one-wave workgroups, five of them take a second pillar
  chunk_edges   occupancies 1, 2, 63, 64, 65, 128, 129, 200 (+ 1..8): the edges of the encode kernel's 64-point chunks
  crowded       one pillar of 700 points: eleven chunks, the last of 60
  every M > 2048 (encode_pass): pillar_dyn_offsets_kernel scans 2048 occupancies per round -- a third round of five
tie: two bit-identical points in the 66-point pillar 0, at non-adjacent flat indices; in flat order (the host shim's) they are the
pillar's 2nd and 66th point -- different 64-chunks.  (On the GPU the list order is whatever the atomic cursor gave; no placement can
split two of 66 points for EVERY order.  The rule makes the result the same.)
"""
import numpy as np

from pillar_cases import BOUNDS, EPS, H, MOMENTUM, VOXEL, W, geometry  # the tiny grid  # noqa: F401

# name: (M, C, CHANNELS, B, dropped points, variant)
CASES = {
    "one_point": (1, 4, 64, 1, 2, None),
    "five": (5, 4, 128, 1, 3, None),
    "chunk_edges": (37, 5, 128, 1, 9, "chunk_edges"),
    "crowded": (9, 3, 64, 1, 5, "crowded"),
    "empty_middle": (41, 4, 128, 3, 7, "empty_middle"),
    "second_pass": (1029, 4, 128, 4, 11, None),
    "many_points": (300, 4, 64, 1, 13, "many_points"),
    "encode_pass": (4101, 3, 64, 13, 6, None),
    "tie": (5, 4, 128, 1, 4, "tie"),
    "empty": (0, 4, 128, 2, 3, None),
}
CASE_IDS = sorted(CASES)
CHUNK_EDGES = (1, 2, 63, 64, 65, 128, 129, 200)
MANY_POINTS = 256 * 256 + 37


def tiny_cfg():
    """The tiny grid as a dynamic pillar configuration of the package (car anchors); MAX_OCCUPANCY = 8 is what the hard form would keep."""
    from vision3d_amd.core.config import pillar_dynamic_car_cfg
    cfg = pillar_dynamic_car_cfg()
    cfg.merge_from_dict(dict(GRID_BOUNDS=list(BOUNDS), VOXEL_SIZE=list(VOXEL), MAX_OCCUPANCY=8, MAX_VOXELS=400))
    return cfg


def _occupancies(name, M, variant, rng):
    if name == "one_point":
        return np.array([1], np.int64)
    if name == "five":
        return np.array([7, 1, 3, 5, 2], np.int64)
    if variant == "chunk_edges":
        occ = rng.integers(1, 9, size=M)
        occ[rng.permutation(M)[:len(CHUNK_EDGES)]] = CHUNK_EDGES
        return occ
    if variant == "crowded":
        occ = np.ones(M, np.int64)
        occ[4] = 700
        return occ
    if variant == "many_points":
        occ = np.full(M, MANY_POINTS // M, np.int64)
        occ[:MANY_POINTS - int(occ.sum())] += 1
        return occ
    if variant == "tie":
        return np.array([66, 1, 4, 2, 3], np.int64)
    if name in ("second_pass",):
        return rng.integers(1, 4, size=M)
    if name == "encode_pass":
        return rng.integers(1, 3, size=M)
    return rng.integers(1, 13, size=M)


def build(name):
    M, C, CH, B, n_drop, variant = CASES[name]
    rng = np.random.default_rng([20261, CASE_IDS.index(name)])
    K = C + 6
    frames = [f for f in range(B) if not (variant == "empty_middle" and f == 1)]
    counts = np.zeros(B, np.int64)
    for i in range(M):
        counts[frames[i % len(frames)]] += 1
    coords = np.zeros((M, 4), np.int32)
    at = 0
    for b in range(B):
        cells = rng.choice(H * W, size=int(counts[b]), replace=False)
        if M and b == frames[-1] and counts[b] and (H * W - 1) not in cells:
            cells[-1] = H * W - 1
        coords[at:at + counts[b], 0] = b
        coords[at:at + counts[b], 2] = cells // W
        coords[at:at + counts[b], 3] = cells % W
        at += counts[b]
    occupancy = _occupancies(name, M, variant, rng).astype(np.int32)

    def cloud(v, n):
        u = rng.uniform(0.05, 0.95, size=(n, 3))
        p = np.zeros((n, C), np.float32)
        p[:, 0] = BOUNDS[0] + (coords[v, 3] + u[:, 0]) * VOXEL[0]
        p[:, 1] = BOUNDS[1] + (coords[v, 2] + u[:, 1]) * VOXEL[1]
        p[:, 2] = BOUNDS[2] + u[:, 2] * VOXEL[2]
        p[:, 3:] = rng.uniform(0.0, 1.0, size=(n, C - 3))
        return p

    # per frame: the pillars' points and the frame's share of the dropped points, shuffled together
    drop_frame = np.sort(rng.integers(0, B, size=n_drop)) if B else np.zeros(0, np.int64)
    if n_drop:
        drop_frame[0], drop_frame[-1] = 0, B - 1
    points, point_voxel, ends = [], [], []
    for b in range(B):
        pts = [cloud(v, int(occupancy[v])) for v in range(M) if coords[v, 0] == b]
        pv = [np.full(int(occupancy[v]), v, np.int32) for v in range(M) if coords[v, 0] == b]
        d = int((drop_frame == b).sum())
        if d:
            junk = np.zeros((d, C), np.float32)
            junk[:, :3] = np.asarray(BOUNDS[:3]) + rng.uniform(0.05, 0.95, size=(d, 3)) * (np.asarray(BOUNDS[3:]) - np.asarray(BOUNDS[:3]))
            junk[:, 3:] = rng.uniform(2.0, 3.0, size=(d, C - 3))
            pts.append(junk)
            pv.append(np.full(d, -1, np.int32))
        pts = np.concatenate(pts) if pts else np.zeros((0, C), np.float32)
        pv = np.concatenate(pv) if pv else np.zeros(0, np.int32)
        order = rng.permutation(len(pv))
        points.append(pts[order])
        point_voxel.append(pv[order])
        ends.append(len(pv))
    points = np.concatenate(points) if points else np.zeros((0, C), np.float32)
    point_voxel = np.concatenate(point_voxel) if point_voxel else np.zeros(0, np.int32)

    def swap(i, j):
        points[[i, j]] = points[[j, i]]
        point_voxel[[i, j]] = point_voxel[[j, i]]
    if n_drop:  # a dropped point first and last
        swap(0, int(np.flatnonzero(point_voxel[:ends[0]] < 0)[0]))
        last = len(point_voxel) - 1
        swap(last, last - ends[-1] + 1 + int(np.flatnonzero(point_voxel[last - ends[-1] + 1:] < 0)[-1]))
    if variant == "tie":
        mine = np.flatnonzero(point_voxel == 0)
        # the pillar's 2nd and 66th point in flat order: bit-identical, and at a corner of the cell with the largest extra channel --
        # y is linear in the point, so a corner of the cloud is the maximum of a fair share of the channels
        points[mine[1], 0] = BOUNDS[0] + (coords[0, 3] + 0.95) * VOXEL[0]
        points[mine[1], 1] = BOUNDS[1] + (coords[0, 2] + 0.95) * VOXEL[1]
        points[mine[1], 2] = BOUNDS[2] + 0.95 * VOXEL[2]
        points[mine[1], 3:] = 1.0
        points[mine[-1]] = points[mine[1]]
    mean = np.zeros((M, C), np.float32)
    if M:
        keep = point_voxel >= 0
        total = np.zeros((M, C), np.float64)
        np.add.at(total, point_voxel[keep], points[keep].astype(np.float64))
        mean = (total / occupancy[:, None].astype(np.float64)).astype(np.float32)
    bound = 1.0 / np.sqrt(K)
    weight = rng.uniform(-bound, bound, size=(CH, K)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, size=CH).astype(np.float32)
    beta = rng.normal(0.0, 0.2, size=CH).astype(np.float32)
    running_mean = rng.normal(0.0, 0.5, size=CH).astype(np.float32)
    running_var = rng.uniform(0.5, 2.0, size=CH).astype(np.float32)
    d_rows = (rng.normal(0.0, 1.0, size=(M, CH)) * rng.uniform(0.1, 3.0, size=(M, 1))).astype(np.float32)
    return dict(name=name, M=M, N=len(point_voxel), C=C, K=K, CH=CH, B=B, variant=variant, points=points, point_voxel=point_voxel,
                voxel_mean=mean, occupancy=occupancy, coordinates=coords, batch_size=B, frame_sizes=ends, geom=geometry(), weight=weight,
                gamma=gamma, beta=beta, running_mean=running_mean, running_var=running_var, d_rows=d_rows, eps=EPS, momentum=MOMENTUM)


def permuted(c, seed=1):
    """The same case with the flat points and point_voxel shuffled TOGETHER (across the whole array); -> (case, perm) with
    new_points[j] = points[perm[j]], so old index i sits at inverse[i]."""
    perm = np.random.default_rng([seed, c["N"]]).permutation(c["N"])
    d = dict(c, points=np.ascontiguousarray(c["points"][perm]), point_voxel=np.ascontiguousarray(c["point_voxel"][perm]))
    return d, perm


def check_well_formed(c):
    """The layout promises of the docstring, asserted on the case itself."""
    M, N = c["M"], c["N"]
    co, occ, pv, pts = c["coordinates"], c["occupancy"], c["point_voxel"], c["points"]
    assert pts.shape == (N, c["C"]) and pv.shape == (N,) and pts.dtype == np.float32 and pv.dtype == np.int32
    assert (co[:, 1] == 0).all() and (co[:, 0] >= 0).all() and (co[:, 0] < c["B"]).all()
    assert (co[:, 2] >= 0).all() and (co[:, 2] < H).all() and (co[:, 3] >= 0).all() and (co[:, 3] < W).all()
    keys = (co[:, 0].astype(np.int64) * H + co[:, 2]) * W + co[:, 3]
    assert len(np.unique(keys)) == M, "distinct cells"
    assert (np.diff(co[:, 0]) >= 0).all(), "frame-major pillars"
    assert ((pv >= 0) & (pv < M) | (pv == -1)).all()
    dropped = pv < 0
    assert dropped.sum() == CASES[c["name"]][4] and dropped[0] and dropped[-1], "dropped points, the first and the last entry among them"
    assert (np.bincount(pv[~dropped], minlength=M)[:M] == occ).all() and (occ >= 1).all(), "occupancy = the true counts"
    if M:
        assert ((co[:, 2] == H - 1) & (co[:, 3] == W - 1)).any(), "the last cell"
        # flat = the frames concatenated: a kept point lies inside its frame's stretch
        starts = np.concatenate([[0], np.cumsum(c["frame_sizes"])])
        frame_of_point = np.searchsorted(starts, np.arange(N), side="right") - 1
        assert (frame_of_point[~dropped] == co[pv[~dropped], 0]).all()
        v = pv[~dropped]
        fx = (pts[~dropped, 0].astype(np.float64) - BOUNDS[0]) / VOXEL[0] - co[v, 3]
        fy = (pts[~dropped, 1].astype(np.float64) - BOUNDS[1]) / VOXEL[1] - co[v, 2]
        fz = (pts[~dropped, 2].astype(np.float64) - BOUNDS[2]) / VOXEL[2]
        for t in (fx, fy, fz):
            assert (t > 0.04).all() and (t < 0.96).all(), "points strictly inside their cell"
        big = int(np.argmax(occ))
        if occ[big] >= 4:  # not contiguous: the largest pillar's points are spread over more flat entries than it has points
            mine = np.flatnonzero(pv == big)
            assert mine[-1] - mine[0] + 1 > len(mine)
    if c["variant"] == "empty_middle":
        assert not (co[:, 0] == 1).any() and (co[:, 0] == 0).any() and (co[:, 0] == 2).any()
    if c["variant"] == "chunk_edges":
        assert set(CHUNK_EDGES) <= set(occ.tolist())
    if c["variant"] == "crowded":
        assert sorted(occ.tolist()) == [1] * (M - 1) + [700]
    if c["variant"] == "many_points":
        assert int(occ.sum()) == MANY_POINTS
    if c["variant"] == "tie":
        mine = np.flatnonzero(pv == 0)
        assert len(mine) == 66 and (pts[mine[1]] == pts[mine[-1]]).all() and mine[-1] - mine[1] > 1
        assert 1 // 64 != 65 // 64  # 2nd and 66th of the pillar in flat order: different chunks

"""Seeded cases of the pillar feature encoder (vision3d_amd/detector/pillar.py), shared by tests/test_host_pillar.py and
tests/test_gpu_pillar.py.  numpy only; nothing here computes an expected value.

Tiny grid: bounds [0, -4, -3, 6.4, 4, 1], pillars 0.4 x 0.4 x 4 -> a 20 x 16 map (H along y, W along x).  Every pillar sits in a cell
of its own, its points strictly inside (at least 5 % of the cell away from every face).  Where M >= 2 the occupancies contain both 1
and P; the last cell (y = H - 1, x = W - 1) of the last frame is always occupied.  beta ~ N(0, 0.2) gives shifts of both signs, so the
padded candidate wins in some channels and loses in others (tests/test_host_pillar.py counts both on the reference).

The kernels give four pillars to a workgroup per pass and at most 256 workgroups leave partial sums: M = 5 and 37 end in a partial
workgroup and cross workgroups, M = 1029 = 4 * 256 + 5 makes every workgroup take a second pass, the last one partial.
"""
import numpy as np

BOUNDS = [0.0, -4.0, -3.0, 6.4, 4.0, 1.0]
VOXEL = [0.4, 0.4, 4.0]
H, W = 20, 16
EPS, MOMENTUM = 1e-3, 0.01

# name: (M, P, C, CHANNELS, B, variant)
CASES = {
    "one_pillar": (1, 3, 4, 64, 1, None),
    "five": (5, 3, 4, 128, 1, None),
    "single_slot": (37, 1, 3, 64, 1, None),
    "thirtyseven": (37, 8, 5, 128, 1, None),
    "full_slots": (41, 32, 4, 128, 3, "empty_middle"),
    "second_pass": (1029, 3, 4, 128, 4, None),
    "tie": (5, 8, 4, 128, 1, "tie"),
    "tie_narrow": (6, 8, 3, 64, 1, "tie"),
    "empty": (0, 8, 4, 128, 2, None),
}
CASE_IDS = sorted(CASES)


def geometry():
    """-> the six fp32 numbers (vx, vy, vz, vx / 2 + x0, vy / 2 + y0, vz / 2 + z0), each offset one fp32 sum, as Python floats."""
    v = np.asarray(VOXEL, np.float32)
    o = v / np.float32(2) + np.asarray(BOUNDS[:3], np.float32)
    return tuple(float(x) for x in np.concatenate([v, o]))


def tiny_cfg():
    """The tiny grid as a pillar configuration of the package (car anchors)."""
    from vision3d_amd.core.config import pillar_car_cfg
    cfg = pillar_car_cfg()
    cfg.merge_from_dict(dict(GRID_BOUNDS=list(BOUNDS), VOXEL_SIZE=list(VOXEL), MAX_OCCUPANCY=8, MAX_VOXELS=400))
    return cfg


def build(name):
    M, P, C, CH, B, variant = CASES[name]
    rng = np.random.default_rng([20260, CASE_IDS.index(name)])
    K = C + 6
    # distinct cells: frame sizes, then cells drawn without replacement per frame; the last frame owns the last cell
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
    occupancy = rng.integers(1, P + 1, size=M).astype(np.int32)
    if M >= 2:
        occupancy[0], occupancy[1] = P, 1
    if variant == "tie":
        occupancy[0] = max(4, P - 2)  # short of P, so the padded candidate competes with the tied rows too
        occupancy[2] = P
    features = np.zeros((M, P, C), np.float32)
    for m in range(M):
        n = int(occupancy[m])
        u = rng.uniform(0.05, 0.95, size=(n, 3))
        features[m, :n, 0] = BOUNDS[0] + (coords[m, 3] + u[:, 0]) * VOXEL[0]
        features[m, :n, 1] = BOUNDS[1] + (coords[m, 2] + u[:, 1]) * VOXEL[1]
        features[m, :n, 2] = BOUNDS[2] + u[:, 2] * VOXEL[2]
        features[m, :n, 3:] = rng.uniform(0.0, 1.0, size=(n, C - 3))
    if variant == "tie":
        features[0, 2] = features[0, 1]  # two identical points: rows 1 and 2 tie in every channel, row 1 must win where either does
    bound = 1.0 / np.sqrt(K)
    weight = rng.uniform(-bound, bound, size=(CH, K)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, size=CH).astype(np.float32)
    beta = rng.normal(0.0, 0.2, size=CH).astype(np.float32)
    running_mean = rng.normal(0.0, 0.5, size=CH).astype(np.float32)
    running_var = rng.uniform(0.5, 2.0, size=CH).astype(np.float32)
    d_rows = (rng.normal(0.0, 1.0, size=(M, CH)) * rng.uniform(0.1, 3.0, size=(M, 1))).astype(np.float32)  # random, non-uniform
    return dict(name=name, M=M, P=P, C=C, K=K, CH=CH, B=B, variant=variant, features=features, occupancy=occupancy, coordinates=coords,
                batch_size=B, geom=geometry(), weight=weight, gamma=gamma, beta=beta, running_mean=running_mean, running_var=running_var,
                d_rows=d_rows, eps=EPS, momentum=MOMENTUM)


def check_well_formed(c):
    """The layout promises of the docstring, asserted on the case itself."""
    M, P = c["M"], c["P"]
    co, occ, f = c["coordinates"], c["occupancy"], c["features"]
    assert (co[:, 1] == 0).all() and (co[:, 0] >= 0).all() and (co[:, 0] < c["B"]).all()
    assert (co[:, 2] >= 0).all() and (co[:, 2] < H).all() and (co[:, 3] >= 0).all() and (co[:, 3] < W).all()
    keys = (co[:, 0].astype(np.int64) * H + co[:, 2]) * W + co[:, 3]
    assert len(np.unique(keys)) == M, "distinct cells"
    assert (occ >= 1).all() and (occ <= P).all()
    if M >= 2:
        assert (occ == 1).any() and (occ == P).any()
    if M:
        assert ((co[:, 2] == H - 1) & (co[:, 3] == W - 1)).any(), "the last cell"
    for m in range(M):
        n = int(occ[m])
        assert (f[m, n:] == 0).all()
        fx = (f[m, :n, 0].astype(np.float64) - BOUNDS[0]) / VOXEL[0] - co[m, 3]
        fy = (f[m, :n, 1].astype(np.float64) - BOUNDS[1]) / VOXEL[1] - co[m, 2]
        fz = (f[m, :n, 2].astype(np.float64) - BOUNDS[2]) / VOXEL[2]
        for t in (fx, fy, fz):
            assert (t > 0.04).all() and (t < 0.96).all(), "points strictly inside their cell"
    if c["variant"] == "empty_middle":
        assert not (co[:, 0] == 1).any() and (co[:, 0] == 0).any() and (co[:, 0] == 2).any()
    if c["variant"] == "tie":
        assert occ[0] >= 3 and occ[0] < P and (f[0, 1] == f[0, 2]).all()

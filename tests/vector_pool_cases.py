"""Seeded inputs of the VectorPool tests: B = 2 frames of 300 support rows in the box [20, 23.2] x [-3, 0.2] x [-2, -0.4] -- uniform, or
nodes of its 0.2 x 0.2 x 0.4 m lattice in shuffled order -- plus 17 appended duplicates of random rows (N = 317, no multiple of 64),
and M = 37 queries uniform in the box grown by 0.3 m, so that some lie wholly outside."""
import numpy as np

BOX_LO, BOX_HI = np.array([20.0, -3.0, -2.0]), np.array([23.2, 0.2, -0.4])
B, N_ROWS, N_DUP, M = 2, 300, 17, 37
GROUPS = [((2, 2, 2), 0.2), ((3, 3, 3), 0.4), ((3, 2, 1), 0.4), ((3, 3, 3), 0.8)]
KINDS = ("uniform", "lattice")


def make_case(kind, seed=0):
    """-> xyz (B, 317, 3) float32, q (B, 37, 3) float32."""
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    frames = []
    for _ in range(B):
        if kind == "uniform":
            rows = BOX_LO + rng.random((N_ROWS, 3)) * (BOX_HI - BOX_LO)
        else:
            steps = np.array([0.2, 0.2, 0.4])
            counts = np.round((BOX_HI - BOX_LO) / steps).astype(int)
            nodes = np.stack(np.meshgrid(*[np.arange(c) for c in counts], indexing="ij"), -1).reshape(-1, 3)
            rows = BOX_LO + nodes[rng.permutation(len(nodes))[:N_ROWS]] * steps
        rows = rows.astype(np.float32)
        frames.append(np.concatenate([rows, rows[rng.integers(0, N_ROWS, N_DUP)]]))
    q = (BOX_LO - 0.3 + rng.random((B, M, 3)) * (BOX_HI - BOX_LO + 0.6)).astype(np.float32)
    return np.stack(frames), q


# ---- cases of the search over the shared cell grid (csrc/cell_grid.hip); tests/test_host_vector_pool.py checks that the restatement
# leaves at most GRID_CAP of the centres of each undecided
GRID_CAP = 0.001
GRID_BUILD_N = (4096, 4097, 12289, 20481)
GRID_BUILD_SEEDS = {4096: 0, 4097: 1, 12289: 1, 20481: 0}  # (the first seeds that leave no centre of either group undecided)
GRID_GROUPS = [((3, 3, 3), 0.4), ((2, 2, 2), 0.2)]
GRID_SINGLE_KINDS = ("within", "equal")


def grid_build_case(n):
    """Two frames of n rows, uniform in 12.8 x 12.8 x 1.6 m; the second shifted by (40, -30, 0) m and half as wide; 8 queries per
    frame ON support rows."""
    rng = np.random.default_rng([GRID_BUILD_SEEDS[n], 61, n])
    xyz = rng.random((2, n, 3)) * np.array([12.8, 12.8, 1.6])
    xyz[1, :, :2] = xyz[1, :, :2] * 0.5 + np.array([40.0, -30.0])
    xyz = xyz.astype(np.float32)
    q = np.stack([f[rng.choice(n, 8, replace=False)] for f in xyz])
    return xyz, q


def grid_growth_case(seed=1):
    """Two frames of 2 000 rows uniform over 200 m x 200 m x 2 m plus, around each of 16 of them (the queries), 20 further rows within
    0.3 m: with the reach 0.301 m of (2, 2, 2) / 0.2 the first try is some 440 000 cells against 32 768 keys."""
    rng = np.random.default_rng([seed, 62])
    frames, qs = [], []
    for _ in range(2):
        rows = rng.random((2000, 3)) * np.array([200.0, 200.0, 2.0]) + np.array([-100.0, -100.0, -1.0])
        picked = rng.choice(2000, 16, replace=False)
        around = rows[picked][:, None, :] + rng.uniform(-0.3, 0.3, (16, 20, 3))
        frame = np.concatenate([rows, around.reshape(-1, 3)])
        order = rng.permutation(len(frame))
        frames.append(frame[order].astype(np.float32))
        qs.append(frames[-1][np.argsort(order)[picked]])
    return np.stack(frames), np.stack(qs)


def grid_single_cell_case(kind, seed=2):
    """within: 60 rows inside 0.25 m along every axis, less than one reach of (2, 2, 2) / 0.2; equal: 100 rows bit-equal (extent 0).
    8 queries per frame: four on the rows, four up to 0.25 m off."""
    rng = np.random.default_rng([seed, 63, kind == "equal"])
    base = np.array([[31.0, -12.0, -1.0], [-7.5, 44.0, 0.5]])
    if kind == "within":
        xyz = base[:, None, :] + rng.random((2, 60, 3)) * 0.25
    else:
        xyz = np.repeat(base[:, None, :], 100, 1)
    xyz = xyz.astype(np.float32)
    q = np.stack([f[rng.integers(0, f.shape[0], 8)] for f in xyz])
    q[:, 4:] += rng.uniform(-0.25, 0.25, (2, 4, 3)).astype(np.float32)
    return xyz, q


def make_features(channels, seed=0, n=N_ROWS + N_DUP):
    """(B, n, channels) float32; the appended duplicates get features of their own (they must never show)."""
    return np.random.default_rng([seed, 77, channels]).standard_normal((B, n, channels)).astype(np.float32)


def randomize(module, seed):
    """Non-trivial weights and eval BatchNorm statistics for a VectorPoolAggregationMSG (its initialisation gives outputs of 1e-5)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("local_weight") or (name.endswith("weight") and p.dim() == 2):
                p.copy_(torch.randn(p.shape, generator=g) * (1.5 / p.shape[-2 if name.endswith("local_weight") else -1] ** 0.5))
        for mod in module.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) * 0.5 + 0.75)
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) * 0.5 + 0.75)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
    return module

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

"""Measures and builders shared by tests/test_host_pillar_dynamic.py and tests/test_gpu_pillar_dynamic.py.  The bounds and the error
measures are the project's, from tests/pillar_checks.py (stated in tests/test_host_pillar.py)."""
import numpy as np
import torch

import pillar_dynamic_cases as cases
import pillar_dynamic_ref as ref
from pillar_checks import GRAD_BOUND, VALUE_BOUND, grad_error, value_error  # noqa: F401


def module_for(c, dtype=torch.float32):
    """DynamicPillarFeatureNet on the tiny grid with the case's tensors loaded."""
    from vision3d_amd.detector.pillar import DynamicPillarFeatureNet
    cfg = cases.tiny_cfg()
    cfg.merge_from_dict(dict(C_IN=c["C"], PILLAR=dict(CHANNELS=c["CH"])))
    net = DynamicPillarFeatureNet(cfg)
    with torch.no_grad():
        net.linear.weight.copy_(torch.from_numpy(c["weight"]))
        net.norm.weight.copy_(torch.from_numpy(c["gamma"]))
        net.norm.bias.copy_(torch.from_numpy(c["beta"]))
        net.norm.running_mean.copy_(torch.from_numpy(c["running_mean"]))
        net.norm.running_var.copy_(torch.from_numpy(c["running_var"]))
    return net.to(dtype)


def item_of(c, device="cpu"):
    return dict(flat_points=torch.from_numpy(c["points"]).to(device), point_voxel=torch.from_numpy(c["point_voxel"]).to(device),
                voxel_mean=torch.from_numpy(c["voxel_mean"]).to(device), occupancy=torch.from_numpy(c["occupancy"]).to(device),
                coordinates=torch.from_numpy(c["coordinates"]).to(device), batch_size=c["batch_size"])


def winner_validity(c, r, winner, bound):
    """Every (pillar, channel): the winner is a point of that pillar, and the float64 activation there lies within `bound` (value
    convention) of the float64 maximum.  r = ref.encode(c, ...) in float64; -> the largest gap."""
    winner = np.asarray(winner).astype(np.int64)
    assert (winner >= 0).all() and (winner < c["N"]).all()
    assert (c["point_voxel"][winner] == np.arange(c["M"])[:, None]).all(), "a winner inside its pillar"
    at = ref.gather_winner(r["a"], r["idx"], winner, c["N"]).numpy()
    best = r["rows"].numpy()
    gap = float(np.abs(best - at).max() / max(1.0, np.abs(best).max()))
    assert gap <= bound, f"winner not a maximum within the forward bound: {gap:.3e} > {bound:.3e}"
    return gap


def tie_pair(c):
    """The flat indices (lower, higher) of the two identical points of the tie case's pillar 0."""
    mine = np.flatnonzero(c["point_voxel"] == 0)
    return int(mine[1]), int(mine[-1])

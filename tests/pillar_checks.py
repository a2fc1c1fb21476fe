"""Measures and builders shared by tests/test_host_pillar.py and tests/test_gpu_pillar.py (the bounds are stated in the former)."""
import numpy as np
import torch

import pillar_cases as cases
import pillar_ref as ref

VALUE_BOUND, GRAD_BOUND = 2e-6, 1e-6  # the project bounds: relative on a value, of the largest gradient


def value_error(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max())) if want.size else 0.0


def grad_error(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def module_for(c, dtype=torch.float32):
    """PillarFeatureNet on the tiny grid with the case's tensors loaded."""
    from vision3d_amd.detector.pillar import PillarFeatureNet
    cfg = cases.tiny_cfg()
    cfg.merge_from_dict(dict(C_IN=c["C"], MAX_OCCUPANCY=c["P"], PILLAR=dict(CHANNELS=c["CH"])))
    net = PillarFeatureNet(cfg)
    with torch.no_grad():
        net.linear.weight.copy_(torch.from_numpy(c["weight"]))
        net.norm.weight.copy_(torch.from_numpy(c["gamma"]))
        net.norm.bias.copy_(torch.from_numpy(c["beta"]))
        net.norm.running_mean.copy_(torch.from_numpy(c["running_mean"]))
        net.norm.running_var.copy_(torch.from_numpy(c["running_var"]))
    return net.to(dtype)


def item_of(c, device="cpu"):
    return dict(features=torch.from_numpy(c["features"]).to(device), occupancy=torch.from_numpy(c["occupancy"]).to(device),
                coordinates=torch.from_numpy(c["coordinates"]).to(device), batch_size=c["batch_size"])


def winner_validity(a64, winner, real, bound):
    """Every (m, c): the float64 activation at the given winner within `bound` (value convention) of the float64 maximum, and the
    index inside the pillar."""
    occ = real.sum(1).numpy()
    assert (winner >= -1).all() and (winner < occ[:, None]).all()
    assert not ((winner == -1) & (occ == real.shape[1])[:, None]).any(), "a full pillar has no padded candidate"
    at = ref.gather_winner(a64, winner).numpy()
    best = a64.max(dim=1).values.numpy()
    gap = float(np.abs(best - at).max() / max(1.0, np.abs(best).max()))
    assert gap <= bound, f"winner not a maximum within the forward bound: {gap:.3e} > {bound:.3e}"
    return gap

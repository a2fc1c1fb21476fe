"""Pillar feature encoder for SECOND (the PFN layer of PointPillars, arXiv 1812.05784), opt-in: cfg.PILLAR.

No upstream counterpart; the definition is this repository's (csrc/pillar_device.h, restated in float64 by tests/pillar_ref.py).
With a voxel as tall as the grid the Preprocessor's voxels are pillars: `features` (M, P, C) point slots, `occupancy` (M),
`coordinates` (M, 4) = (b, 0, y, x).  Per pillar: every real point becomes [its C channels | xyz - mean xyz of the pillar's points |
xyz - pillar centre] (K = C + 6), the padded slots stay zero; linear (no bias) -> BatchNorm1d over ALL M * P rows (the padded rows
count, as in the published encoder, so its checkpoints keep their meaning) -> ReLU -> maximum over all P rows.  The rows are
scattered into the (B, CHANNELS, H, W) canvas the dense RPN reads; no 3-D convolution runs.

PillarFeatureNet.forward runs csrc/pillar.hip (one launch in eval mode; three forwards and two backwards in training, through
PillarEncodeFunction); forward_torch is the op-by-op statement of the same arithmetic, and the path of CPU tensors and of shapes
beyond the native limits (P <= 64, 3 <= C <= 8, CHANNELS 64 or 128).  Gradients reach linear.weight, norm.weight and norm.bias, never
the points.

cfg.PILLAR.DYNAMIC (opt-in; DynamicPillarFeatureNet below): the same layer over the dynamic voxelizer's outputs -- every point of a
pillar counts, the BatchNorm population is the real points alone.  The key lives in core/config.py (pillar_dynamic_enabled reads it with
its default, False); PILLAR_DEFAULTS keeps the two keys every pillar configuration has had.

cfg.PILLAR.PLAN (opt-in; core/config.py pillar_plan_enabled): Second's raw-point entry points run on pillar_plan.PillarPlan, which
reads this module's parameters (linear.weight, _folded()) and writes the dense head's input itself; nothing in this file changes.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import _lib as L
from .. import spconv
from ..stamp import cached

PILLAR_DEFAULTS = dict(ENABLED=False, CHANNELS=128)
MAX_P, MIN_C, MAX_C, WIDTHS = 64, 3, 8, (64, 128)  # the native limits (csrc/pillar_device.h)
MAX_POINTS = 1 << 22  # the dynamic encoder's (and the dynamic voxelizer's) limit on the points of a call


def pillar_config(cfg):
    """-> the keys of cfg.PILLAR over their defaults (a config written before the key existed means "disabled")."""
    out = dict(PILLAR_DEFAULTS)
    out.update(cfg.get("PILLAR") or {})
    return out


def pillar_enabled(cfg):
    return bool(pillar_config(cfg)["ENABLED"])


def refuse_pillar(cfg, what):
    """The entry points that do not know the pillar encoder yet (follow-ups) say so instead of running the sparse backbone beside it."""
    if pillar_enabled(cfg):
        raise ValueError(f"cfg.PILLAR.ENABLED: {what} does not support the pillar encoder yet (Second.forward / inference on a "
                         "Preprocessor item do)")


def pillar_geometry(cfg):
    """-> (six fp32 numbers vx, vy, vz, vx / 2 + x0, vy / 2 + y0, vz / 2 + z0 -- each offset ONE fp32 sum --, (H, W)); refuses a grid
    that is not one pillar tall."""
    voxel, bounds = np.asarray(cfg.VOXEL_SIZE, np.float64), np.asarray(cfg.GRID_BOUNDS, np.float64).reshape(2, 3)
    cells = np.round((bounds[1] - bounds[0]) / voxel).astype(np.int64)  # the voxelizer's grid (x, y, z): spconv/utils.py
    if cells[2] != 1 or abs(voxel[2] - (bounds[1, 2] - bounds[0, 2])) > 1e-6 * (bounds[1, 2] - bounds[0, 2]):
        raise ValueError(f"cfg.PILLAR.ENABLED: VOXEL_SIZE[2] = {voxel[2]} must span the z extent of GRID_BOUNDS exactly once "
                         f"({bounds[0, 2]} .. {bounds[1, 2]}): a pillar is one voxel tall")
    v = voxel.astype(np.float32)
    o = v / np.float32(2) + bounds[0].astype(np.float32)
    return tuple(float(x) for x in np.concatenate([v, o])), (int(cells[1]), int(cells[0]))


def _native_shape(features, channels):
    return features.dim() == 3 and 1 <= features.shape[1] <= MAX_P and MIN_C <= features.shape[2] <= MAX_C and channels in WIDTHS


def pillar_encode(features, occupancy, coordinates, geom, weight, scale, shift):
    """v3d_pillar_encode (eval): -> rows (M, CHANNELS) f32; one launch, no host read."""
    L.require_gpu("pillar_encode", features, occupancy, coordinates, weight, scale, shift)
    features, weight = L.as_f32("pillar_encode", features), L.as_f32("pillar_encode", weight)
    occupancy, coordinates = L.as_i32("pillar_encode", occupancy), L.as_i32("pillar_encode", coordinates)
    scale, shift = L.as_f32("pillar_encode", scale), L.as_f32("pillar_encode", shift)
    M, P, C = features.shape
    CH = weight.shape[0]
    rows = torch.empty((M, CH), dtype=torch.float32, device=features.device)
    with L.device_guard(features.device):
        L.check(L.lib().v3d_pillar_encode(L.ptr(features), L.ptr(occupancy), L.ptr(coordinates), M, P, C, L.host_f32(geom), L.ptr(weight), CH,
                                          L.ptr(scale), L.ptr(shift), L.ptr(rows), L.stream_ptr()), "pillar_encode")
    return rows


def pillar_train_forward(features, occupancy, coordinates, geom, weight, gamma, beta, eps):
    """v3d_pillar_train_fwd: -> rows (M, CH) f32, winner (M, CH) i32, bn (4, CH) f32 = batch mean, biased variance, scale, shift,
    moments f64 (kept for the backward); three launches, no host read.  M >= 1."""
    L.require_gpu("pillar_train_forward", features, occupancy, coordinates, weight, gamma, beta)
    features, weight = L.as_f32("pillar_train_forward", features), L.as_f32("pillar_train_forward", weight)
    occupancy, coordinates = L.as_i32("pillar_train_forward", occupancy), L.as_i32("pillar_train_forward", coordinates)
    gamma, beta = L.as_f32("pillar_train_forward", gamma), L.as_f32("pillar_train_forward", beta)
    M, P, C = features.shape
    CH, K = weight.shape
    dev = features.device
    rows = torch.empty((M, CH), dtype=torch.float32, device=dev)
    winner = torch.empty((M, CH), dtype=torch.int32, device=dev)
    bn = torch.empty((4, CH), dtype=torch.float32, device=dev)
    moments = torch.empty(K + K * (K + 1) // 2, dtype=torch.float64, device=dev)
    lib = L.lib()
    ws = L.workspace(lib.v3d_pillar_train_workspace(M, P, C, CH), dev)
    with L.device_guard(dev):
        L.check(lib.v3d_pillar_train_fwd(L.ptr(features), L.ptr(occupancy), L.ptr(coordinates), M, P, C, L.host_f32(geom), L.ptr(weight), CH,
                                         L.ptr(gamma), L.ptr(beta), float(eps), L.ptr(rows), L.ptr(winner), L.ptr(bn), L.ptr(moments),
                                         L.ptr(ws), ws.numel(), L.stream_ptr()), "pillar_train_forward")
    return rows, winner, bn, moments


def pillar_train_backward(features, occupancy, coordinates, geom, weight, gamma, eps, rows, winner, d_rows, moments):
    """v3d_pillar_train_bwd: -> dW (CH, K), d_gamma (CH), d_beta (CH) f32; two launches, no host read."""
    L.require_gpu("pillar_train_backward", features, d_rows)
    d_rows = L.as_f32("pillar_train_backward", d_rows)
    winner = L.as_i32("pillar_train_backward", winner)
    M, P, C = features.shape
    CH, K = weight.shape
    dev = features.device
    dW = torch.empty((CH, K), dtype=torch.float32, device=dev)
    d_gamma = torch.empty(CH, dtype=torch.float32, device=dev)
    d_beta = torch.empty(CH, dtype=torch.float32, device=dev)
    lib = L.lib()
    ws = L.workspace(lib.v3d_pillar_train_workspace(M, P, C, CH), dev)
    with L.device_guard(dev):
        L.check(lib.v3d_pillar_train_bwd(L.ptr(features), L.ptr(occupancy), L.ptr(coordinates), M, P, C, L.host_f32(geom), L.ptr(weight), CH,
                                         L.ptr(gamma), float(eps), L.ptr(rows), L.ptr(winner), L.ptr(d_rows), L.ptr(moments), L.ptr(dW),
                                         L.ptr(d_gamma), L.ptr(d_beta), L.ptr(ws), ws.numel(), L.stream_ptr()), "pillar_train_backward")
    return dW, d_gamma, d_beta


class PillarEncodeFunction(torch.autograd.Function):
    """Training forward / backward of the encoder on csrc/pillar.hip: (features, occupancy, coordinates, geom, eps, weight, gamma,
    beta) -> rows, winner, bn (mean, biased variance, scale, shift); only `rows` carries a gradient, to weight, gamma and beta."""

    @staticmethod
    def forward(ctx, features, occupancy, coordinates, geom, eps, weight, gamma, beta):
        features, occupancy, coordinates = features.contiguous(), occupancy.contiguous(), coordinates.contiguous()
        weight, gamma = weight.detach().contiguous(), gamma.detach().contiguous()
        rows, winner, bn, moments = pillar_train_forward(features, occupancy, coordinates, geom, weight, gamma, beta.detach(), eps)
        ctx.save_for_backward(features, occupancy, coordinates, weight, gamma, rows, winner, moments)
        ctx.geom, ctx.eps = geom, eps
        ctx.mark_non_differentiable(winner, bn)
        return rows, winner, bn

    @staticmethod
    def backward(ctx, d_rows, _d_winner, _d_bn):
        features, occupancy, coordinates, weight, gamma, rows, winner, moments = ctx.saved_tensors
        dW, d_gamma, d_beta = pillar_train_backward(features, occupancy, coordinates, ctx.geom, weight, gamma, ctx.eps, rows, winner,
                                                    d_rows.contiguous(), moments)
        return None, None, None, None, None, dW, d_gamma, d_beta


class PillarFeatureNet(nn.Module):
    """item (features, occupancy, coordinates, batch_size of the Preprocessor) -> BEV map (B, CHANNELS, H, W) f32."""

    native = True  # False: forward_torch for every call (A/B measurements, the cross-check of the tests)

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.opt = pillar_config(cfg)
        self.channels = int(self.opt["CHANNELS"])
        self.geom, self.map_shape = pillar_geometry(cfg)
        self.linear = nn.Linear(int(cfg.C_IN) + 6, self.channels, bias=False)
        self.norm = nn.BatchNorm1d(self.channels, eps=1e-3, momentum=0.01)
        self.last_winner = None  # (M, CHANNELS) i32 of the last native training forward (diagnostics, tests)

    # ---- the canvas
    def canvas(self, rows, coordinates, batch_size):
        H, W = self.map_shape
        if rows.is_cuda:
            # the canvas is one cell tall: the z index is written as 0 whatever a hand-built item holds (one small elementwise launch;
            # no host read -- check_coordinates is the loud form), so no row can land outside its (b, y, x) column
            mask = self.__dict__.get("_z_mask")
            if mask is None or mask.device != coordinates.device:
                mask = self.__dict__["_z_mask"] = torch.tensor([1, 0, 1, 1], dtype=torch.int32, device=coordinates.device)
            flat = coordinates.int() * mask
            dense = spconv.SparseConvTensor(rows, flat, [1, H, W], batch_size).dense()  # differentiable where rows need it
            return dense.reshape(int(batch_size), rows.shape[1], H, W)
        out = rows.new_zeros((int(batch_size), H, W, rows.shape[1]))
        co = coordinates.long()
        return out.index_put((co[:, 0], co[:, 2], co[:, 3]), rows).permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def check_coordinates(coordinates):
        """Pillars have z index 0 (pillar_geometry refuses every grid that could give another).  One host read: for callers that
        build `coordinates` themselves; forward() does not stall on it."""
        if coordinates.numel() and int(coordinates[:, 1].abs().max()) != 0:
            raise ValueError("PillarFeatureNet: coordinates[:, 1] (the z index) must be 0: a pillar spans the whole z extent")

    def _check(self, item):
        features, coordinates = item["features"], item["coordinates"]
        if features.dim() != 3 or features.shape[2] + 6 != self.linear.in_features:
            raise ValueError(f"PillarFeatureNet: features must be (M, P, {self.linear.in_features - 6}), got {tuple(features.shape)}")
        if item["occupancy"].shape[0] != features.shape[0] or coordinates.shape != (features.shape[0], 4):
            raise ValueError("PillarFeatureNet: occupancy (M) and coordinates (M, 4) must match features (M, P, C)")

    # ---- eval-mode BatchNorm folded to scale / shift, cached until a tensor changes (as RPN._folded)
    def _folded(self):
        n = self.norm

        def build():
            with torch.no_grad():
                scale = torch.rsqrt(n.running_var + n.eps) * n.weight
                return scale.contiguous(), (n.bias - n.running_mean * scale).contiguous()
        return cached(self, "_fold_cache", (n.running_mean, n.running_var, n.weight, n.bias), build)

    def forward(self, item):
        self._check(item)
        features = item["features"]
        if not (self.native and features.is_cuda and features.dtype == torch.float32 and _native_shape(features, self.channels)
                and item["occupancy"].dtype == torch.int32 and item["coordinates"].dtype == torch.int32):
            return self.forward_torch(item)
        occupancy, coordinates, B = item["occupancy"], item["coordinates"], int(item["batch_size"])
        if features.shape[0] == 0:
            return features.new_zeros((B, self.channels) + self.map_shape)
        if not self.training:
            if torch.is_grad_enabled():  # (autograd through an eval-mode encoder: the torch statement carries it, as RPN.forward)
                return self.forward_torch(item)
            scale, shift = self._folded()
            rows = pillar_encode(features, occupancy, coordinates, self.geom, self.linear.weight.detach(), scale, shift)
            return self.canvas(rows, coordinates, B)
        rows, winner, bn = PillarEncodeFunction.apply(features, occupancy, coordinates, self.geom, float(self.norm.eps), self.linear.weight,
                                                      self.norm.weight, self.norm.bias)
        self.last_winner = winner
        self._update_running(bn[0], bn[1], features.shape[0] * features.shape[1])
        return self.canvas(rows, coordinates, B)

    def _update_running(self, mean, var, rows):
        """nn.BatchNorm1d's update from the batch mean and BIASED variance over `rows` rows: unbiased variance, momentum."""
        n = self.norm
        if not n.track_running_stats or n.running_mean is None:
            return
        with torch.no_grad():
            n.num_batches_tracked += 1
            mom = n.momentum if n.momentum is not None else 1.0 / float(n.num_batches_tracked)
            n.running_mean.mul_(1 - mom).add_(mean, alpha=mom)
            n.running_var.mul_(1 - mom).add_(var * (rows / max(rows - 1, 1)), alpha=mom)

    def forward_torch(self, item, winner=None):
        """The op-by-op torch statement of the encoder (any device, any P / C / CHANNELS).  winner (M, CHANNELS) integer: the maximum
        is READ at these rows instead of searched (-1 = the padded candidate, read at the pillar's last slot, a zero-feature row) --
        the statement of what PillarEncodeFunction differentiates, for cross-checks that must not depend on near-tied maxima."""
        self._check(item)
        dtype = self.linear.weight.dtype  # (fp32; a .double() module states the same in float64)
        features, occupancy, coordinates, B = item["features"].to(dtype), item["occupancy"], item["coordinates"], int(item["batch_size"])
        M, P, C = features.shape
        if M == 0:
            return features.new_zeros((B, self.channels) + self.map_shape)
        g = torch.tensor(self.geom, dtype=dtype, device=features.device)
        real = (torch.arange(P, device=features.device)[None, :] < occupancy[:, None]).unsqueeze(-1)  # (M, P, 1)
        xyz = features[..., :3]
        mean = (xyz * real).sum(dim=1, keepdim=True) / occupancy.to(dtype).view(M, 1, 1)
        centre = (coordinates[:, [3, 2, 1]].to(dtype) * g[:3] + g[3:]).unsqueeze(1)
        f = torch.cat([features, xyz - mean, xyz - centre], dim=-1) * real
        y = self.norm(self.linear(f).view(M * P, self.channels)).view(M, P, self.channels)
        if winner is None:
            rows = torch.max(F.relu(y), dim=1).values
        else:
            at = torch.where(winner < 0, P - 1, winner).long()
            rows = torch.take_along_dim(F.relu(y), at.unsqueeze(1), dim=1).squeeze(1)
        return self.canvas(rows, coordinates, B)


# ------------------------------------------------------------------------------------------------------------- the dynamic encoder
def _dynamic_args(what, points, point_voxel, voxel_mean, occupancy, coordinates):
    points, voxel_mean = L.as_f32(what, points), L.as_f32(what, voxel_mean)
    return points, L.as_i32(what, point_voxel), voxel_mean, L.as_i32(what, occupancy), L.as_i32(what, coordinates)


def pillar_dynamic_encode(points, point_voxel, voxel_mean, occupancy, coordinates, geom, weight, scale, shift, want_winner=False):
    """v3d_pillar_dynamic_encode (eval): -> rows (M, CHANNELS) f32 [, winner (M, CHANNELS) i32 = flat point indices]; three launches,
    no host read."""
    what = "pillar_dynamic_encode"
    L.require_gpu(what, points, point_voxel, voxel_mean, occupancy, coordinates, weight, scale, shift)
    points, point_voxel, voxel_mean, occupancy, coordinates = _dynamic_args(what, points, point_voxel, voxel_mean, occupancy, coordinates)
    weight, scale, shift = L.as_f32(what, weight), L.as_f32(what, scale), L.as_f32(what, shift)
    (N, C), M, CH, dev = points.shape, voxel_mean.shape[0], weight.shape[0], points.device
    rows = torch.empty((M, CH), dtype=torch.float32, device=dev)
    winner = torch.empty((M, CH), dtype=torch.int32, device=dev) if want_winner else None
    lib = L.lib()
    ws = L.workspace(lib.v3d_pillar_dynamic_workspace(N, M, C, CH), dev)
    with L.device_guard(dev):
        L.check(lib.v3d_pillar_dynamic_encode(L.ptr(points), L.ptr(point_voxel), N, L.ptr(voxel_mean), L.ptr(occupancy), L.ptr(coordinates), M, C,
                                              L.host_f32(geom), L.ptr(weight), CH, L.ptr(scale), L.ptr(shift), L.ptr(rows),
                                              L.ptr(winner) if want_winner else None, L.ptr(ws), ws.numel(), L.stream_ptr()), what)
    return (rows, winner) if want_winner else rows


def pillar_dynamic_train_forward(points, point_voxel, voxel_mean, occupancy, coordinates, geom, weight, gamma, beta, eps):
    """v3d_pillar_dynamic_train_fwd: -> rows (M, CH) f32, winner (M, CH) i32 (flat point indices), bn (4, CH) f32 = batch mean, biased
    variance, scale, shift over the kept points, moments f64 whose LAST entry is N_kept (kept for the backward); five launches, no host
    read.  M >= 1."""
    what = "pillar_dynamic_train_forward"
    L.require_gpu(what, points, point_voxel, voxel_mean, occupancy, coordinates, weight, gamma, beta)
    points, point_voxel, voxel_mean, occupancy, coordinates = _dynamic_args(what, points, point_voxel, voxel_mean, occupancy, coordinates)
    weight, gamma, beta = L.as_f32(what, weight), L.as_f32(what, gamma), L.as_f32(what, beta)
    (N, C), M, (CH, K), dev = points.shape, voxel_mean.shape[0], weight.shape, points.device
    rows = torch.empty((M, CH), dtype=torch.float32, device=dev)
    winner = torch.empty((M, CH), dtype=torch.int32, device=dev)
    bn = torch.empty((4, CH), dtype=torch.float32, device=dev)
    moments = torch.empty(K + K * (K + 1) // 2 + 1, dtype=torch.float64, device=dev)
    lib = L.lib()
    ws = L.workspace(lib.v3d_pillar_dynamic_workspace(N, M, C, CH), dev)
    with L.device_guard(dev):
        L.check(lib.v3d_pillar_dynamic_train_fwd(L.ptr(points), L.ptr(point_voxel), N, L.ptr(voxel_mean), L.ptr(occupancy), L.ptr(coordinates), M,
                                                 C, L.host_f32(geom), L.ptr(weight), CH, L.ptr(gamma), L.ptr(beta), float(eps), L.ptr(rows),
                                                 L.ptr(winner), L.ptr(bn), L.ptr(moments), L.ptr(ws), ws.numel(), L.stream_ptr()), what)
    return rows, winner, bn, moments


def pillar_dynamic_train_backward(points, point_voxel, voxel_mean, coordinates, geom, weight, gamma, eps, rows, winner, d_rows, moments):
    """v3d_pillar_dynamic_train_bwd: -> dW (CH, K), d_gamma (CH), d_beta (CH) f32; two launches, no host read."""
    what = "pillar_dynamic_train_backward"
    L.require_gpu(what, points, d_rows)
    d_rows, winner = L.as_f32(what, d_rows), L.as_i32(what, winner)
    (N, C), M, (CH, K), dev = points.shape, voxel_mean.shape[0], weight.shape, points.device
    dW = torch.empty((CH, K), dtype=torch.float32, device=dev)
    d_gamma = torch.empty(CH, dtype=torch.float32, device=dev)
    d_beta = torch.empty(CH, dtype=torch.float32, device=dev)
    lib = L.lib()
    ws = L.workspace(lib.v3d_pillar_dynamic_workspace(N, M, C, CH), dev)
    with L.device_guard(dev):
        L.check(lib.v3d_pillar_dynamic_train_bwd(L.ptr(points), L.ptr(point_voxel), N, L.ptr(voxel_mean), L.ptr(coordinates), M, C,
                                                 L.host_f32(geom), L.ptr(weight), CH, L.ptr(gamma), float(eps), L.ptr(rows), L.ptr(winner),
                                                 L.ptr(d_rows), L.ptr(moments), L.ptr(dW), L.ptr(d_gamma), L.ptr(d_beta), L.ptr(ws), ws.numel(),
                                                 L.stream_ptr()), what)
    return dW, d_gamma, d_beta


class DynamicPillarEncodeFunction(torch.autograd.Function):
    """Training forward / backward of the dynamic encoder on csrc/pillar.hip: (points, point_voxel, voxel_mean, occupancy, coordinates,
    geom, eps, weight, gamma, beta) -> rows, winner, bn, moments; only `rows` carries a gradient, to weight, gamma and beta."""

    @staticmethod
    def forward(ctx, points, point_voxel, voxel_mean, occupancy, coordinates, geom, eps, weight, gamma, beta):
        what = "DynamicPillarEncodeFunction"
        points, point_voxel, voxel_mean, occupancy, coordinates = _dynamic_args(what, points, point_voxel, voxel_mean, occupancy, coordinates)
        weight, gamma = weight.detach().contiguous(), gamma.detach().contiguous()
        rows, winner, bn, moments = pillar_dynamic_train_forward(points, point_voxel, voxel_mean, occupancy, coordinates, geom, weight, gamma,
                                                                 beta.detach(), eps)
        ctx.save_for_backward(points, point_voxel, voxel_mean, coordinates, weight, gamma, rows, winner, moments)
        ctx.geom, ctx.eps = geom, eps
        ctx.mark_non_differentiable(winner, bn, moments)
        return rows, winner, bn, moments

    @staticmethod
    def backward(ctx, d_rows, _d_winner, _d_bn, _d_moments):
        points, point_voxel, voxel_mean, coordinates, weight, gamma, rows, winner, moments = ctx.saved_tensors
        dW, d_gamma, d_beta = pillar_dynamic_train_backward(points, point_voxel, voxel_mean, coordinates, ctx.geom, weight, gamma, ctx.eps, rows,
                                                            winner, d_rows.contiguous(), moments)
        return None, None, None, None, None, None, None, dW, d_gamma, d_beta


class DynamicPillarFeatureNet(PillarFeatureNet):
    """The dynamic pillar encoder (DynamicPillarVFE of MVF, arXiv 1910.06528), opt-in: cfg.PILLAR.DYNAMIC.  item (flat_points,
    point_voxel, voxel_mean, occupancy, coordinates, batch_size of the Preprocessor in that mode) -> BEV map (B, CHANNELS, H, W) f32.

    EVERY point of a pillar counts (no MAX_OCCUPANCY, no slot tensor): a kept point i of pillar v = point_voxel[i] becomes [its C
    channels | xyz - voxel_mean[v, :3] | xyz - pillar centre], linear (no bias) -> BatchNorm1d -> ReLU -> maximum over the pillar's
    points (csrc/pillar_device.h "The DYNAMIC encoder").  Same parameters (`linear`, `norm`), same state_dict keys and the same canvas
    as PillarFeatureNet, so a checkpoint loads into either -- but the batch population of the BatchNorm differs: the hard form counts
    all M * P rows, padded ones included (y = 0), this one the N_kept = sum(occupancy) real points only, so batch and running
    statistics of the two are not interchangeable in training.

    forward runs csrc/pillar.hip on CUDA fp32 tensors within the native limits (3 <= C <= 8, CHANNELS 64 or 128, at most 2^22 points):
    three launches in eval mode, five forwards and two backwards in training (DynamicPillarEncodeFunction); forward_torch is the
    op-by-op statement, the path of any other device / C / CHANNELS.  last_winner: (M, CHANNELS) i32 FLAT point indices."""

    def _check(self, item):
        points, pv, vm = item["flat_points"], item["point_voxel"], item["voxel_mean"]
        C = self.linear.in_features - 6
        if points.dim() != 2 or points.shape[1] != C:
            raise ValueError(f"DynamicPillarFeatureNet: flat_points must be (N, {C}), got {tuple(points.shape)}")
        if pv.shape != (points.shape[0],):
            raise ValueError("DynamicPillarFeatureNet: point_voxel (N) must match flat_points (N, C)")
        if vm.dim() != 2 or vm.shape[1] != C:
            raise ValueError(f"DynamicPillarFeatureNet: voxel_mean must be (M, {C}), got {tuple(vm.shape)}")
        if item["occupancy"].shape != (vm.shape[0],) or item["coordinates"].shape != (vm.shape[0], 4):
            raise ValueError("DynamicPillarFeatureNet: occupancy (M) and coordinates (M, 4) must match voxel_mean (M, C)")

    def _native_item(self, item):
        points, vm = item["flat_points"], item["voxel_mean"]
        return (self.native and points.is_cuda and points.dtype == torch.float32 and vm.dtype == torch.float32
                and MIN_C <= points.shape[1] <= MAX_C and self.channels in WIDTHS and points.shape[0] <= MAX_POINTS
                and all(item[k].dtype == torch.int32 for k in ("point_voxel", "occupancy", "coordinates")))

    def forward(self, item):
        self._check(item)
        if not self._native_item(item):
            return self.forward_torch(item)
        points, pv, vm = item["flat_points"], item["point_voxel"], item["voxel_mean"]
        occupancy, coordinates, B = item["occupancy"], item["coordinates"], int(item["batch_size"])
        if vm.shape[0] == 0:
            return vm.new_zeros((B, self.channels) + self.map_shape)
        if not self.training:
            if torch.is_grad_enabled():  # (autograd through an eval-mode encoder: the torch statement carries it)
                return self.forward_torch(item)
            scale, shift = self._folded()
            rows = pillar_dynamic_encode(points, pv, vm, occupancy, coordinates, self.geom, self.linear.weight.detach(), scale, shift)
            return self.canvas(rows, coordinates, B)
        rows, winner, bn, moments = DynamicPillarEncodeFunction.apply(points, pv, vm, occupancy, coordinates, self.geom, float(self.norm.eps),
                                                                      self.linear.weight, self.norm.weight, self.norm.bias)
        self.last_winner = winner
        self._update_running_counted(bn[0], bn[1], moments[-1])
        return self.canvas(rows, coordinates, B)

    def _update_running_counted(self, mean, var, n_kept):
        """nn.BatchNorm1d's update from the batch mean and BIASED variance over n_kept rows, n_kept a 0-d tensor on the device (no
        host read): unbiased factor n / max(n - 1, 1), momentum."""
        n = self.norm
        if not n.track_running_stats or n.running_mean is None:
            return
        with torch.no_grad():
            n.num_batches_tracked += 1
            mom = n.momentum if n.momentum is not None else 1.0 / float(n.num_batches_tracked)
            count = n_kept.to(torch.float64)
            factor = (count / torch.clamp(count - 1, min=1)).to(n.running_var.dtype)
            n.running_mean.mul_(1 - mom).add_(mean.detach().to(n.running_mean.dtype), alpha=mom)
            n.running_var.mul_(1 - mom).add_(var.detach().to(n.running_var.dtype) * factor, alpha=mom)

    def forward_torch(self, item, winner=None):
        """The op-by-op torch statement of the dynamic encoder (any device, any C / CHANNELS).  The batch statistics are stated
        explicitly -- mean and biased variance over the kept rows -- so that a single kept point is legal (nn.BatchNorm1d refuses one
        row).  winner (M, CHANNELS) integer: the maximum is READ at these flat point indices instead of searched (-1: no point, a zero)
        -- the statement of what DynamicPillarEncodeFunction differentiates."""
        self._check(item)
        dtype = self.linear.weight.dtype  # (fp32; a .double() module states the same in float64)
        points, pv, vm = item["flat_points"].to(dtype), item["point_voxel"].long(), item["voxel_mean"].to(dtype)
        coordinates, B = item["coordinates"], int(item["batch_size"])
        M = vm.shape[0]
        if M == 0:
            return vm.new_zeros((B, self.channels) + self.map_shape)
        kept = ((pv >= 0) & (pv < M)).nonzero().squeeze(1)  # flat indices of the kept points, ascending
        p, v = points[kept], pv[kept]
        g = torch.tensor(self.geom, dtype=dtype, device=points.device)
        xyz = p[:, :3]
        centre = coordinates[:, [3, 2, 1]].to(dtype) * g[:3] + g[3:]
        f = torch.cat([p, xyz - vm[v, :3], xyz - centre[v]], dim=1)
        y = self.linear(f)
        n = self.norm
        if self.training:
            count = y.shape[0]
            mean = y.sum(dim=0) / count
            var = ((y - mean) ** 2).sum(dim=0) / count
            self._update_running_counted(mean, var, torch.tensor(float(count), dtype=torch.float64, device=y.device))
        else:
            mean, var = n.running_mean, n.running_var
        a = F.relu((y - mean) / torch.sqrt(var + n.eps) * n.weight + n.bias)
        if winner is None:
            rows = a.new_zeros((M, self.channels)).scatter_reduce(0, v[:, None].expand(-1, self.channels), a, "amax", include_self=False)
        else:
            where = torch.full((points.shape[0] + 1,), -1, dtype=torch.long, device=points.device)  # flat index -> row of `a`; [-1] stays -1
            where[kept] = torch.arange(kept.shape[0], device=points.device)
            at = where[winner.long().clamp(min=-1, max=points.shape[0])]
            rows = torch.where(at >= 0, torch.gather(a, 0, at.clamp(min=0)), a.new_zeros(()))
        return self.canvas(rows, coordinates, B)

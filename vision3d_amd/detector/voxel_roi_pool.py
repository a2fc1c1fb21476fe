"""Voxel RoI pooling for PV-RCNN's stage 2 (the pooling of Voxel R-CNN, arXiv 2012.15712), opt-in through `cfg.VOXELPOOL.ENABLED`:
the G^3 regular grid points of every RoI query the sparse backbone's own voxels by integer coordinates and a small PointNet pools
the voxels found -- stage 2 without keypoints (no furthest-point sampling, no set abstraction, no BEV lookup).  Upstream has no
statement of it; the definition is this repository's, restated in numpy in tests/voxel_roi_pool_ref.py:

  grid points   centre + Rz(yaw) (((i + .5) / G - .5) w, ((j + .5) / G - .5) l, ((k + .5) / G - .5) h), point (i * G + j) * G + k:
                the product of roi_grid_pool.gridpoints with those fixed samples.
  voxel query   per point p and level l (stride s, size = base_voxel_size * s rounded in float32, active coordinates (b, z, y, x)):
                home cell v = floor((p - voxel_offset) / size); candidates v + (dz, dy, dx), |d| <= RANGE[l] = (rz, ry, rx), in ascending
                (dz, dy, dx) order; a hit lies inside the level's shape, is active in the RoI's own frame and has
                |centre(u) - p|^2 < RADIUS[l]^2 (strict, float32; centre(u) = (u * size + voxel_offset) + size / 2); the first NSAMPLE
                hits are taken, missing slots repeat the first hit; no hit: indices -1, pooled features exactly zero.
  pooling       row of a hit = [centre(u) - p, feat(u)] through the level's shared MLP (Linear without bias + BatchNorm(eps 1e-3) + ReLU
                per layer), max over the slots; levels concatenated on channels; per RoI the (G^3 * C) row in (grid point, channel)
                order through MLP(MLPS_REDUCTION) -> (B, n_roi, 256), what RefinementLayer takes.

A level is handed over as `VoxelLevel`: its features and coordinates (all `cap` rows of the backbone plan's buffers, the live count in
device memory, or exactly the live rows), its shape and its stride.  Inference (CUDA, float32, eval, no autograd) runs per level one
v3d_voxel_query, one v3d_linear_rows over the active voxels (the first layer's feature part, once per voxel instead of once per
neighbour) and one v3d_voxel_pool_pair (csrc/voxel_pool.hip) writing the level's column block -- no host read of a row count, so the
chain can be captured.  The torch statements are kept beside them: the training path (differentiable in the features and the
parameters), the fallback beyond the kernels' limits, and the cross-check."""
from collections import namedtuple

import torch
from torch import nn

from ..stamp import cached
from .layers import MLP
from .roi_grid_pool import gridpoints

VOXELPOOL_DEFAULTS = dict(ENABLED=False, GRID=6, LEVELS=[2, 3, 4], RANGE=[[2, 2, 2], [2, 2, 2], [1, 2, 2]], RADIUS=[0.4, 0.8, 1.6],
                          NSAMPLE=16, MLPS=[[32, 32], [32, 32], [32, 32]], MLPS_REDUCTION=None, LEVEL_CHANNELS=None)
BN_EPS = 1e-3
MAX_ROWS, MAX_NSAMPLE, MAX_RANGE = 1 << 22, 64, 7  # limits of csrc/voxel_pool.hip: beyond them the torch statements run
PAIR_WIDTHS = {(16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64)}

# features (cap, C), coords (cap, 4) int32 = (b, z, y, x), n: (1,) int32 DEVICE count of live rows or None (every row is live),
# shape [D, H, W], stride of the level against the input grid
VoxelLevel = namedtuple("VoxelLevel", "features coords n shape stride")


def voxelpool_config(cfg):
    """-> the keys of cfg.VOXELPOOL over their defaults (a config written before the key existed means "disabled")."""
    out = dict(VOXELPOOL_DEFAULTS)
    out.update(cfg.get("VOXELPOOL") or {})
    return out


def level_channels(cfg, levels):
    """Feature channels of the backbone levels: level 1 is the voxelized input, level k + 1 the output of backbone stage k."""
    from .sparse_cnn import FHD_STAGES
    table = [int(cfg.C_IN)] + [stage[-1][1] for stage in FHD_STAGES]
    return [table[int(lv) - 1] for lv in levels]


def voxel_query(points, rows_per_frame, level, scale, offset, rng, radius, nsample):
    """The native query of one level (v3d_voxel_query): points (R, 3) float32 on the GPU, frame of a row = row // rows_per_frame.
    -> idx (R, nsample) int32, empty (R,) uint8."""
    from .. import _lib as L
    L.require_gpu("voxel_query", points, level.coords)
    pts = L.as_f32("voxel_query", points).reshape(-1, 3)
    coords = L.as_i32("voxel_query", level.coords)
    cap = coords.shape[0]
    n = level.n if level.n is not None else torch.full((1,), cap, dtype=torch.int32, device=pts.device)
    rows = pts.shape[0]
    idx = torch.empty((rows, int(nsample)), dtype=torch.int32, device=pts.device)
    empty = torch.empty(rows, dtype=torch.uint8, device=pts.device)
    workspace = L.workspace(L.lib().v3d_voxel_query_workspace(cap), pts.device)
    with L.device_guard(pts.device):
        L.check(L.lib().v3d_voxel_query(L.ptr(pts), rows, int(rows_per_frame), L.ptr(coords), L.ptr(n), cap, L.host_i32(level.shape),
                                        L.host_f32(scale), L.host_f32(offset), L.host_i32(rng), float(radius), int(nsample), L.ptr(idx),
                                        L.ptr(empty), L.ptr(workspace), workspace.numel(), L.stream_ptr()), "voxel_query")
    return idx, empty


def voxel_pool_pair(p, coords, points, idx, scale, offset, wx, b1, w2, b2, out):
    """The native pooling of one level (v3d_voxel_pool_pair): p (cap, K1) first-layer products of the voxels, coords (cap, 4), points
    (R, 3), idx (R, ns) from `voxel_query`, wx (3, K1), b1 (K1), w2 (K1, Nout), b2 (Nout); `out` (R, Nout) a view with unit column
    stride (a column block of a wider matrix), written in place."""
    from .. import _lib as L
    L.require_gpu("voxel_pool_pair", p, coords, points, idx, out)
    rows, ns = idx.shape
    k1, nout = w2.shape
    if out.dim() != 2 or out.shape != (rows, nout) or out.stride(1) != 1 or out.dtype != torch.float32 or p.dtype != torch.float32 \
            or p.dim() != 2 or p.stride(1) != 1 or p.shape[1] < k1 or p.shape[0] != coords.shape[0] or tuple(wx.shape) != (3, k1) \
            or b1.numel() != k1 or b2.numel() != nout or points.shape != (rows, 3) or not idx.is_contiguous():
        raise RuntimeError("voxel_pool_pair: mismatched shapes, or `out` is not a float32 (R, Nout) view with unit column stride")
    pts = L.as_f32("voxel_pool_pair", points)
    coords = L.as_i32("voxel_pool_pair", coords)
    ldo = out.stride(0) if rows > 1 else max(out.stride(0), nout)
    ldp = p.stride(0) if p.shape[0] > 1 else max(p.stride(0), k1)
    with L.device_guard(out.device):
        L.check(L.lib().v3d_voxel_pool_pair(L.ptr(p), ldp, L.ptr(coords), coords.shape[0], L.ptr(pts), L.ptr(idx), rows, ns,
                                            L.host_f32(scale), L.host_f32(offset), k1, L.ptr(L.as_f32("voxel_pool_pair", wx)),
                                            L.ptr(L.as_f32("voxel_pool_pair", b1)), L.ptr(L.as_f32("voxel_pool_pair", w2)),
                                            L.ptr(L.as_f32("voxel_pool_pair", b2)), nout, L.ptr(out), ldo, L.stream_ptr()), "voxel_pool_pair")
    return out


class VoxelRoiPool(nn.Module):

    native = True  # False: the torch statements everywhere (the cross-check of the tests)

    def __init__(self, cfg, voxel_offset=None, base_voxel_size=None):
        super().__init__()
        self.cfg = cfg
        vp = voxelpool_config(cfg)
        self.grid = int(vp["GRID"])
        self.levels = [int(v) for v in vp["LEVELS"]]
        self.ranges = [[int(v) for v in r] for r in vp["RANGE"]]
        self.radii = [float(v) for v in vp["RADIUS"]]
        self.nsample = int(vp["NSAMPLE"])
        widths = [[int(v) for v in m] for m in vp["MLPS"]]
        if not (len(self.levels) == len(self.ranges) == len(self.radii) == len(widths)) or any(len(r) != 3 for r in self.ranges):
            raise ValueError("VOXELPOOL: LEVELS, RANGE ([rz, ry, rx] per level), RADIUS and MLPS need one entry per level")
        if self.grid < 1 or self.nsample < 1 or any(r <= 0 for r in self.radii) or any(v < 0 for r in self.ranges for v in r):
            raise ValueError("VOXELPOOL: GRID and NSAMPLE >= 1, RADIUS > 0, RANGE >= 0")
        if any(lv < 1 or lv > len(cfg.STRIDES) for lv in self.levels):
            raise ValueError(f"VOXELPOOL.LEVELS: levels 1 .. {len(cfg.STRIDES)} exist (1: the voxelized input)")
        channels = vp["LEVEL_CHANNELS"] or level_channels(cfg, self.levels)
        self.strides = [int(cfg.STRIDES[lv - 1]) for lv in self.levels]
        self.mlps = nn.ModuleList(MLP([3 + int(c), *w], bias=False, bn=True, relu=True) for c, w in zip(channels, widths))
        for m in self.mlps.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.eps = BN_EPS
        c_total = sum(w[-1] for w in widths)
        reduction = vp["MLPS_REDUCTION"] or [self.grid ** 3 * c_total, 256, 256]
        if int(reduction[0]) != self.grid ** 3 * c_total:
            raise ValueError(f"VOXELPOOL.MLPS_REDUCTION[0] must be GRID^3 * {c_total} = {self.grid ** 3 * c_total}")
        self.reduction = MLP([int(v) for v in reduction])
        for name, values in (("base_voxel_size", cfg.VOXEL_SIZE), ("voxel_offset", cfg.GRID_BOUNDS[:3])):
            given = base_voxel_size if name == "base_voxel_size" else voxel_offset
            t = given.detach().clone().float() if given is not None else torch.tensor(values, dtype=torch.float32)
            self.register_buffer(name, t, persistent=False)

    # ---- geometry
    def level_geometry(self, k):
        """((sx, sy, sz), (ox, oy, oz)) of level k as python floats: base_voxel_size * stride rounded in float32 like the tensor product
        (SparseCNNBase.to_global), once, on the host."""
        cache = self.__dict__.setdefault("_geometry", {})
        if k not in cache:
            cache[k] = ((self.base_voxel_size.detach().cpu().float() * self.strides[k]).tolist(), self.voxel_offset.detach().cpu().float().tolist())
        return cache[k]

    def grid_points(self, boxes):
        """boxes (B, n, 7) -> (B, n, G^3, 3): `gridpoints` with the fixed samples ((i + .5) / G, (j + .5) / G, (k + .5) / G)."""
        b, n = boxes.shape[:2]
        cache = self.__dict__.setdefault("_samples", {})
        key = (b, n, str(boxes.device), boxes.dtype)
        if key not in cache:
            t = (torch.arange(self.grid, dtype=torch.float32) + 0.5) / self.grid
            cell = torch.stack(torch.meshgrid(t, t, t, indexing="ij"), -1).reshape(-1, 3)
            cache.clear()
            cache[key] = cell.to(boxes.device, boxes.dtype).expand(b, n, -1, -1).contiguous()
        return gridpoints(boxes, cache[key])

    # ---- the torch statements
    def _live(self, level):
        """(features, coords) of the level's live rows (a plan's level: one host read of its count)."""
        if level.n is None:
            return level.features, level.coords
        n = min(int(level.n.item()), level.coords.shape[0])
        return level.features[:n], level.coords[:n]

    def centres(self, zyx, k, dtype):
        """integer (..., 3) = (z, y, x) -> (..., 3) = (x, y, z) centres of level k's voxels in `dtype`."""
        size = (self.base_voxel_size * self.strides[k]).to(dtype)
        return (zyx.flip(-1).to(dtype) * size + self.voxel_offset.to(dtype)) + 0.5 * size

    def query_torch(self, points, rows_per_frame, coords, shape, k):
        """points (R, 3), coords (n, 4) live rows of level k -> idx (R, NSAMPLE) int64 (-1: none), empty (R,) bool, op by op."""
        dev, dtype = points.device, points.dtype
        rows, ns = points.shape[0], self.nsample
        if rows == 0 or coords.shape[0] == 0:
            return torch.full((rows, ns), -1, dtype=torch.long, device=dev), torch.ones(rows, dtype=torch.bool, device=dev)
        size = (self.base_voxel_size * self.strides[k]).to(dtype)
        home = torch.floor((points - self.voxel_offset.to(dtype)) / size).clamp(-2 ** 30, 2 ** 30).long().flip(-1)  # (R, 3) = z, y, x
        rz, ry, rx = self.ranges[k]
        window = torch.stack(torch.meshgrid(torch.arange(-rz, rz + 1), torch.arange(-ry, ry + 1), torch.arange(-rx, rx + 1), indexing="ij"),
                             -1).reshape(-1, 3).to(dev)  # ascending (dz, dy, dx)
        cand = home[:, None, :] + window[None]  # (R, W, 3)
        d, h, w = (int(v) for v in shape)
        lim = torch.tensor([d, h, w], device=dev)
        inside = ((cand >= 0) & (cand < lim)).all(-1)
        frame = (torch.arange(rows, device=dev) // int(rows_per_frame))[:, None]
        key = ((frame * d + cand[..., 0]) * h + cand[..., 1]) * w + cand[..., 2]
        co = coords.long()
        site_key = ((co[:, 0] * d + co[:, 1]) * h + co[:, 2]) * w + co[:, 3]
        order = torch.argsort(site_key)
        sorted_key = site_key[order]
        pos = torch.searchsorted(sorted_key, key.reshape(-1)).clamp(max=sorted_key.numel() - 1).reshape(key.shape)
        row = order[pos]
        active = inside & (sorted_key[pos] == key)
        rel = self.centres(cand, k, dtype) - points[:, None, :]
        d2 = (rel[..., 0] * rel[..., 0] + rel[..., 1] * rel[..., 1]) + rel[..., 2] * rel[..., 2]
        radius2 = torch.tensor(self.radii[k], dtype=dtype, device=dev) ** 2
        hit = active & (d2 < radius2)
        count = hit.sum(1)
        first = torch.argsort((~hit).to(torch.uint8), dim=1, stable=True)[:, :ns]  # the hits' window positions in scan order, then the rest
        if first.shape[1] < ns:
            first = torch.cat([first, first[:, :1].expand(-1, ns - first.shape[1])], 1)
        slot = torch.arange(ns, device=dev)[None]
        first = torch.where(slot < count[:, None], first, first[:, :1])
        idx = torch.gather(row, 1, first)
        empty = count == 0
        return torch.where(empty[:, None], torch.full_like(idx, -1), idx), empty

    def pool_torch(self, points, idx, features, coords, k):
        """points (R, 3), idx (R, ns) (-1 rows: empty) -> (R, C_out): the hits' rows through the level's MLP, max over the slots."""
        rows, ns = idx.shape
        mlp = self.mlps[k]
        c_out = [m for m in mlp if isinstance(m, nn.Linear)][-1].out_features
        out = features.new_zeros((rows, c_out))
        live = idx[:, 0] >= 0
        if not bool(live.any()):
            return out
        ii = idx[live].long()
        rel = self.centres(coords[ii][..., 1:4], k, points.dtype) - points[live][:, None, :]
        x = torch.cat([rel.to(features.dtype), features[ii]], -1).reshape(-1, 3 + features.shape[1])
        pooled = nn.Sequential.forward(mlp, x).reshape(ii.shape[0], ns, c_out).max(1).values
        return out.index_put((live.nonzero().squeeze(1),), pooled)

    def forward_torch(self, boxes, levels):
        """boxes (B, n, 7), levels [VoxelLevel] in the order of cfg.VOXELPOOL.LEVELS -> (B, n, 256), op by op (any device / dtype,
        under autograd: differentiable in the levels' features and the parameters; the boxes are constants)."""
        b, n = boxes.shape[:2]
        points = self.grid_points(boxes.detach()).reshape(-1, 3)
        blocks = []
        for k, level in enumerate(levels):
            features, coords = self._live(level)
            idx, _ = self.query_torch(points, n * self.grid ** 3, coords, level.shape, k)
            blocks.append(self.pool_torch(points, idx, features, coords, k))
        per_roi = torch.cat(blocks, -1).reshape(b, n, -1)
        return nn.Sequential.forward(self.reduction, per_roi)

    # ---- the native path
    def native_ok(self, boxes, levels):
        """CUDA, float32, eval, no autograd, two-layer level MLPs of widths the PAIR kernel covers, sizes within its limits."""
        if not self.native or self.training or torch.is_grad_enabled() or not boxes.is_cuda or boxes.dtype != torch.float32 \
                or boxes.dim() != 3 or boxes.shape[-1] != 7 or boxes.shape[0] > 64:
            return False
        rows = boxes.shape[0] * boxes.shape[1] * self.grid ** 3
        if rows == 0 or rows > MAX_ROWS or self.nsample > MAX_NSAMPLE or any(v > MAX_RANGE for r in self.ranges for v in r):
            return False
        for mlp, level in zip(self.mlps, levels):
            lins = [m for m in mlp if isinstance(m, nn.Linear)]
            if len(lins) != 2 or (lins[0].out_features, lins[1].out_features) not in PAIR_WIDTHS or (lins[0].in_features - 3) % 4:
                return False
            f, c = level.features, level.coords
            if not (f.is_cuda and f.dtype == torch.float32 and f.dim() == 2 and f.stride(1) == 1 and f.shape[1] == lins[0].in_features - 3
                    and (f.shape[0] < 2 or f.stride(0) % 4 == 0) and f.data_ptr() % 16 == 0 and c.dtype == torch.int32 and c.is_contiguous()
                    and c.data_ptr() % 16 == 0 and c.shape[0] == f.shape[0] and c.shape[0] < (1 << 24) - 1):
                return False
        return self.reduction.native_ok(boxes)

    def _folded(self, k):
        """Level k's MLP with eval BatchNorm folded in, as the kernels take it: (W1[3:]^T (C, K1), W1[0:3]^T (3, K1), b1 (K1),
        W2^T (K1, Nout), b2 (Nout)), cached until a parameter or running statistic changes."""
        mlp = self.mlps[k]
        tensors = (t for m in mlp for t in list(m._parameters.values()) + list(m._buffers.values()))
        return cached(self, "_fold_cache", tensors, lambda: self._fold(mlp), k)

    @staticmethod
    def _fold(mlp):
        lins = [m for m in mlp if isinstance(m, nn.Linear)]
        bns = [m for m in mlp if isinstance(m, nn.BatchNorm1d)]
        folded = []
        with torch.no_grad():
            for lin, bn in zip(lins, bns):
                scale = bn.weight.float() * torch.rsqrt(bn.running_var.float() + bn.eps)
                folded.append(((lin.weight.float() * scale[:, None]).t().contiguous(), (bn.bias.float() - bn.running_mean.float() * scale).contiguous()))
        (w1, b1), (w2, b2) = folded
        return w1[3:].contiguous(), w1[0:3].contiguous(), b1, w2, b2

    def forward_native(self, boxes, levels):
        """`native_ok` inputs: per level query + first-layer products + pooling into the level's column block of ONE (R, C_total) matrix,
        then the reduction on v3d_linear_rows.  Only enqueues: no host read."""
        from ..pointnet2.pointnet2_utils import linear_rows
        b, n = boxes.shape[:2]
        m = self.grid ** 3
        points = self.grid_points(boxes).reshape(-1, 3)
        widths = [[mod for mod in mlp if isinstance(mod, nn.Linear)][-1].out_features for mlp in self.mlps]
        pooled = torch.empty((b * n * m, sum(widths)), dtype=torch.float32, device=boxes.device)
        col = 0
        for k, (level, width) in enumerate(zip(levels, widths)):
            scale, offset = self.level_geometry(k)
            w1f, wx, b1, w2, b2 = self._folded(k)
            idx, _ = voxel_query(points, n * m, level, scale, offset, self.ranges[k], self.radii[k], self.nsample)
            if level.features.shape[0] > 0:
                p = linear_rows(level.features, w1f)  # (cap, K1): once per voxel (rows beyond the live count are never gathered)
            else:
                p = torch.empty((0, w1f.shape[1]), dtype=torch.float32, device=boxes.device)
            voxel_pool_pair(p, level.coords, points, idx, scale, offset, wx, b1, w2, b2, pooled[:, col:col + width])
            col += width
        return self.reduction.native_forward(pooled.view(b, n, m * pooled.shape[1]))

    def forward(self, boxes, levels):
        if len(levels) != len(self.mlps):
            raise RuntimeError(f"VoxelRoiPool: {len(self.mlps)} levels configured, {len(levels)} handed in")
        if self.native_ok(boxes, levels):
            return self.forward_native(boxes, levels)
        return self.forward_torch(boxes, levels)

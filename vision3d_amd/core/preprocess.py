"""Batch preprocessing with the voxelizer ON THE DEVICE (interface of vision3d/core/preprocess.py:10-79).

`Preprocessor(cfg)(item)` consumes `item['points']` = list of per-frame (Np, C) clouds and adds
  points (B, Np_max, C) f32 | features (M, K, C) f32 | coordinates (M, 4) i32 (b,z,y,x) |
  occupancy (M,) i32 | batch_size int            (all tensors already on the GPU)
-- the same keys/shapes the reference produces on the host (preprocess.py:47-61); the detector's
`.cuda()` calls on them become no-ops.  Voxel order/content equals the sequential reference loop
(first-touch order, first-come slots).  Extra key `voxel_mean` (M, C) carries the fused
VoxelFeatureExtractor output for callers that want to skip `features`.

cfg.DYNAMIC_VOXELIZATION (opt-in): every point of a voxel counts (csrc/voxelize.hip "DYNAMIC").  The item then has
  points | coordinates | occupancy (the TRUE counts) | voxel_mean (order-independent) | point_voxel (sum Np,) i32 | batch_size
and no `features` (the slot tensor does not exist in this mode); same voxels in the same order.

cfg.PILLAR.ENABLED with cfg.PILLAR.DYNAMIC (opt-in, the dynamic pillar encoder): the same dynamic item -- MAX_OCCUPANCY is ignored --
plus `flat_points` (sum Np, C), the concatenation of the frames that `point_voxel` indexes (a key of this mode only).
"""
from collections import defaultdict

import numpy as np
import torch
from torch import nn

from ..spconv.utils import VoxelGenerator, voxelize_batch, voxelize_dynamic_batch
from .config import dynamic_voxel_enabled, pillar_dynamic_enabled, refuse_dynamic_with_pillar


class Preprocessor(nn.Module):

    def __init__(self, cfg, seed=None):
        super().__init__()
        self.cfg = cfg
        refuse_dynamic_with_pillar(cfg)
        self.pillar_dynamic = pillar_dynamic_enabled(cfg)  # cfg.PILLAR.DYNAMIC (opt-in): dynamic pillars, the item keeps `flat_points`
        self.dynamic = dynamic_voxel_enabled(cfg) or self.pillar_dynamic  # cfg.DYNAMIC_VOXELIZATION (opt-in): see forward
        self.voxel_generator = self.build_voxel_generator(cfg)
        self._rng = np.random.default_rng(seed)  # reference pads with unseeded np.random (H12)

    def build_voxel_generator(self, cfg):
        return VoxelGenerator(voxel_size=cfg.VOXEL_SIZE, point_cloud_range=cfg.GRID_BOUNDS,
                              max_voxels=cfg.MAX_VOXELS, max_num_points=cfg.MAX_OCCUPANCY)

    @staticmethod
    def _to_device(p):
        if isinstance(p, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).cuda(non_blocking=True)
        return p.cuda()

    def generate_batch_voxels(self, points):
        """One fused launch sequence for the whole batch (the reference loops frames on the host)."""
        offsets = np.concatenate([[0], np.cumsum([p.shape[0] for p in points])]).astype(np.int64).tolist()
        flat = torch.cat(points, dim=0) if len(points) > 1 else points[0]
        voxels, coords, occ, mean, n_vox = voxelize_batch(flat, offsets, self.cfg.VOXEL_SIZE, self.cfg.GRID_BOUNDS,
                                                          self.cfg.MAX_OCCUPANCY, self.cfg.MAX_VOXELS)
        m = int(n_vox.item())
        return voxels[:m], coords[:m], occ[:m], mean[:m]

    def generate_batch_voxels_dynamic(self, points):
        """cfg.DYNAMIC_VOXELIZATION: every point of a voxel counts.  -> (coordinates, occupancy (true counts), mean, point_voxel (sum N_b,)
        row of every point of the concatenated clouds, -1 = dropped, flat = those clouds).  The one host read brings the status word
        with the count."""
        offsets = np.concatenate([[0], np.cumsum([p.shape[0] for p in points])]).astype(np.int64).tolist()
        flat = torch.cat(points, dim=0) if len(points) > 1 else points[0]
        coords, occ, mean, point_voxel, n_out = voxelize_dynamic_batch(flat, offsets, self.cfg.VOXEL_SIZE, self.cfg.GRID_BOUNDS,
                                                                       self.cfg.MAX_VOXELS)
        m, status = n_out.tolist()
        if status & 1:
            raise ValueError("dynamic voxelization: a point inside GRID_BOUNDS holds a channel value that is not finite or not below "
                             "2^16 in magnitude (the precondition of the exact integer sums; that voxel's mean is NaN)")
        return coords[:m], occ[:m], mean[:m], point_voxel, flat

    def pad_for_batch(self, points):
        """Dense (B, N, C) minibatch; short frames are padded by resampling their own points."""
        n_max = max(p.shape[0] for p in points)
        rows = []
        for p in points:
            pad = n_max - p.shape[0]
            if pad:
                idx = torch.from_numpy(self._rng.integers(0, p.shape[0], pad)).to(p.device)
                p = torch.cat((p, p[idx]))
            rows.append(p)
        return torch.stack(rows, dim=0)

    def forward(self, item):
        points = [self._to_device(p) for p in item["points"]]
        if self.dynamic:  # no `features`: the slot tensor does not exist in this mode
            coordinates, occupancy, mean, point_voxel, flat = self.generate_batch_voxels_dynamic(points)
            item.update(points=self.pad_for_batch(points), coordinates=coordinates, occupancy=occupancy, voxel_mean=mean,
                        point_voxel=point_voxel, batch_size=len(points))
            if self.pillar_dynamic:
                item["flat_points"] = flat
            return item
        features, coordinates, occupancy, mean = self.generate_batch_voxels(points)
        item.update(points=self.pad_for_batch(points), features=features, coordinates=coordinates,
                    occupancy=occupancy, voxel_mean=mean, batch_size=len(points))
        return item


class TrainPreprocessor(Preprocessor):

    def collate_mapping(self, key, val):
        if key in ("G_cls", "G_reg", "M_cls", "M_reg", "G_dir"):
            return torch.stack(val)
        return val

    def collate(self, items):
        batch = defaultdict(list)
        for it in items:
            for key, val in it.items():
                batch[key].append(val)
        return self({k: self.collate_mapping(k, v) for k, v in batch.items()})

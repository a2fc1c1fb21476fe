"""Detection metrics on the device: KITTI 2-D bbox / BEV / 3-D average precision and AOS (kitti.py states the protocol;
kernels in csrc/kitti_eval.hip).  `python -m vision3d_amd.evaluation --labels DIR --results DIR [--metrics ...]` evaluates a
directory of result files."""
from .kitti import KittiEvaluator, camera_box_overlaps, lidar_to_camera, write_kitti_results

__all__ = ["KittiEvaluator", "camera_box_overlaps", "lidar_to_camera", "write_kitti_results"]

"""Detection metrics on the device: KITTI BEV / 3-D average precision (kitti.py states the protocol; kernels in
csrc/kitti_eval.hip).  `python -m vision3d_amd.evaluation --labels DIR --results DIR` evaluates a directory of result files."""
from .kitti import KittiEvaluator, camera_box_overlaps, lidar_to_camera, write_kitti_results

__all__ = ["KittiEvaluator", "camera_box_overlaps", "lidar_to_camera", "write_kitti_results"]

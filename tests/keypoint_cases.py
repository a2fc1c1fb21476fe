"""The named inputs of the keypoint-sampling tests (host and GPU) and their expected results by the numpy restatement, computed once.

A case is (points (B, N, 4) f32, K, S, proposals (B, P, 7) f32 or None, radius).  Every case comes out of synth.make_keypoint_case,
so every finite point keeps the azimuth margin for the case's S (tests/test_host_keypoint_sampling.py checks that)."""
import functools

import numpy as np

import keypoint_sampling_ref as ref
from vision3d_amd import synth

K = 64


def _general(s):
    points, proposals = synth.make_keypoint_case(s, batch=2, n_points=1500, n_sectors=s, n_proposals=5)
    return points, K, s, proposals, 1.6


def _short(seed):
    """1 460 points 20 m and more away + 40 within 4 m of the sensor, one proposal around the sensor: 40 candidates for K = 64."""
    rng = np.random.default_rng(seed)
    far, _ = synth.make_keypoint_case(seed, batch=1, n_points=1460, n_sectors=6, n_proposals=0, r_range=(20.0, 60.0))
    close, _ = synth.make_keypoint_case(seed + 50, batch=1, n_points=40, n_sectors=6, n_proposals=0, r_range=(3.0, 4.0))
    frame = np.concatenate([far[0], close[0]])
    rng.shuffle(frame)
    return frame


@functools.lru_cache(maxsize=None)
def all_cases():
    c = {f"general_s{s}": _general(s) for s in (1, 6, 7, 64)}
    plain = lambda seed, counts, s: synth.make_keypoint_case(seed, batch=1, n_points=sum(counts), n_sectors=s, n_proposals=0, counts=counts)[0]
    c["empty_sector"] = (plain(10, [300, 0, 300, 300, 300, 300], 6), K, 6, None, 1.6)
    c["one_point_sector"] = (plain(11, [1, 299, 300, 300, 300, 300], 6), K, 6, None, 1.6)
    c["equal_remainders"] = (plain(12, [500, 500, 500], 3), K, 3, None, 1.6)
    points, proposals = synth.make_keypoint_case(13, batch=1, n_points=1000, n_sectors=6, n_proposals=5)
    again = np.random.default_rng(13).integers(0, 1000, 500)  # a short frame padded by resampling its own points (pad_for_batch)
    c["duplicates"] = (np.concatenate([points, points[:, again]], 1), K, 6, proposals, 1.6)
    points, proposals = synth.make_keypoint_case(14, batch=2, n_points=1500, n_sectors=6, n_proposals=5)
    points = points.copy()
    points[0, [0, 7, 700], 0] = [np.nan, np.inf, -np.inf]
    points[0, [64, 1499], 1] = [np.inf, np.nan]
    points[1, [3, 511, 512], 2] = [np.nan, np.inf, np.nan]
    c["nonfinite"] = (points, K, 6, proposals, 1.6)
    box = np.tile(np.array([0, 0, -0.5, 2, 2, 2, 0], np.float32), (2, 1, 1))
    c["short"] = (np.stack([_short(15), _short(16)]), K, 6, box, 4.5)
    points, proposals = synth.make_keypoint_case(17, batch=2, n_points=1500, n_sectors=6, n_proposals=5)
    far = proposals.copy()
    far[:, :, :2] += 1000.0
    c["far_proposals"] = (points, K, 6, far, 1.6)
    c["no_proposals"] = (points, K, 6, proposals[:, :0], 1.6)
    c["single_point"] = (synth.make_keypoint_case(18, batch=1, n_points=1, n_sectors=6, n_proposals=0)[0], 1, 6, None, 1.6)
    c["nothing_finite"] = (np.full((1, 50, 4), np.nan, np.float32), 8, 6, None, 1.6)
    points, proposals = synth.make_keypoint_case(19, batch=3, n_points=1500, n_sectors=6, n_proposals=5)
    c["three_frames"] = (points, K, 6, proposals, 1.6)
    c["over_capacity"] = (synth.make_keypoint_case(20, batch=1, n_points=70000, n_sectors=1, n_proposals=0)[0], 32, 1, None, 1.6)
    # every body of the chain kernel: 16 register slots per thread (8 193 - 16 384 points in a sector), 24 (- 24 576, the register
    # capacity: one sector exactly at it, its neighbour one point above, on the streamed chain), a large and a small sector side by side
    c["slots_16"] = (plain(21, [16384], 1), 32, 1, None, 1.6)
    c["slots_24"] = (plain(22, [20000, 20000], 2), 32, 2, None, 1.6)
    c["at_capacity"] = (plain(23, [24576, 24577], 2), 32, 2, None, 1.6)
    c["mixed_sizes"] = (plain(24, [26000, 3000, 9000, 2], 4), 48, 4, None, 1.6)
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (idx (B, K) int32, counts (B, S) int32) of case `name` by the restatement."""
    points, k, s, proposals, radius = all_cases()[name]
    return ref.sector_point_sample(points, k, s, proposals, radius)


@functools.lru_cache(maxsize=None)
def random_quota_cases():
    """Small frames with random (S, K, n_k) -- empty sectors, K above, below and exactly at the number of candidates -- for the
    quota rule on the device: [(points (1, N, 4), K, S)]."""
    rng = np.random.default_rng(77)
    out = []
    for i in range(8):
        s = int(rng.integers(2, 65))
        counts = (rng.integers(1, 40, s) * (rng.random(s) < 0.7)).tolist()
        counts[0] = max(counts[0], 1)
        n = sum(counts)
        k = n if i < 2 else int(rng.integers(1, 2 * n))
        out.append((synth.make_keypoint_case(100 + i, batch=1, n_points=n, n_sectors=s, n_proposals=0, counts=counts)[0], k, s))
    return out

"""numpy restatement of the sectorized proposal-centric keypoint sampling (the definition in the module docstring of
vision3d_amd/pointnet2/pointnet2_utils.py), step by step in fp32 with one plain loop per step.  Imports nothing from the package.

Per frame: points (N, C >= 3) f32, K, S, proposals (P, 7) or None, radius ->
    idx (K,) int32, n_k (S,) candidates per sector, q_k (S,) quotas, used_filter (bool).
`sector_margin(points, S)` is the distance of every point's azimuth * S / 2 pi from an integer, in float64: the condition under
which the device's atan2f and numpy's agree on every sector (synth.make_keypoint_case keeps it above 1e-3)."""
import numpy as np

from fps_ref import fps_f32

F = np.float32


def candidates(points, proposals, radius):
    """-> (mask (N,) of the candidate set, used_filter)."""
    xyz = np.asarray(points, F)[:, :3]
    finite = np.isfinite(xyz).all(1)
    near = np.zeros(len(xyz), bool)
    if proposals is not None:
        for box in np.asarray(proposals, F).reshape(-1, 7):
            R = F(0.5) * np.fmax(np.fmax(box[3], box[4]), box[5]) + F(radius)
            with np.errstate(invalid="ignore", over="ignore"):
                dx, dy, dz = xyz[:, 0] - box[0], xyz[:, 1] - box[1], xyz[:, 2] - box[2]
                near |= ((dx * dx + dy * dy) + dz * dz) < R * R
    near &= finite
    if near.any():
        return near, True
    return finite, False


def sectors(points, S):
    """Sector of every point (fp32 arithmetic in the written order); meaningful for finite points."""
    xyz = np.asarray(points, F)[:, :3]
    with np.errstate(invalid="ignore"):
        t = (np.arctan2(xyz[:, 1], xyz[:, 0]).astype(F) + F(3.14159274)) * (F(S) * F(0.159154937))
    t = np.where(np.isfinite(t), t, 0)
    return np.minimum(S - 1, np.maximum(0, t.astype(np.int64))).astype(np.int64)


def sector_margin(points, S):
    xyz = np.asarray(points, np.float64)[:, :3]
    ok = np.isfinite(xyz).all(1)
    t = (np.arctan2(xyz[ok, 1], xyz[ok, 0]) + np.pi) * (S / (2 * np.pi))
    return np.abs(t - np.round(t))


def quotas(n_k, K):
    n_k = [int(v) for v in n_k]
    n = sum(n_k)
    if n < K:
        return list(n_k)
    q = [(K * v) // n for v in n_k]
    rem = [(K * v) % n for v in n_k]
    order = sorted(range(len(n_k)), key=lambda k: (-rem[k], k))
    for k in order[:K - sum(q)]:
        q[k] += 1
    return q


def fps_chain(xyz, picks):
    """xyz (n, 3) f32 in original-index order -> `picks` rows: first = row 0, then the largest running distance, lowest row on ties."""
    return [int(r) for r in fps_f32(np.asarray(xyz, F), picks)]  # stated once, in tests/fps_ref.py


def sector_point_sample_frame(points, K, S, proposals=None, radius=1.6):
    points = np.asarray(points, F)
    mask, used = candidates(points, proposals, radius)
    sec = sectors(points, S)
    n_k = [int((mask & (sec == k)).sum()) for k in range(S)]
    q_k = quotas(n_k, K)
    picked = []
    for k in range(S):
        if q_k[k] == 0:
            continue
        rows = np.flatnonzero(mask & (sec == k))  # increasing original index
        picked += [int(rows[r]) for r in fps_chain(points[rows, :3], q_k[k])]
    filled = len(picked)
    idx = np.zeros(K, np.int32)
    for i in range(K):
        idx[i] = picked[i % filled] if filled else 0
    return idx, np.asarray(n_k, np.int32), np.asarray(q_k, np.int32), used


def sector_point_sample(points, K, S, proposals=None, radius=1.6):
    """points (B, N, C), proposals (B, P, 7) or None -> idx (B, K) int32, counts (B, S) int32."""
    out = [sector_point_sample_frame(points[b], K, S, None if proposals is None else proposals[b], radius) for b in range(len(points))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

"""Farthest-point sampling (csrc/pointops.hip v3d_furthest_point_sample) restated, and its two kernels modelled.  numpy only; imports
nothing from the package.

The operation: pick 0 is point 0; every point keeps a running distance that starts at 1e10 and is lowered to its squared distance
(dx*dx + dy*dy) + dz*dz from each new pick; the next pick is the point with the largest running distance, the lowest index among equals.

fps_f32            the operation in float32, one vectorised step per pick: what the kernels must return bit for bit.
check_farthest_f64 follows a GIVEN chain of picks in float64 and asserts that every pick is a farthest point up to float32 rounding.
slab_model         the slab-skipping algorithm of fps_slab_kernel in float32 numpy, with a knob that narrows the slab bounds: used on
                   the host only, to show that the cases of tests/fps_cases.py see a wrong bound.  Not a reference for the GPU tests.
plain_model        the arg-max hierarchy of fps_kernel (slots of a thread, lanes of a wave, waves), with a knob per level: likewise.
"""
import numpy as np

F = np.float32
START = 1e10  # the running distances start here (and so never exceed it: a point 1e6 away is "1e10 away")

SLAB_THREADS = 256  # sorted positions per slab
SLAB_BINS = 1024


def _fps_one(xyz, k):
    out = np.zeros(k, np.int32)
    x, y, z = (np.ascontiguousarray(xyz[:, a]) for a in range(3))
    td = np.full(len(xyz), F(START), F)
    for s in range(1, k):
        with np.errstate(over="ignore", under="ignore"):
            dx, dy, dz = x - x[out[s - 1]], y - y[out[s - 1]], z - z[out[s - 1]]
            np.minimum(td, (dx * dx + dy * dy) + dz * dz, out=td)
        out[s] = np.argmax(td)  # the first maximum
    return out


def fps_f32(xyz, k):
    """xyz (N, 3) or (B, N, 3) float32 -> picks (k,) or (B, k) int32."""
    xyz = np.asarray(xyz)
    assert xyz.dtype == F and xyz.shape[-1] == 3 and 1 <= k <= xyz.shape[-2]
    if xyz.ndim == 2:
        return _fps_one(xyz, k)
    return np.stack([_fps_one(frame, k) for frame in xyz]) if len(xyz) else np.zeros((0, k), np.int32)


# Why 1e-6: the inputs are exact float32 numbers, and a float32 squared distance (dx*dx + dy*dy) + dz*dz carries five roundings on its
# way (subtraction, doubled by the square; the square; two sums of non-negative terms), each relative to its own result: a relative
# error of at most 5 * 2^-24 = 3e-7.  The minimum of correctly rounded numbers is a correctly rounded minimum.  The kernel's pick holds
# the largest FLOAT32 running distance, so in exact arithmetic it holds at least (1 - 3e-7) / (1 + 3e-7) > 1 - 1e-6 of the true maximum.
# (Where a square underflows the error is absolute, below 1e-37; the cases keep the distances they compare far above that.)
FARTHEST_RTOL = 1e-6


def check_farthest_f64(xyz, idx, rtol=FARTHEST_RTOL):
    """xyz (N, 3), idx (K,): follow the chain idx in float64 (the running distances start at 1e10 as the operation says) and assert at
    every step that the point picked holds at least (1 - rtol) of the largest running distance.  Nothing is excluded: the chain followed
    is the given one, so a pick that differs from some other implementation's never makes the rest incomparable."""
    p = np.asarray(xyz, np.float64)
    idx = np.asarray(idx).astype(np.int64)
    assert idx.ndim == 1 and p.ndim == 2
    assert idx[0] == 0, f"the first pick is {idx[0]}, not 0"
    assert idx.min() >= 0 and idx.max() < len(p), "a pick outside the cloud"
    x, y, z = (np.ascontiguousarray(p[:, a]) for a in range(3))
    td = np.full(len(p), START, np.float64)
    for s in range(1, len(idx)):
        dx, dy, dz = x - x[idx[s - 1]], y - y[idx[s - 1]], z - z[idx[s - 1]]
        np.minimum(td, dx * dx + dy * dy + dz * dz, out=td)
        top = td.max()
        assert td[idx[s]] >= (1.0 - rtol) * top, f"pick {s} = point {idx[s]} is {td[idx[s]]!r} away, point {int(td.argmax())} is {top!r} away"


def slab_bins(xyz):
    """The kernel's x range and bins: -> (bin of every point (N,) int64, mn, width), all float32 arithmetic in the kernel's order."""
    x = np.asarray(xyz, F)[:, 0]
    mn, mx = x.min(), x.max()
    span = np.maximum(mx - mn, F(1e-20))
    inv, width = F(SLAB_BINS) / span, span / F(SLAB_BINS)
    with np.errstate(under="ignore"):
        b = ((x - mn) * inv).astype(np.int64)  # truncation, like the kernel's (int)
    return np.clip(b, 0, SLAB_BINS - 1), mn, width


def slab_layout(xyz):
    """-> (order (N,): original index at every sorted position -- the STABLE sort by bin; the kernel's order inside a bin differs from
    run to run --, slab of every sorted position, first and last bin of every slab)."""
    b, _, _ = slab_bins(xyz)
    order = np.argsort(b, kind="stable")
    n = len(order)
    slabs = (n + SLAB_THREADS - 1) // SLAB_THREADS
    first = b[order[np.arange(slabs) * SLAB_THREADS]]
    last = b[order[np.minimum(n, (np.arange(slabs) + 1) * SLAB_THREADS) - 1]]
    return order, np.arange(n) // SLAB_THREADS, first, last


def slab_model(xyz, k, narrow=0, shift=0):
    """The slab algorithm as fps_slab_kernel states it: x range and bins, stable sort by bin, one slab per 256 sorted positions with the
    bounds  mn + (first bin - 2 + narrow) * width  and  mn + (last bin + 3 - narrow) * width,  a slab touched at a step only if
    gap^2 < D* (gap = x distance from the last pick to the slab, D* = the running distance the last pick had), the pick = the lowest
    original index among the maxima.  narrow = 0, shift = 0 is the kernel; narrow > 0 pulls every bound inwards by that many bins;
    shift = 1 gives slab j the bounds of slab j + 1 (the last one those of an empty slab, which is never touched).
    -> (picks (k,) int32, mean fraction of the slabs touched per step)."""
    xyz = np.asarray(xyz, F)
    _, mn, width = slab_bins(xyz)
    order, slab_of_pos, first, last = slab_layout(xyz)
    slab = np.empty(len(xyz), np.int64)
    slab[order] = slab_of_pos  # slab of every ORIGINAL index
    xlo = mn + (first - 2 + narrow).astype(F) * width
    xhi = mn + (last + 3 - narrow).astype(F) * width
    if shift:
        xlo, xhi = np.append(xlo[shift:], [F(3.4e38)] * shift), np.append(xhi[shift:], [F(-3.4e38)] * shift)
    out = np.zeros(k, np.int32)
    td = np.full(len(xyz), F(START), F)
    dstar = F(START)
    touched = []
    for s in range(1, k):
        c = xyz[out[s - 1]]
        with np.errstate(over="ignore", under="ignore"):
            gap = np.maximum(np.maximum(xlo - c[0], c[0] - xhi), F(0))
            touch = gap * gap < dstar
            d = xyz - c
            d = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        td = np.where(touch[slab], np.minimum(td, d), td)
        dstar = td.max()
        out[s] = np.argmax(td)  # first maximum in original-index order = lowest original index
        touched.append(touch.mean())
    return out, float(np.mean(touched)) if touched else 0.0


PLAIN_THREADS = 1024
NO_INDEX = 0x7FFFFFFF


def plain_model(xyz, k, strict=True, filtered=True, empty=-1.0):
    """The arg-max of fps_kernel as the kernel states it, level by level: point n in register slot n // 1024 of thread n % 1024; a thread
    walks its slots in order and takes a slot whose running distance is > its best so far (from -1; a slot without a point holds
    `empty` = -1); a wave takes the largest of its 64 threads' bests and the lowest index among the threads that hold it; the workgroup
    the same over its 16 waves.  The knobs are the three ways in which that can go wrong by one token: strict=False takes >= in the
    thread, filtered=False takes the wave's lowest index over ALL its threads, empty=0.0 lets a slot without a point hold 0.
    -> picks (k,) int64; a pick may then lie outside the cloud, and the chain ends there (the rest is NO_INDEX).  Host only, to show
    which cases see which mistake; not a reference for the GPU tests."""
    xyz = np.asarray(xyz, F)
    n = len(xyz)
    slots = max(2, 2 * ((-(-n // PLAIN_THREADS) + 1) // 2))  # the kernel holds its slots in pairs
    index = np.arange(slots * PLAIN_THREADS).reshape(slots, PLAIN_THREADS)  # slot j of thread t holds point t + 1024 j
    real = index < n
    td = np.where(real, F(START), F(empty)).astype(F)
    out = np.full(k, NO_INDEX, np.int64)
    out[0] = 0
    for s in range(1, k):
        c = xyz[out[s - 1]]
        with np.errstate(over="ignore", under="ignore"):
            d = xyz - c
            d = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        flat = td.reshape(-1)
        flat[:n] = np.minimum(flat[:n], d)  # (a slot without a point keeps `empty`: min(d, -1) = -1, min(d, 0) = 0)
        bd = np.full(PLAIN_THREADS, F(-1))
        bn = np.full(PLAIN_THREADS, NO_INDEX, np.int64)
        for j in range(slots):
            better = td[j] > bd if strict else td[j] >= bd
            bd = np.where(better, td[j], bd)
            bn = np.where(better, index[j], bn)
        bd, bn = bd.reshape(16, 64), bn.reshape(16, 64)
        wd = bd.max(1)
        wn = np.where(bd == wd[:, None], bn, NO_INDEX).min(1) if filtered else bn.min(1)
        out[s] = np.where(wd == wd.max(), wn, NO_INDEX).min()
        if out[s] >= n:
            break
    return out

"""Committed cases of the rotated 3-D IoU loss tests (tests/test_host_iou_loss.py on the CPU, tests/test_gpu_iou_loss.py on the GPU):
named pairs that sit on the edges of the definition, and a seeded random generator of overlapping pairs.  Boxes are
(x, y, z, w, l, h, yaw), yaw in radians."""
import math

import numpy as np

BASE = [0.3, -0.2, 0.1, 2.0, 4.0, 1.5, 0.4]


def _with(**kw):
    box = list(BASE)
    for k, v in kw.items():
        box["xyzwlht".index(k)] = v
    return box


# (pairs meant to be smooth differ in z and h and avoid yaw 0: equal z faces are a kink of the overlap height, tied extents and
# |sin 0| kinks of the DIoU cuboid)
# name -> (a, b, kink): kink = the term is not differentiable there (only value and finiteness are checked)
NAMED = {
    "identical": (BASE, BASE, True),
    "a_inside_b": (_with(w=1.0, l=2.0, h=1.0), _with(t=0.9), False),
    "b_inside_a": (_with(t=0.9), _with(w=1.0, l=2.0, h=1.0, x=0.4), False),
    "cross": (_with(w=1.0, l=5.0, t=0.2), _with(w=1.2, l=5.5, z=0.4, t=0.2 + math.pi / 2 + 0.3), False),  # 8-vertex polygon
    "octagon": (_with(w=3.0, l=3.0, t=0.02), _with(w=3.0, l=3.0, h=1.2, z=0.3, t=math.pi / 4, x=0.35, y=-0.15), False),  # 8 vertices, all four clips cut
    "triangle": (_with(w=2.0, l=2.0, t=0.03, x=0.0, y=0.0), _with(w=2.0, l=2.0, h=1.1, t=math.pi / 4 + 0.1, x=1.9, y=1.7), False),
    "equal_yaw_offset": (BASE, _with(x=0.9, y=0.5, z=0.3), True),  # parallel edges
    "yaw_plus_pi": (_with(x=0.9, y=0.5, z=0.3, h=1.2, t=0.4 + 0.3), _with(t=0.4 + math.pi), False),
    "yaw_zero_twin": (_with(x=0.9, y=0.5, z=0.3, h=1.2, t=0.4 + 0.3), _with(t=0.4), False),  # the same IoU as yaw_plus_pi
    "bev_disjoint": (BASE, _with(x=9.0, y=0.5, z=0.3, t=0.7), False),
    "z_disjoint": (BASE, _with(z=4.0, t=0.7), False),
    "z_contained": (_with(h=3.0), _with(h=1.0, z=0.4, t=0.7), False),
    "touching_edges": (_with(x=0.0, y=0.0, t=0.0, w=2.0), _with(x=2.0, y=0.0, t=0.0, w=2.0), True),
    "touching_z": (_with(z=0.0, h=1.0), _with(z=1.0, h=1.0, t=0.6), True),
}


def named_pairs():
    """-> names, a (n, 7) float32, b (n, 7) float32, kink (n,) bool."""
    names = list(NAMED)
    a = np.array([NAMED[k][0] for k in names], np.float32)
    b = np.array([NAMED[k][1] for k in names], np.float32)
    return names, a, b, np.array([NAMED[k][2] for k in names], bool)


def bad_pairs():
    """Rows under the bad-row rule: a zero size, a negative size, and a NaN and an Inf in every column, in either box.
    -> a (n, 7), b (n, 7) float32."""
    rows_a, rows_b = [], []
    other = _with(x=0.6, t=0.7)
    for col in (3, 4, 5):
        for value in (0.0, -1.0):
            for first in (True, False):
                box = list(BASE)
                box[col] = value
                rows_a.append(box if first else other)
                rows_b.append(other if first else box)
    for col in range(7):
        for value in (math.nan, math.inf, -math.inf):
            for first in (True, False):
                box = list(BASE)
                box[col] = value
                rows_a.append(box if first else other)
                rows_b.append(other if first else box)
    return np.array(rows_a, np.float32), np.array(rows_b, np.float32)


def random_pairs(n, seed=0):
    """a: centre U(-1, 1)^3, w U(1, 3), l U(2, 5), h U(1, 2), yaw U(-pi, pi); b = a + N(0, (.5, .5, .3, .3, .4, .2, .3)) with its
    sizes replaced by |size| + 0.2.  -> a (n, 7), b (n, 7) float32."""
    rng = np.random.default_rng(seed)
    a = np.concatenate([rng.uniform(-1, 1, (n, 3)), rng.uniform(1, 3, (n, 1)), rng.uniform(2, 5, (n, 1)), rng.uniform(1, 2, (n, 1)),
                        rng.uniform(-math.pi, math.pi, (n, 1))], 1)
    b = a + rng.normal(0, 1, (n, 7)) * np.array([0.5, 0.5, 0.3, 0.3, 0.4, 0.2, 0.3])
    b[:, 3:6] = np.abs(b[:, 3:6]) + 0.2
    return a.astype(np.float32), b.astype(np.float32)


MARGIN = 1e-3        # gradient comparisons use the random pairs whose decisions are at least this far from flipping ...
MAX_LEFT_OUT = 0.10  # ... which may leave out at most this share of them
N_RANDOM = 400

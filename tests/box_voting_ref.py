"""IoU-weighted box voting (cfg.BOX_VOTING) restated in plain numpy, float64.  The IoU matrix is an INPUT: the
restatement judges the vote, not the clipper -- whoever calls it passes the matrix of the implementation under test (the host shim's
own, or ops.box_iou_rotated's), so that both make the same membership decisions and no test needs a margin around the threshold.

    member_j = s_j > 0 and b_j finite (all seven) and u_kj >= float32(iou)          (a NaN compares false)
    w_j = s_j u_kj,  W = sum w_j
    out[c] = b_k[c] + sum w_j (b_j[c] - b_k[c]) / W   (c < 6),   out[6] = yaw_k + sum w_j wrap(yaw_j - yaw_k) / W
    wrap(d) = d - PI32 rint(d / PI32)  (numpy's rint rounds half to even),  W not finite or not > 0: out = b_k"""
import numpy as np

PI32 = float(np.float32(np.pi))  # the pi of the wrap is the fp32 constant in every statement: d = +-PI32 / 2 is then a tie in all of them


def wrap(d):
    return d - PI32 * np.rint(d / PI32)


def vote(boxes, scores, iou, iou_threshold):
    """boxes (G, T, 7), scores (G, T), iou (G, T, T) with iou[g, k, j] = IoU(centre k, candidate j) -> (voted (G, T, 7) float64,
    voters (G, T) = the number of members of every centre).  A row that is not voted is the input row (NaN and all)."""
    b, s, u = (np.asarray(a, np.float64) for a in (boxes, scores, iou))
    thr = float(np.float32(iou_threshold))
    G, T = s.shape
    out, voters = b.copy(), np.zeros((G, T), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        candidate = (s > 0) & np.isfinite(b).all(-1)
        for g in range(G):
            for k in range(T):
                m = candidate[g] & (u[g, k] >= thr)
                voters[g, k] = int(m.sum())
                w = s[g, m] * u[g, k, m]
                W = w.sum()
                if not (np.isfinite(W) and W > 0):
                    continue
                off = b[g, m] - b[g, k]
                off[:, 6] = wrap(off[:, 6])
                out[g, k] = b[g, k] + (w[:, None] * off).sum(0) / W
    return out, voters


def scaled_error(got, ref):
    """max |got - ref| / max(1, |ref|) over the entries where the reference is finite; where it is not, `got` must be non-finite too"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert not np.isfinite(got[~fin]).any(), "a non-finite reference entry came out finite"
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max())

"""Rotated 3-D IoU / DIoU loss of aligned box pairs (no upstream counterpart; the definition is this repository's, restated in
float64 by another algorithm in tests/iou_loss_ref.py).

Boxes are (x, y, z, w, l, h, yaw), z = centre, yaw in RADIANS read geometrically: w lies along (cos yaw, sin yaw), l along
(-sin yaw, cos yaw) -- the geometry of points-in-boxes, NOT the reading of `box_iou_rotated_3d`, which stays as it is.

    IoU  = A_bev * max(min(zhi) - max(zlo), 0) / (vol_a + vol_b - inter)       (0 where the union is not positive)
    term = 1 - IoU ("iou")  |  1 - IoU + rho2 / c2 ("diou": squared centre distance over the squared diagonal of the smallest
           world-aligned cuboid around both boxes; no penalty where c2 == 0)
    a pair with a non-finite number or a size <= 0 has IoU 0, term 1 and zero gradient

`iou3d_loss` / `box_iou3d_aligned` run in libvision3d_hip.so (csrc/iou_loss.hip: one launch, one lane per pair, the gradient
written with the forward); `iou3d_loss_torch` states the same arithmetic op by op in torch for any device and dtype."""
import torch

from .. import _lib as L

KINDS = {"iou": 0, "diou": 1}


def _kind(kind):
    try:
        return KINDS[kind]
    except KeyError:
        raise ValueError(f"iou3d_loss: kind must be one of {sorted(KINDS)}, got {kind!r}") from None


def _pairs(name, pred, target):
    L.require_gpu(name, pred, target)
    a, b = L.as_f32(name, pred.detach()), L.as_f32(name, target.detach())
    if a.dim() != 2 or a.shape[-1] != 7 or a.shape != b.shape or a.device != b.device:
        raise RuntimeError(f"{name}: expected two (N, 7) tensors on one device")
    return a, b


def _launch(a, b, kind, want_grad):
    n, dev = a.shape[0], a.device
    term = torch.empty(n, dtype=torch.float32, device=dev)
    iou = torch.empty(n, dtype=torch.float32, device=dev)
    grad = torch.empty((2, n, 7), dtype=torch.float32, device=dev) if want_grad else None  # [d_pred | d_target]
    with L.device_guard(dev):
        L.check(L.lib().v3d_iou3d_loss_fwd_bwd(L.ptr(a), L.ptr(b), n, kind, L.ptr(term), L.ptr(iou), L.ptr(grad),
                                               L.ptr(grad[1]) if want_grad else 0, L.stream_ptr()), "iou3d_loss_fwd_bwd")
    return term, iou, grad


class IoU3dLossFunction(torch.autograd.Function):
    """(pred (N, 7), target (N, 7)) -> term (N,) in one native pass that also writes d term / d pred and d term / d target; they stay
    on the node and backward multiplies them, in place and once, with the upstream gradient (the protocol of detector/fused_loss.py)."""

    @staticmethod
    def forward(ctx, pred, target, kind):
        a, b = _pairs("iou3d_loss", pred, target)
        term, _, grad = _launch(a, b, kind, True)
        ctx.grad = grad
        return term

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_term):
        from ..detector.fused_loss import take_gradient
        grad = take_gradient(ctx, "iou3d")
        grad.mul_(g_term.to(torch.float32).reshape(1, -1, 1))
        return (grad[0] if ctx.needs_input_grad[0] else None), (grad[1] if ctx.needs_input_grad[1] else None), None


def iou3d_loss(pred, target, kind="iou"):
    """(N, 7), (N, 7) float32 GPU tensors -> (N,) loss terms, differentiable in both arguments."""
    return IoU3dLossFunction.apply(pred, target, _kind(kind))


def box_iou3d_aligned(a, b):
    """(N, 7), (N, 7) float32 GPU tensors -> (N,) rotated 3-D IoU of the aligned pairs (true geometry, yaw in radians); no gradient."""
    a, b = _pairs("box_iou3d_aligned", a, b)
    return _launch(a, b, 0, False)[1]


# ---- the torch statement ---------------------------------------------------------------------------------------------------------
def _clip(px, py, cnt, lab, nx, ny, cx, cy, h, own):
    """il_clip of csrc/iou_loss_device.h over (N, 8) polygons: keep the part with n . (p - c) <= h; label `own` on the new edge."""
    slot = torch.arange(8, device=px.device)[None]
    valid = slot < cnt[:, None]
    nxt = torch.where(slot + 1 < cnt[:, None], slot + 1, torch.zeros_like(slot))
    d = (nx[:, None] * (px - cx[:, None]) + ny[:, None] * (py - cy[:, None])) - h[:, None]
    qx, qy, dn, = px.gather(1, nxt), py.gather(1, nxt), d.gather(1, nxt)
    # the vertices outside are held to ONE run (il_one_run): the runs that hold the vertex farthest outside, or a NaN distance
    out = valid & ~(d <= 0)
    nan = out & torch.isnan(d)
    ranked = torch.where(out & ~nan, d, torch.full_like(d, -float("inf")))
    seed = nan | ((slot == ranked.argmax(1, keepdim=True)) & (ranked.max(1, keepdim=True).values > -float("inf")))
    prv = torch.where(slot >= 1, slot - 1, (cnt[:, None] - 1).clamp(min=0))
    reach = seed & out
    for _ in range(7):
        reach = reach | (out & (reach.gather(1, nxt) | reach.gather(1, prv)))
    ic = ~reach
    inn = ic.gather(1, nxt)
    e1, e2 = valid & ic, valid & (ic != inn)
    t = d / (d - dn)
    ix, iy = px + t * (qx - px), py + t * (qy - py)
    lab2 = torch.where(ic, torch.full_like(lab, own), lab)
    k1, k2 = e1.long(), e2.long()
    before = torch.cumsum(k1 + k2, 1) - (k1 + k2)
    dump = torch.full_like(before, 8)
    pos1 = torch.where(e1 & (before < 8), before, dump)
    pos2 = torch.where(e2 & (before + k1 < 8), before + k1, dump)
    ox, oy, ol = px.new_zeros(px.shape[0], 9), px.new_zeros(px.shape[0], 9), lab.new_zeros(px.shape[0], 9)
    for pos, sx, sy, sl in ((pos1, px, py, lab), (pos2, ix, iy, lab2)):
        ox.scatter_(1, pos, sx)
        oy.scatter_(1, pos, sy)
        ol.scatter_(1, pos, sl)
    return ox[:, :8], oy[:, :8], (k1 + k2).sum(1).clamp(max=8), ol[:, :8]


def _pair_torch(a, b, kind):
    """iou3d_loss_pair of csrc/iou_loss_device.h, expression by expression: -> term (N,), iou (N,), d_a (N, 7), d_b (N, 7)."""
    zero, one = a.new_zeros(()), a.new_ones(())
    f = lambda m: torch.where(m, one, zero)
    ok = torch.isfinite(a).all(-1) & torch.isfinite(b).all(-1) & (a[:, 3:6] > 0).all(-1) & (b[:, 3:6] > 0).all(-1)
    ca, sa, cb, sb = torch.cos(a[:, 6]), torch.sin(a[:, 6]), torch.cos(b[:, 6]), torch.sin(b[:, 6])
    dx, dy, dz = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], b[:, 2] - a[:, 2]
    hwa, hla, hwb, hlb = a[:, 3] * 0.5, a[:, 4] * 0.5, b[:, 3] * 0.5, b[:, 4] * 0.5
    wx, wy, lx, ly = hwa * ca, hwa * sa, -(hla * sa), hla * ca
    pad = [torch.zeros_like(wx)] * 4
    px = torch.stack([-wx - lx, wx - lx, wx + lx, lx - wx] + pad, 1)
    py = torch.stack([-wy - ly, wy - ly, wy + ly, ly - wy] + pad, 1)
    lab = torch.tensor([0, 1, 2, 3, 0, 0, 0, 0], device=a.device).repeat(a.shape[0], 1)
    cnt = torch.full((a.shape[0],), 4, dtype=torch.long, device=a.device)
    for own, (nx, ny, h) in enumerate(((sb, -cb, hlb), (cb, sb, hwb), (-sb, cb, hlb), (-cb, -sb, hwb))):
        px, py, cnt, lab = _clip(px, py, cnt, lab, nx, ny, dx, dy, h, 4 + own)

    slot = torch.arange(8, device=a.device)[None]
    live = (slot < cnt[:, None]) & (cnt[:, None] >= 3)
    nxt = torch.where(slot + 1 < cnt[:, None], slot + 1, torch.zeros_like(slot))
    qx, qy = px.gather(1, nxt), py.gather(1, nxt)
    cross = px * qy - qx * py
    ex, ey = qx - px, qy - py
    length = torch.sqrt(ex * ex + ey * ey)
    of_b, odd = lab >= 4, (lab & 1) != 0
    pos = ((lab & 3) == 1) | ((lab & 3) == 2)
    ux, uy = torch.where(of_b, cb[:, None], ca[:, None]), torch.where(of_b, sb[:, None], sa[:, None])
    nx, ny = torch.where(odd, ux, -uy), torch.where(odd, uy, ux)
    nx, ny = torch.where(pos, nx, -nx), torch.where(pos, ny, -ny)
    mx = 0.5 * (px + qx) - torch.where(of_b, dx[:, None], zero)
    my = 0.5 * (py + qy) - torch.where(of_b, dy[:, None], zero)
    gx, gy, gh, gt = length * nx, length * ny, 0.5 * length, length * (mx * ny - my * nx)
    masks = (~of_b, ~of_b, ~of_b & odd, ~of_b & ~odd, ~of_b, of_b, of_b, of_b & odd, of_b & ~odd, of_b)
    parts = (gx, gy, gh, gh, gt) * 2
    acc = [torch.zeros_like(dx) for _ in range(11)]  # twice the area, then dA / d(x, y, w, l, yaw) of a and of b
    for i in range(8):  # in the kernel's order
        acc[0] = acc[0] + torch.where(live[:, i], cross[:, i], zero)
        for k in range(10):
            acc[1 + k] = acc[1 + k] + torch.where(live[:, i] & masks[k][:, i], parts[k][:, i], zero)
    half = 0.5 * acc[0]
    area = torch.where(half > 0, half, zero)
    gax, gay, gaw, gal, gat, gbx, gby, gbw, gbl, gbt = acc[1:]

    hza, hzb = a[:, 5] * 0.5, b[:, 5] * 0.5
    top, bot = torch.minimum(hza, dz + hzb), torch.maximum(-hza, dz - hzb)
    diff = top - bot
    oh = torch.where(diff > 0, diff, zero)
    alive, top_a, bot_a = oh > 0, hza < dz + hzb, -hza > dz - hzb
    ta, tb, ba, bb = f(alive & top_a), f(alive & ~top_a), f(alive & bot_a), f(alive & ~bot_a)
    inter = area * oh
    va, vb = a[:, 3] * a[:, 4] * a[:, 5], b[:, 3] * b[:, 4] * b[:, 5]
    uni = va + vb - inter
    has = uni > 0
    iou = torch.where(has, inter / uni, zero)
    val = torch.where(has, 1.0 - iou, one)
    z0 = torch.zeros_like(dx)
    di_a = torch.stack((oh * gax, oh * gay, area * (ta - ba), oh * gaw, oh * gal, area * (0.5 * (ta + ba)), oh * gat), 1)
    di_b = torch.stack((oh * gbx, oh * gby, area * (tb - bb), oh * gbw, oh * gbl, area * (0.5 * (tb + bb)), oh * gbt), 1)
    dv_a = torch.stack((z0, z0, z0, a[:, 4] * a[:, 5], a[:, 3] * a[:, 5], a[:, 3] * a[:, 4], z0), 1)
    dv_b = torch.stack((z0, z0, z0, b[:, 4] * b[:, 5], b[:, 3] * b[:, 5], b[:, 3] * b[:, 4], z0), 1)
    ui, u2 = (uni + inter)[:, None], (uni * uni)[:, None]
    t_da = torch.where(has[:, None], -((ui * di_a - inter[:, None] * dv_a) / u2), zero)
    t_db = torch.where(has[:, None], -((ui * di_b - inter[:, None] * dv_b) / u2), zero)

    if kind == KINDS["diou"]:
        aca, asa, acb, asb = ca.abs(), sa.abs(), cb.abs(), sb.abs()
        hxa, hya = (aca * a[:, 3] + asa * a[:, 4]) * 0.5, (asa * a[:, 3] + aca * a[:, 4]) * 0.5
        hxb, hyb = (acb * b[:, 3] + asb * b[:, 4]) * 0.5, (asb * b[:, 3] + acb * b[:, 4]) * 0.5
        rho2 = dx * dx + dy * dy + dz * dz
        xhi, xlo, yhi, ylo = hxa >= dx + hxb, -hxa <= dx - hxb, hya >= dy + hyb, -hya <= dy - hyb
        zhi, zlo = hza >= dz + hzb, -hza <= dz - hzb
        ex = torch.maximum(hxa, dx + hxb) - torch.minimum(-hxa, dx - hxb)
        ey = torch.maximum(hya, dy + hyb) - torch.minimum(-hya, dy - hyb)
        ez = torch.maximum(hza, dz + hzb) - torch.minimum(-hza, dz - hzb)
        c2 = ex * ex + ey * ey + ez * ez
        wide = c2 > 0
        pen = rho2 / c2
        val = torch.where(wide, val + pen, val)
        cxa, cxb, cya, cyb = f(xhi) - f(xlo), f(~xhi) - f(~xlo), f(yhi) - f(ylo), f(~yhi) - f(~ylo)
        cza, czb = f(zhi) - f(zlo), f(~zhi) - f(~zlo)
        sxa, sxb, sya, syb = f(xhi) + f(xlo), f(~xhi) + f(~xlo), f(yhi) + f(ylo), f(~yhi) + f(~ylo)
        sza, szb = f(zhi) + f(zlo), f(~zhi) + f(~zlo)
        dca, dsa = torch.where(ca >= 0, -sa, sa), torch.where(sa >= 0, ca, -ca)
        dcb, dsb = torch.where(cb >= 0, -sb, sb), torch.where(sb >= 0, cb, -cb)
        hxa_t, hya_t = (dca * a[:, 3] + dsa * a[:, 4]) * 0.5, (dsa * a[:, 3] + dca * a[:, 4]) * 0.5
        hxb_t, hyb_t = (dcb * b[:, 3] + dsb * b[:, 4]) * 0.5, (dsb * b[:, 3] + dcb * b[:, 4]) * 0.5
        hc_a = torch.stack((ex * cxa, ey * cya, ez * cza, ex * (sxa * (0.5 * aca)) + ey * (sya * (0.5 * asa)),
                            ex * (sxa * (0.5 * asa)) + ey * (sya * (0.5 * aca)), ez * (sza * 0.5),
                            ex * (sxa * hxa_t) + ey * (sya * hya_t)), 1)
        hc_b = torch.stack((ex * cxb, ey * cyb, ez * czb, ex * (sxb * (0.5 * acb)) + ey * (syb * (0.5 * asb)),
                            ex * (sxb * (0.5 * asb)) + ey * (syb * (0.5 * acb)), ez * (szb * 0.5),
                            ex * (sxb * hxb_t) + ey * (syb * hyb_t)), 1)
        hr_b = torch.stack((dx, dy, dz, z0, z0, z0, z0), 1)
        t_da = torch.where(wide[:, None], t_da + (2.0 * (-hr_b - pen[:, None] * hc_a)) / c2[:, None], t_da)
        t_db = torch.where(wide[:, None], t_db + (2.0 * (hr_b - pen[:, None] * hc_b)) / c2[:, None], t_db)

    ok = ok & torch.isfinite(val) & torch.isfinite(iou) & torch.isfinite(t_da).all(-1) & torch.isfinite(t_db).all(-1)
    return (torch.where(ok, val, one), torch.where(ok, iou, zero), torch.where(ok[:, None], t_da, zero),
            torch.where(ok[:, None], t_db, zero))


def iou3d_loss_torch(pred, target, kind="iou"):
    """`iou3d_loss` op by op in torch (any device / dtype): the fallback and the cross-check of the native pass.  The value and
    the gradient are the expressions of csrc/iou_loss_device.h (clipped polygon, shoelace sum, boundary integral), evaluated without
    a graph; autograd sees the term as linear in both boxes around their values, which is its exact first derivative."""
    kind = _kind(kind)
    if pred.dim() != 2 or pred.shape[-1] != 7 or pred.shape != target.shape:
        raise RuntimeError("iou3d_loss_torch: expected two (N, 7) tensors")
    target = target.to(pred.dtype)
    with torch.no_grad():
        term, _, d_a, d_b = _pair_torch(pred, target, kind)
    for box, grad in ((pred, d_a), (target, d_b)):
        if box.requires_grad:
            moved = torch.where(grad != 0, box - box.detach(), torch.zeros_like(box))  # exactly 0; rows without gradient stay out
            term = term + (moved * grad).sum(-1)
    return term


def box_iou3d_aligned_torch(a, b):
    """The IoU of `_pair_torch` alone (no gradient): the torch statement beside `box_iou3d_aligned`."""
    with torch.no_grad():
        return _pair_torch(a, b.to(a.dtype), 0)[1]

"""GPU: the rotated 3-D IoU loss (csrc/iou_loss.hip) -- the aligned operator and the fused stage-2 term of RefinementLoss -- against
the float64 restatement by another algorithm (tests/iou_loss_ref.py) and against the torch statement on the same device
(ops/iou_loss.py:iou3d_loss_torch, RefinementLoss.forward_torch), on the committed cases (tests/iou_loss_cases.py).

Bars against float64: four times the worst error of the fp32 HOST build of the same header against the restatement over the same
cases (tools/mb_iou_loss.py, profiles/iou_loss.txt: IoU 1.965e-7, term 2.000e-7, gradient 3.120e-6 of the pair's largest gradient);
the factor pays for device cosf / sinf / expf that differ from libm by a few ulp.
Bars against the torch statement on the device: those of tests/test_gpu_refine_loss.py for the stage-2 term (rtol 1e-6 on the loss,
rtol 1e-5 / atol 1e-7 on the gradient, which is divided by the row count there).  The aligned operator returns per-pair terms in
[0, 2] and per-pair gradients of order 1 under upstream gradients up to 2.5: the same rtol, with atol 1.2e-7 on the terms (one ulp
of the 1 that 1 - IoU is taken from) and atol 1e-6 on the gradients (two ulp at magnitude 4)."""
import numpy as np
import pytest
import torch

import iou_loss_cases as cases
import iou_loss_ref as ref
from vision3d_amd.core.config import _defaults, second_car_cfg

pytestmark = pytest.mark.gpu

MEASURED = dict(iou=1.965e-7, term=2.000e-7, grad=3.120e-6)  # fp32 host build against float64 (profiles/iou_loss.txt)
BAR = {k: 4 * v for k, v in MEASURED.items()}
KINDS = ("iou", "diou")
_CACHE = {}


def _pairs():
    """All pairs of the aligned tests, once: the first 257 committed random pairs, then the named ones.  -> a, b (float32 numpy),
    smooth (bool): the rows whose gradient is compared (random pairs clear of a decision flip, named pairs that are no kink)."""
    if "pairs" not in _CACHE:
        ra, rb = (x[:257] for x in cases.random_pairs(cases.N_RANDOM))  # of the pairs the bars were measured on
        keep = ref.margin(torch.tensor(ra), torch.tensor(rb)).numpy() > cases.MARGIN
        assert 1.0 - keep.mean() <= cases.MAX_LEFT_OUT
        _, na, nb, kink = cases.named_pairs()
        _CACHE["pairs"] = (np.concatenate((ra, na)), np.concatenate((rb, nb)), np.concatenate((keep, ~kink)))
    return _CACHE["pairs"]


def _upstream(n):
    return 0.5 + 2.0 * ((np.arange(n) * 37) % 101) / 101.0  # non-constant, in [0.5, 2.5)


def _reference(kind):
    """float64 term, iou and the gradients under `_upstream` for all of `_pairs`, once per kind."""
    if kind not in _CACHE:
        a, b, _ = _pairs()
        ta, tb = torch.tensor(a, dtype=torch.float64, requires_grad=True), torch.tensor(b, dtype=torch.float64, requires_grad=True)
        term, iou = ref.iou3d_terms(ta, tb, kind)
        da, db = torch.autograd.grad(term.sum(), (ta, tb))  # per pair: rows are independent, so upstream g scales row i by g[i]
        _CACHE[kind] = tuple(x.detach().numpy() for x in (term, iou, da, db))
    return _CACHE[kind]


def _grad_error(got_a, got_b, want_a, want_b):
    scale = np.maximum(np.abs(want_a).max(1), np.abs(want_b).max(1))
    err = np.maximum(np.abs(got_a - want_a).max(1), np.abs(got_b - want_b).max(1))
    return err / np.maximum(scale, 1e-30)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, "named"])
def test_aligned_operator_matches_restatement_and_torch_statement(kind, n):
    from vision3d_amd.ops import box_iou3d_aligned, iou3d_loss, iou3d_loss_torch
    a, b, smooth = _pairs()
    rows = slice(257, None) if n == "named" else slice(0, n)
    a, b, smooth = a[rows], b[rows], smooth[rows]
    w_term, w_iou, w_da, w_db = (x[rows] for x in _reference(kind))
    g = _upstream(len(a))
    up = torch.tensor(g, dtype=torch.float32, device="cuda")
    outs = []
    for fn in (iou3d_loss, iou3d_loss_torch):
        pa, pb = torch.tensor(a, device="cuda", requires_grad=True), torch.tensor(b, device="cuda", requires_grad=True)
        term = fn(pa, pb, kind)
        assert term.shape == (len(a),) and term.dtype == torch.float32
        (term * up).sum().backward()
        outs.append((term.detach().cpu().numpy(), pa.grad.cpu().numpy(), pb.grad.cpu().numpy()))
    (term, da, db), (s_term, s_da, s_db) = outs
    iou = box_iou3d_aligned(torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")).cpu().numpy()
    if len(a) == 0:
        assert da.shape == (0, 7) and db.shape == (0, 7) and iou.shape == (0,)
        return
    err = _grad_error(da[smooth], db[smooth], (w_da * g[:, None])[smooth], (w_db * g[:, None])[smooth]) if smooth.any() else np.zeros(1)
    print(f"{kind} n={n}: |IoU err| {np.abs(iou - w_iou).max():.3e} |term err| {np.abs(term - w_term).max():.3e} grad err {err.max():.3e}; "
          f"vs torch statement: term {np.abs(term - s_term).max():.3e} grad {max(np.abs(da - s_da).max(), np.abs(db - s_db).max()):.3e}")
    np.testing.assert_allclose(iou, w_iou, rtol=0, atol=BAR["iou"])
    np.testing.assert_allclose(term, w_term, rtol=0, atol=BAR["term"])
    assert np.isfinite(da).all() and np.isfinite(db).all()
    assert (err <= BAR["grad"]).all()
    np.testing.assert_allclose(term, s_term, rtol=1e-6, atol=1.2e-7)
    np.testing.assert_allclose(da, s_da, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(db, s_db, rtol=1e-5, atol=1e-6)
    if kind == "iou":
        np.testing.assert_array_equal(term, (1.0 - iou).astype(np.float32))


def test_aligned_operator_bad_rows_target_only_gradient_and_second_backward():
    from vision3d_amd.ops import box_iou3d_aligned, iou3d_loss
    a, b = (torch.tensor(x, device="cuda") for x in cases.bad_pairs())
    for kind in KINDS:
        pa, pb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        term = iou3d_loss(pa, pb, kind)
        term.sum().backward()
        assert bool((term == 1).all()) and bool((pa.grad == 0).all()) and bool((pb.grad == 0).all())
    assert bool((box_iou3d_aligned(a, b) == 0).all())
    ra, rb, _ = _pairs()
    pb = torch.tensor(rb[:65], device="cuda", requires_grad=True)  # d_target alone
    term = iou3d_loss(torch.tensor(ra[:65], device="cuda"), pb, "iou")
    term.sum().backward(retain_graph=True)
    np.testing.assert_allclose(pb.grad.cpu().numpy(), _reference("iou")[3][:65], rtol=0, atol=BAR["grad"] * np.abs(_reference("iou")[3][:65]).max())
    with pytest.raises(RuntimeError, match="backward called twice"):
        term.sum().backward()
    with pytest.raises(RuntimeError, match="GPU"):
        iou3d_loss(torch.zeros(2, 7), torch.zeros(2, 7))
    with pytest.raises(RuntimeError, match="GPU"):
        box_iou3d_aligned(torch.zeros(2, 7), torch.zeros(2, 7))
    with pytest.raises(ValueError, match="kind"):
        iou3d_loss(a, b, "giou")


# ---- the stage-2 term ----------------------------------------------------------------------------------------------------------
def _stage2(batch, n, seed=4, empty=False):
    """-> head (batch, n, 8) whose first 7 columns are R_reg, and the item's constants: proposals jittered around their matched
    ground truths (the random pairs), ~40 % of the rows in M_rreg, some of those with R_match = -1, one with an overflowing exp."""
    rows = batch * n
    a, b = cases.random_pairs(rows, seed=seed)
    rng = np.random.default_rng(seed)
    head = torch.tensor(rng.normal(0, 0.1, (batch, n, 8)).astype(np.float32))
    mask = rng.random(rows) < (0.0 if empty else 0.4)
    match = np.arange(rows)
    if empty:
        pass
    elif rows > 1:
        mask[:4] = True
        match[mask.nonzero()[0][1::7]] = -1  # masked rows without a ground truth
        head.view(rows, 8)[2, 3] = 200.0  # exp overflows: the bad-row rule
    else:
        mask[:] = True
    cut = rows // 2
    item = dict(proposals=torch.tensor(a).reshape(batch, n, 7).cuda(), boxes=[torch.tensor(b[:cut]).cuda(), torch.tensor(b[cut:]).cuda()],
                R_match=torch.tensor(match).reshape(batch, n).cuda(), M_rreg=torch.tensor(mask).reshape(batch, n).cuda())
    item["M_rcls"] = item["M_rreg"].clone()
    item["G_conf"] = torch.full((batch, n), 0.5, device="cuda")
    item["G_rreg"] = torch.zeros(batch, n, 7, device="cuda")
    return head.cuda(), item, torch.tensor(b)


def _loss(kind, enabled=True, weight=1.0):
    from vision3d_amd.detector import RefinementLoss
    cfg = _defaults()
    cfg.TRAIN.REFINEMENT_IOU_LOSS.merge_from_dict(dict(ENABLED=enabled, KIND=kind, WEIGHT=weight))
    return RefinementLoss(cfg)


def _run(loss, head, item, fused, contiguous=False):
    x = head.clone().requires_grad_(True)
    r_reg, r_cls = x.split([7, 1], dim=-1)
    full = dict(item, R_reg=r_reg.contiguous() if contiguous else r_reg, R_cls=r_cls)
    return x, (loss(full) if fused else loss.forward_torch(full))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(2, 70), (1, 1)])
def test_stage2_term_matches_torch_and_the_restatement(kind, shape):
    head, item, gt = _stage2(*shape)
    loss = _loss(kind)
    R64 = head[..., :7].detach().cpu().double().requires_grad_(True)
    want, count = ref.refine_iou_loss(R64, item["proposals"].cpu(), gt, item["R_match"].cpu(), item["M_rreg"].cpu(), kind)
    want_g, = torch.autograd.grad(3.0 * want, R64)
    want_g = want_g.reshape(-1, 7).numpy()
    assert count > 0 and (shape == (1, 1) or count < int(item["M_rreg"].sum()))
    y, stated = _run(loss, head, item, False)
    (3.0 * stated["refine_iou_loss"]).backward()
    for contiguous in (False, True):
        x, got = _run(loss, head, item, True, contiguous)
        assert got["refine_iou_loss"].shape == () and got["refine_iou_loss"].grad_fn.counts.tolist() == [count]
        (3.0 * got["refine_iou_loss"]).backward()
        assert float(x.grad[..., 7].abs().max()) == 0.0
        gg, sg = x.grad[..., :7].reshape(-1, 7).cpu().numpy(), y.grad[..., :7].reshape(-1, 7).cpu().numpy()
        scale = np.abs(want_g).max(1)
        err = (np.abs(gg - want_g).max(1) / np.maximum(scale, 1e-30))[scale > 0]
        t_got, t_stated = float(got["refine_iou_loss"].detach()), float(stated["refine_iou_loss"].detach())
        print(f"{kind} {shape} contiguous={contiguous}: term {t_got:.8f} torch {t_stated:.8f} float64 {float(want.detach()):.8f}; grad err vs float64 "
              f"{err.max():.3e}, vs torch {np.abs(gg - sg).max():.3e} (largest {np.abs(sg).max():.3e})")
        assert abs(t_got - float(want.detach())) <= BAR["term"]
        assert (err <= BAR["grad"]).all() and (gg[scale == 0] == 0).all()
        if shape != (1, 1):
            assert (gg[2] == 0).all()  # the row whose exp overflowed
        np.testing.assert_allclose(t_got, t_stated, rtol=1e-6)
        np.testing.assert_allclose(gg, sg, rtol=1e-5, atol=1e-7)


def test_stage2_term_is_bit_repeatable_and_empty_mask_gives_zero():
    head, item, _ = _stage2(2, 70)
    loss = _loss("diou")
    outs = []
    for _ in range(2):
        x, got = _run(loss, head, item, True)
        got["loss"].backward()
        outs.append((got["refine_iou_loss"].detach().clone(), got["loss"].detach().clone(), x.grad.clone()))
    for u, v in zip(*outs):
        assert torch.equal(u, v)
    head, item, _ = _stage2(2, 70, empty=True)
    x, got = _run(loss, head, item, True)
    got["refine_iou_loss"].backward()
    assert float(got["refine_iou_loss"].detach()) == 0.0 and got["refine_iou_loss"].grad_fn.counts.tolist() == [0]
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="backward called twice"):
        got["refine_iou_loss"].backward()


def test_refinement_loss_enabled_combines_three_parts_and_paths_agree():
    head, item, _ = _stage2(2, 70)
    loss = _loss("iou", weight=0.5)
    x, got = _run(loss, head, item, True)
    y, stated = _run(loss, head, item, False)
    assert sorted(got) == sorted(stated) == ["loss", "refine_cls_loss", "refine_iou_loss", "refine_reg_loss"]
    want = got["refine_cls_loss"] + loss.cfg.TRAIN.LAMBDA * got["refine_reg_loss"] + 0.5 * got["refine_iou_loss"]
    assert torch.equal(got["loss"].detach(), want.detach())
    for k in got:
        np.testing.assert_allclose(float(got[k].detach()), float(stated[k].detach()), rtol=1e-6, err_msg=k)
    got["loss"].backward()
    stated["loss"].backward()
    np.testing.assert_allclose(x.grad.cpu().numpy(), y.grad.cpu().numpy(), rtol=1e-5, atol=1e-7)
    with pytest.raises(RuntimeError, match="R_match"):
        loss({k: v for k, v in dict(item, R_reg=head[..., :7], R_cls=head[..., 7:]).items() if k != "R_match"})


def test_refinement_loss_disabled_is_unchanged():
    from vision3d_amd.detector import RefinementLoss
    head, item, _ = _stage2(2, 70)
    x, off = _run(_loss("iou", enabled=False), head, item, True)
    y, base = _run(RefinementLoss(_defaults()), head, item, True)
    assert sorted(off) == sorted(base) == ["loss", "refine_cls_loss", "refine_reg_loss"]
    off["loss"].backward()
    base["loss"].backward()
    for k in base:
        assert torch.equal(off[k].detach(), base[k].detach()), k
    assert torch.equal(x.grad, y.grad)


def test_pvrcnn_train_step_with_the_iou_term():
    import test_gpu_pvrcnn_train as T
    from vision3d_amd.detector import RefinementLoss
    cfg = second_car_cfg()
    cfg.TRAIN.REFINEMENT_IOU_LOSS.merge_from_dict(dict(ENABLED=True, KIND="diou"))
    item, rois, samples = T._batch(cfg)
    model = T._model(cfg, rois)
    torch.manual_seed(1)
    out = model.train_forward(dict(item), samples)
    losses = RefinementLoss(cfg)(out)
    assert sorted(losses) == ["loss", "refine_cls_loss", "refine_iou_loss", "refine_reg_loss"]
    assert all(bool(torch.isfinite(v.detach())) for v in losses.values())
    assert 0.0 <= float(losses["refine_iou_loss"].detach()) <= 2.0
    assert losses["refine_iou_loss"].grad_fn.counts.tolist() == [int(out["M_rreg"].sum())] and int(out["M_rreg"].sum()) > 0
    losses["refine_iou_loss"].backward()
    for name, p in model.named_parameters():
        if name.startswith("refinement_layer."):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.ne(0).any()), name

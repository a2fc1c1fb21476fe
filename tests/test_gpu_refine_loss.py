"""GPU: the fused refinement loss (csrc/refine_targets.hip) against the torch expressions of RefinementLoss.forward_torch on the same
device and against the float64 restatement (tests/refine_targets_ref.py): loss terms, counts, gradients under upstream gradients
(2.0, 3.0) as in tests/test_gpu_proposal_loss.py, repeatability, empty masks, and the consumed gradient buffers."""
import numpy as np
import pytest
import torch

import refine_targets_ref as R
from vision3d_amd.core.config import _defaults

pytestmark = pytest.mark.gpu


def _inputs(seed, b=4, n=300, empty=False, big=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    head = torch.randn(b, n, 8, device="cuda", generator=g) * (12.0 if big else 1.5)  # the head's output: R_reg | R_cls are views of it
    tg = dict(G_conf=(torch.rand(b, n, device="cuda", generator=g) * 1.4 - 0.2).clamp(0, 1),
              G_rreg=torch.randn(b, n, 7, device="cuda", generator=g) * 1.2,
              M_rcls=torch.rand(b, n, device="cuda", generator=g) > (2.0 if empty else 0.4))
    tg["M_rreg"] = tg["M_rcls"] & (torch.rand(b, n, device="cuda", generator=g) > 0.5)
    return head, tg


def _run(head, tg, fused, dtype=torch.float32):
    from vision3d_amd.detector import RefinementLoss
    x = head.clone().to(dtype).requires_grad_(True)
    r_reg, r_cls = x.split([7, 1], dim=-1)
    item = dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in tg.items()}, R_reg=r_reg, R_cls=r_cls)
    loss = RefinementLoss(_defaults())
    out = loss(item) if fused else loss.forward_torch(item)
    return x, out


@pytest.mark.parametrize("case", ["plain", "large_logits", "contiguous_inputs"])
def test_fused_loss_and_gradient_match_torch_and_the_restatement(case):
    head, tg = _inputs(3, big=case == "large_logits")
    x, got = _run(head, tg, True)
    if case == "contiguous_inputs":
        from vision3d_amd.detector import RefinementLoss
        x = head.clone().requires_grad_(True)
        got = RefinementLoss(_defaults())(dict(tg, R_reg=x[..., :7].contiguous(), R_cls=x[..., 7].contiguous()))  # R_cls as (B, n)
    assert got["loss"].shape == () and got["refine_cls_loss"].grad_fn is not None
    y, ref = _run(head, tg, False)
    want = R.loss(head[..., :7].cpu().numpy(), head[..., 7:].cpu().numpy(), **{k: v.cpu().numpy() for k, v in tg.items()})
    counts = got["refine_cls_loss"].grad_fn.counts.tolist()
    print(case, {k: (float(got[k].detach()), float(ref[k].detach()), want[k]) for k in ("refine_cls_loss", "refine_reg_loss", "loss")}, counts)
    assert counts == [want["n_cls"], want["n_reg"]] == [int(tg["M_rcls"].sum()), int(tg["M_rreg"].sum())]
    for k in ("refine_cls_loss", "refine_reg_loss"):
        np.testing.assert_allclose(float(got[k].detach()), float(ref[k].detach()), rtol=1e-6, err_msg=k)
        np.testing.assert_allclose(float(got[k].detach()), want[k], rtol=1e-5, err_msg=k)
    np.testing.assert_allclose(float(got["loss"].detach()), want["loss"], rtol=1e-5)
    (2.0 * got["refine_cls_loss"] + 3.0 * got["refine_reg_loss"]).backward()
    (2.0 * ref["refine_cls_loss"] + 3.0 * ref["refine_reg_loss"]).backward()
    np.testing.assert_allclose(x.grad.cpu().numpy(), y.grad.cpu().numpy(), rtol=1e-5, atol=1e-7)
    want_grad = np.concatenate([3.0 * want["dR_reg"], 2.0 * want["dR_cls"][..., None]], -1)
    np.testing.assert_allclose(x.grad.cpu().numpy(), want_grad, rtol=1e-5, atol=1e-7)


def test_fused_loss_is_bit_repeatable():
    head, tg = _inputs(11, b=8, n=300)
    outs = []
    for _ in range(2):
        x, l = _run(head, tg, True)
        l["loss"].backward()
        outs.append((l["loss"].detach().clone(), l["refine_cls_loss"].detach().clone(), l["refine_reg_loss"].detach().clone(), x.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_empty_masks_give_zero_loss_and_zero_gradients():
    head, tg = _inputs(5, empty=True)
    head[0, 0, :] = float("inf")  # an unselected row must not leak into the sums
    x, l = _run(head, tg, True)
    l["loss"].backward()
    assert float(l["loss"]) == 0.0 and float(l["refine_cls_loss"]) == 0.0 and float(l["refine_reg_loss"]) == 0.0
    assert l["refine_cls_loss"].grad_fn.counts.tolist() == [0, 0]
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) == 0.0


@pytest.mark.parametrize("n", [1, 65])
def test_upstream_gradients_scale_the_two_gradients_exactly(n):
    """Backward under upstream gradients (2, 3) is the stored gradient -- what a backward under (1, 1) returns -- times 2 on the
    confidence column and 3 on the box columns, one exact fp32 multiply per element.  One row; 65 rows as (1, 65): one more than a wave,
    the confidence gradients in front of the 7 * rows box gradients in one buffer."""
    head, tg = _inputs(13, b=1, n=n)
    if n == 1:
        tg["M_rcls"][:] = True
        tg["M_rreg"][:] = True
    grads = {}
    for up in ((1.0, 1.0), (2.0, 3.0)):
        x, l = _run(head, tg, True)
        (up[0] * l["refine_cls_loss"] + up[1] * l["refine_reg_loss"]).backward()
        grads[up] = x.grad
    want = grads[1.0, 1.0].clone()
    assert float(want[..., 7].abs().max()) > 0 and float(want[..., :7].abs().max()) > 0
    want[..., 7] *= 2.0
    want[..., :7] *= 3.0
    assert torch.equal(grads[2.0, 3.0], want)


def test_scale_entry_takes_gradient_buffers_that_are_not_adjacent():
    """v3d_refine_loss_scale with two separately allocated buffers (the autograd node hands it one: a single launch): each is scaled
    by its own upstream gradient, exactly, and nothing behind either is written."""
    from vision3d_amd import _lib as L
    rows = 65
    g = torch.Generator(device="cuda").manual_seed(17)
    reg_buf = torch.full((rows * 7 + 64,), 7.0, device="cuda")
    cls_buf = torch.full((rows + 64,), 7.0, device="cuda")
    d_reg, d_cls = reg_buf[:rows * 7], cls_buf[:rows]
    d_reg.copy_(torch.randn(rows * 7, device="cuda", generator=g))
    d_cls.copy_(torch.randn(rows, device="cuda", generator=g))
    assert d_reg.data_ptr() != d_cls.data_ptr() + 4 * rows
    want_reg, want_cls = 3.0 * d_reg, 2.0 * d_cls
    g_cls, g_reg = torch.tensor(2.0, device="cuda"), torch.tensor(3.0, device="cuda")
    with L.device_guard(d_reg.device):
        L.check(L.lib().v3d_refine_loss_scale(L.ptr(d_reg), L.ptr(d_cls), rows, L.ptr(g_cls), L.ptr(g_reg), L.stream_ptr()), "refine_loss_scale")
    assert torch.equal(d_reg, want_reg) and torch.equal(d_cls, want_cls)
    assert bool((reg_buf[rows * 7:] == 7.0).all()) and bool((cls_buf[rows:] == 7.0).all())


def test_backward_twice_raises():
    head, tg = _inputs(7, b=1, n=64)
    _, l = _run(head, tg, True)
    l["loss"].backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="backward called twice"):
        l["loss"].backward()

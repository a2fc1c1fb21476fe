"""The backward protocol of the fused losses (proposal, refinement, centre heatmap, keypoint segmentation), stated once.  Their
kernels write the gradient with the forward and leave it on the autograd node; backward takes it off the node -- once: the buffer
is scaled in place and handed to autograd -- and multiplies it with the upstream gradients of the loss terms in one launch."""
import torch


def take_gradient(ctx, name):
    """-> the gradient `forward` stored as `ctx.grad`, which leaves the node with this call."""
    grad, ctx.grad = ctx.grad, None
    if grad is None:
        raise RuntimeError(f"fused {name} loss: backward called twice (the gradient buffer is consumed by the first call)")
    return grad


def scale_gradient(entry, grad, args, upstream):
    """`v3d_<entry>(*args, *upstream, stream)` on the device of `grad`: tensors among `args` are passed as pointers, the upstream
    gradients (scalars of any float dtype) as contiguous fp32 device scalars."""
    from .. import _lib as L
    upstream = [g.to(torch.float32).contiguous() for g in upstream]
    with L.device_guard(grad.device):
        L.check(getattr(L.lib(), "v3d_" + entry)(*(L.ptr(a) if torch.is_tensor(a) else a for a in args),
                                                 *(L.ptr(g) for g in upstream), L.stream_ptr()), entry)

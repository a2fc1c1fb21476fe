"""CPU: the one statement of "did these tensors change" (vision3d_amd/stamp.py) and the cache built on it; the captured-graph
runner's rule -- compare with what THIS graph captured -- on stand-in plans (no device in it)."""
import types

import torch
from torch import nn

from vision3d_amd.stamp import cached, stamp_of


def test_stamp_moves_on_in_place_edits_load_state_dict_and_replacement():
    lin = nn.Linear(4, 3)
    tensors = lambda: (lin.weight, lin.bias)  # noqa: E731 (read through the module on every call, as the cache sites do)
    s0 = stamp_of(tensors())
    assert s0 == stamp_of(tensors()) and len(s0) == 2
    with torch.no_grad():
        lin.bias.add_(1.0)
    s1 = stamp_of(tensors())
    assert s1 != s0 and s1[0] == s0[0]  # only the bias moved
    lin.load_state_dict({k: v.clone() for k, v in lin.state_dict().items()})
    s2 = stamp_of(tensors())
    assert s2[0] != s1[0] and s2[1] != s1[1]
    lin.weight = nn.Parameter(lin.weight.detach().clone())  # a Parameter replaced on its module (.cuda(), assign=True)
    s3 = stamp_of(tensors())
    assert s3[0] != s2[0] and s3[1] == s2[1]
    lin.load_state_dict({k: v.clone() for k, v in lin.state_dict().items()}, assign=True)
    assert stamp_of(tensors()) != s3


def test_stamp_skips_none_takes_any_iterable_and_carries_extra():
    a, b = torch.zeros(3), torch.ones(2)
    assert stamp_of([a, None, b]) == stamp_of((a, b)) == stamp_of(t for t in (None, a, b, None))
    assert stamp_of([None]) == ()
    assert stamp_of([a], 1e-5, "fp32") == stamp_of([a]) + (1e-5, "fp32")
    assert stamp_of([a], "fp32") != stamp_of([a], "bf16x3")


def test_cache_builds_once_per_distinct_stamp_and_key():
    owner, calls = types.SimpleNamespace(), []
    w = torch.zeros(4)

    def build(tag):
        calls.append(tag)
        return [tag, float(w.sum())]  # a fresh object per build

    first = cached(owner, "_c", (w,), lambda: build("a"))
    assert cached(owner, "_c", (w,), lambda: build("a")) is first and calls == ["a"]
    other = cached(owner, "_c", (w,), lambda: build("b"), key=2)  # a second key: its own entry, nobody evicted
    assert cached(owner, "_c", (w,), lambda: build("a")) is first and cached(owner, "_c", (w,), lambda: build("b"), key=2) is other
    assert calls == ["a", "b"] and set(owner.__dict__["_c"]) == {None, 2}
    w.add_(1.0)
    second = cached(owner, "_c", (w,), lambda: build("a"))
    assert second == ["a", 4.0] and second is not first and calls == ["a", "b", "a"]
    assert cached(owner, "_c", (w,), lambda: build("b"), key=2) == ["b", 4.0] and calls == ["a", "b", "a", "b"]
    assert cached(owner, "_c", (w,), lambda: build("x"), extra=("fp32",)) == ["x", 4.0]  # `extra` is part of the stamp
    assert cached(owner, "_c", (w,), lambda: build("x"), extra=("fp32",)) == ["x", 4.0] and calls[4:] == ["x"]
    assert cached(owner, "_d", (w,), lambda: build("d")) == ["d", 4.0] and set(owner.__dict__) == {"_c", "_d"}


def test_cache_on_a_module_stays_out_of_its_attributes_and_state():
    lin = nn.Linear(2, 2)
    cached(lin, "_t", lin.parameters(), lambda: lin.weight.detach().t().contiguous())
    assert "_t" in lin.__dict__ and "_t" not in lin.state_dict() and "_t" not in dict(lin.named_buffers())


def test_module_caches_follow_their_tensors():
    """Two of the routed sites on CPU tensors: the RPN's folded BatchNorm and an MLP's packed weights (two keys)."""
    from vision3d_amd.detector.layers import MLP
    from vision3d_amd.detector.second import RPN
    rpn = RPN(C_in=16, C_up=16, C_down=16, blocks=2).eval()
    x = torch.randn(1, 16, 8, 8, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        folded = rpn._folded()
        assert rpn._folded() is folded
        before = rpn.fused_forward(x)
        bn = next(m for m in rpn.modules() if isinstance(m, nn.BatchNorm2d))
        bn.running_var.mul_(4.0)
        assert rpn._folded() is not folded
        assert not torch.equal(rpn.fused_forward(x), before)
        torch.testing.assert_close(rpn.fused_forward(x), rpn.up_block(rpn.down_block(x)), rtol=1e-4, atol=1e-5)
    mlp = MLP([8, 4, 2], bias=True)
    rows = torch.arange(7, -1, -1)
    plain, permuted = mlp._packed(), mlp._packed(rows)
    assert mlp._packed() is plain and mlp._packed(rows) is permuted and plain is not permuted
    assert torch.equal(permuted[0][0], plain[0][0][rows])
    with torch.no_grad():
        mlp.linear_0.weight.add_(1.0)
    assert mlp._packed() is not plain and mlp._packed(rows) is not permuted
    assert torch.equal(mlp._packed()[0][0][:, :4], mlp.linear_0.weight.t())


def test_geometry_buffers_reach_the_torch_statements():
    """The torch halves of the two geometry sites read the buffers on every call (the fused halves: tests/test_gpu_stamp.py)."""
    from vision3d_amd.core.config import second_car_cfg
    from vision3d_amd.detector import sparse_cnn
    from vision3d_amd.detector.layers import BEVFeatureGatherer
    cfg = second_car_cfg()
    cnn = sparse_cnn.CNN_FACTORY[cfg.CNN](cfg)
    ind = torch.tensor([[0, 1, 2, 3], [0, 4, 5, 6]], dtype=torch.int32)
    vol = types.SimpleNamespace(indices=ind, features=torch.randn(2, 4), batch_size=1)  # (what to_global reads of a level)
    xyz0 = cnn.to_global(2, vol)[0].clone()
    cnn.voxel_offset.add_(0.25)
    want = ind.flip(1)[:, :3].float() * (torch.tensor(cfg.VOXEL_SIZE) * 2) + (torch.tensor(cfg.GRID_BOUNDS[:3]) + 0.25)
    assert torch.equal(cnn.to_global(2, vol)[0][0], want) and torch.equal(cnn.to_global_torch(2, vol)[0][0], want)
    assert not torch.equal(want, xyz0[0])
    bev = BEVFeatureGatherer(cfg, torch.tensor(cfg.GRID_BOUNDS[:3]), torch.tensor(cfg.VOXEL_SIZE))
    xy = torch.tensor([[[[1.0, -39.0]]]])
    g0 = bev._to_grid(xy, 16, 16).clone()
    bev.pixel_offset.add_(0.2)
    assert not torch.equal(bev._to_grid(xy, 16, 16), g0)


class _Plan:
    """Stand-in for a shared plan: a stamp of its tensor, and `_stamp` = the stamp of its last upload."""

    def __init__(self):
        self.w, self._stamp = torch.zeros(2), None

    def _param_stamp(self):
        return stamp_of((self.w,))

    def sync_weights(self):
        self._stamp = self._param_stamp()


def test_graph_runner_compares_with_its_own_capture_not_the_shared_upload():
    """Two runners share their plans (a pipeline's slots share the dense head's; slot 0's backbone plan serves eager calls too).
    After a notified edit, an upload by anybody else must not hide the change from a runner that captured before it."""
    from vision3d_amd.detector.graph import GraphedSecond
    model, plan, dense = types.SimpleNamespace(_weights_epoch=0), _Plan(), _Plan()

    def runner():
        g = GraphedSecond.__new__(GraphedSecond)
        g.model, g.plan, g.dense = model, plan, dense
        plan.sync_weights(), dense.sync_weights()                   # (the warm-up of a capture uploads)
        g.captured = (plan._param_stamp(), dense._param_stamp())    # (what _capture records at its end)
        g._seen_epoch = model._weights_epoch
        return g

    a, b = runner(), runner()
    assert not a.weights_changed() and not b.weights_changed()
    dense.w.add_(1.0)
    assert not a.weights_changed()   # an un-notified edit: one integer comparison, the tensors are not looked at
    model._weights_epoch += 1
    dense.sync_weights()             # an eager call, or the first slot's new capture, uploads: the plan says "unchanged" ...
    assert a.weights_changed() and b.weights_changed()  # ... and both runners still know their graphs are stale
    assert not a.weights_changed()   # (the epoch is stored: the caller captures again on True)
    model._weights_epoch += 1
    a.captured = (plan._param_stamp(), dense._param_stamp())
    assert not a.weights_changed()   # the epoch moved and nothing this graph baked in did: no new capture

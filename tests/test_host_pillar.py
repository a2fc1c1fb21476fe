"""CPU: the pillar feature encoder without a GPU.  vision3d_amd/csrc/pillar_device.h -- the text the kernels compile -- built for the
host with g++ (tests/host/pillar_host_shim.cpp) and PillarFeatureNet.forward_torch, both against the float64 restatement
(tests/pillar_ref.py) on the committed cases (tests/pillar_cases.py); the GPU run of the same header is tests/test_gpu_pillar.py.

Bounds (the convention of tests/test_gpu_direction.py).  A value: max |error| over the tensor relative to max(1, largest |reference|),
at most max(2e-6, 4 x the same figure of the fp32 torch statement on the same inputs), measured on every run.  A gradient: max |error|
relative to the tensor's largest |reference| entry, at most max(1e-6, 4 x the figure of the fp32 restatement given the same winners).
The batch statistics of the header come from double moments: they are held to the value bound like everything else.  Moment
identities and the float64 runs of forward_torch are exact up to float64 rounding: 1e-10.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import pillar_cases as cases
import pillar_ref as ref
from pillar_checks import GRAD_BOUND, VALUE_BOUND, grad_error, item_of, module_for, value_error, winner_validity

HERE = os.path.dirname(os.path.abspath(__file__))
EXACT = 1e-10
LIVE = [n for n in cases.CASE_IDS if cases.CASES[n][0] > 0]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def host():
    so = os.path.join(HERE, "host", "_build", "libpillar_host.so")
    src = os.path.join(HERE, "host", "pillar_host_shim.cpp")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-std=c++17", "-o", so, src])
    lib = C.CDLL(so)
    lib.host_pillar_bn.argtypes = [C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 4
    lib.host_pillar_bn.restype = None
    lib.host_pillar_backward.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 2 + [C.c_int, C.c_void_p, C.c_float] + [C.c_void_p] * 7

    class Host:
        @staticmethod
        def _base(c):
            return (_p(c["features"]), _p(c["occupancy"]), _p(c["coordinates"]), c["M"], c["P"], c["C"])

        def encode(self, c, scale, shift):
            rows, winner = np.empty((c["M"], c["CH"]), np.float32), np.empty((c["M"], c["CH"]), np.int32)
            geom = np.asarray(c["geom"], np.float32)
            assert lib.host_pillar_encode(*self._base(c), _p(geom), _p(c["weight"]), c["CH"], _p(scale), _p(shift), _p(rows), _p(winner)) == 0
            return rows, winner

        def moments(self, c):
            K = c["K"]
            S, geom = np.empty(K + K * (K + 1) // 2, np.float64), np.asarray(c["geom"], np.float32)
            assert lib.host_pillar_moments(*self._base(c), _p(geom), _p(S)) == 0
            return S

        def bn(self, c, S):
            out = [np.empty(c["CH"], np.float64) for _ in range(4)]
            lib.host_pillar_bn(c["K"], _p(S), float(c["M"] * c["P"]), _p(c["weight"]), c["CH"], _p(c["gamma"]), _p(c["beta"]), c["eps"], *map(_p, out))
            return out  # mean, var, scale, shift

        def backward(self, c, rows, winner, S):
            dW, dg, db = np.empty((c["CH"], c["K"]), np.float64), np.empty(c["CH"], np.float64), np.empty(c["CH"], np.float64)
            geom = np.asarray(c["geom"], np.float32)
            assert lib.host_pillar_backward(*self._base(c), _p(geom), _p(c["weight"]), c["CH"], _p(c["gamma"]), c["eps"], _p(rows),
                                            _p(winner), _p(c["d_rows"]), _p(S), _p(dW), _p(dg), _p(db)) == 0
            return dW, dg, db
    return Host()


@pytest.mark.parametrize("name", cases.CASE_IDS)
def test_cases_are_well_formed(name):
    cases.check_well_formed(cases.build(name))


def test_cases_cover_the_edges():
    specs = cases.CASES.values()
    assert {1, 5, 37, 0}.issubset({s[0] for s in specs}) and any(s[0] > 4 * 256 and s[0] % 4 for s in specs)
    assert {1, 3, 8, 32}.issubset({s[1] for s in specs}) and {3, 4, 5}.issubset({s[2] for s in specs})
    assert {64, 128} == {s[3] for s in specs} and any(s[4] == 3 and s[5] == "empty_middle" for s in specs)


@pytest.mark.parametrize("name", LIVE)
def test_reference_is_well_posed(name):
    """On the reference alone: shifts of both signs; where pillars are short the padded candidate wins some positive maxima and loses
    others; the tie case ties exactly and the rule names the lower row."""
    c = cases.build(name)
    r = ref.encode(c, training=True)
    shift = (torch.as_tensor(c["beta"]).double() - r["mean"] * torch.as_tensor(c["gamma"]).double() / torch.sqrt(r["var"] + c["eps"])).numpy()
    assert (shift > 0).any() and (shift < 0).any()
    short = ~r["real"][:, -1].numpy()
    positive = (r["rows"].numpy() > 0) & short[:, None]
    if c["M"] >= 5 and short.any():
        share = float(((r["winner"] == -1) & positive).sum() / max(positive.sum(), 1))
        print("pillar-padded-share", dict(case=name, share=round(share, 3)))
        assert 0.02 < share < 0.98
    if c["variant"] == "tie":
        a = r["a"].numpy()
        assert (a[0, 1] == a[0, 2]).all() and not (r["winner"][0] == 2).any() and (r["winner"][0] == 1).any()


@pytest.mark.parametrize("name", LIVE)
def test_moment_identities(host, name):
    """The header's moments equal the direct sums, and mean / biased variance from them equal the per-row statistics (float64)."""
    c = cases.build(name)
    r = ref.encode(c, training=True)
    S = host.moments(c)
    want = ref.direct_moments(r["f"]).numpy()
    assert np.abs(S - want).max() <= 1e-6 * max(1.0, np.abs(want).max())  # (the header's rows are fp32 rows: 6e-8 each)
    mean, var, _, _ = host.bn(c, want)
    assert value_error(mean, r["mean"].numpy()) <= EXACT and value_error(var, r["var"].numpy()) <= EXACT


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name", LIVE)
def test_header_forward_against_float64(host, name, training):
    c = cases.build(name)
    r = ref.encode(c, training=training)
    net = module_for(c).train(training)
    with torch.no_grad():
        own = value_error(net.forward_torch(item_of(c)).numpy(), ref.canvas(r["rows"], c, cases.H, cases.W).numpy())
    bound = max(VALUE_BOUND, 4 * own)
    if training:
        mean, var, scale, shift = host.bn(c, host.moments(c))
        assert value_error(mean.astype(np.float32), r["mean"].numpy()) <= bound and value_error(var.astype(np.float32), r["var"].numpy()) <= bound
        scale, shift = scale.astype(np.float32), shift.astype(np.float32)
    else:
        scale, shift = (t.numpy() for t in net._folded())
    rows, winner = host.encode(c, scale, shift)
    err = value_error(rows, r["rows"].numpy())
    gap = winner_validity(r["a"], winner, r["real"], bound)
    print("pillar-host-forward-figures", dict(case=name, training=training, fp32_torch=own, header=err, winner_gap=gap))
    assert err <= bound
    if c["variant"] == "tie":
        either = np.isin(winner[0], (1, 2))
        assert either.any() and (winner[0][either] == 1).all()
        np.testing.assert_array_equal(winner[0][either], r["winner"][0][either])


@pytest.mark.parametrize("name", LIVE)
def test_header_backward_against_float64(host, name):
    c = cases.build(name)
    S = host.moments(c)
    _, _, scale, shift = host.bn(c, S)
    rows, winner = host.encode(c, scale.astype(np.float32), shift.astype(np.float32))
    got = host.backward(c, rows, winner, S)
    want = [g.numpy() for g in ref.gradients_given_winner(c, winner)]
    own = [g.numpy() for g in ref.gradients_given_winner(c, winner, torch.float32)]
    for what, g, w, o in zip(("dW", "d_gamma", "d_beta"), got, want, own):
        err, fp32 = grad_error(g, w), grad_error(o, w)
        print("pillar-host-backward-figures", dict(case=name, what=what, fp32_statement=fp32, header=err))
        assert err <= max(GRAD_BOUND, 4 * fp32)


@pytest.mark.parametrize("name", LIVE)
def test_forward_torch_against_float64(name):
    """forward_torch in float64 is the restatement to rounding, values and gradients (free-running maxima: in float64 both pick the
    same rows, exact ties have identical rows); on CPU tensors forward() is forward_torch."""
    c = cases.build(name)
    for training in (False, True):
        r = ref.encode(c, training=training)
        net = module_for(c, torch.float64).train(training)
        out = net.forward_torch(item_of(c))
        assert value_error(out.detach().numpy(), ref.canvas(r["rows"], c, cases.H, cases.W).numpy()) <= EXACT
        if training:
            assert value_error(net.norm.running_mean.numpy(), r["running_mean"].numpy()) <= EXACT
            assert value_error(net.norm.running_var.numpy(), r["running_var"].numpy()) <= EXACT
            d = ref.canvas(torch.from_numpy(c["d_rows"]).double(), c, cases.H, cases.W)
            (out * d).sum().backward()
            want = ref.gradients_given_winner(c, r["winner"])
            for g, w in zip((net.linear.weight.grad, net.norm.weight.grad, net.norm.bias.grad), want):
                assert grad_error(g.numpy(), w.numpy()) <= 1e-9
            # the maximum READ at given winners (padded candidates among them): the same rows, the same gradients
            given = module_for(c, torch.float64).train()
            again = given.forward_torch(item_of(c), winner=torch.from_numpy(r["winner"].astype(np.int32)))
            assert value_error(again.detach().numpy(), out.detach().numpy()) <= EXACT
            (again * d).sum().backward()
            for g, w in zip((given.linear.weight.grad, given.norm.weight.grad, given.norm.bias.grad), want):
                assert grad_error(g.numpy(), w.numpy()) <= 1e-9
    net, same = module_for(c).train(), module_for(c).train()
    item = item_of(c)
    out = net(item)  # CPU tensors: forward() IS the torch statement, bit for bit
    assert out.dtype == torch.float32 and out.shape == (c["B"], c["CH"], cases.H, cases.W)
    assert torch.equal(out, same.forward_torch(item_of(c))) and torch.equal(net.norm.running_var, same.norm.running_var)
    assert item["features"].grad is None and not item["features"].requires_grad


def test_empty_batch():
    c = cases.build("empty")
    for training in (False, True):
        net = module_for(c).train(training)
        before = net.norm.running_mean.clone()
        out = net.forward_torch(item_of(c))
        assert out.shape == (2, 128, cases.H, cases.W) and float(out.abs().max()) == 0.0
        assert torch.equal(net.norm.running_mean, before) and int(net.norm.num_batches_tracked) == 0


def test_config_helpers():
    from vision3d_amd.core import AnchorGenerator
    from vision3d_amd.core.config import cfg as default_cfg, pillar_car_cfg, second_car_cfg
    from vision3d_amd import detector
    from vision3d_amd.detector.pillar import PillarFeatureNet, pillar_config, pillar_enabled, pillar_geometry, refuse_pillar
    assert detector.PillarFeatureNet is PillarFeatureNet
    assert not pillar_enabled(default_cfg) and not pillar_enabled(second_car_cfg()) and default_cfg.PILLAR.CHANNELS == 128
    old = second_car_cfg()
    del old["PILLAR"]  # a config written before the key existed
    assert not pillar_enabled(old) and pillar_config(old) == dict(ENABLED=False, CHANNELS=128)
    refuse_pillar(old, "anything")
    cfg = pillar_car_cfg()
    assert pillar_enabled(cfg) and cfg.VOXEL_SIZE == [0.4, 0.4, 4.0] and cfg.STRIDES == [1] and cfg.MAX_OCCUPANCY == 32 and cfg.MAX_VOXELS == 12000
    assert tuple(AnchorGenerator(cfg).anchors.shape) == (1, 2, 200, 176, 7)
    geom, shape = pillar_geometry(cfg)
    assert shape == (200, 176) and geom[:3] == tuple(float(np.float32(v)) for v in (0.4, 0.4, 4.0))
    assert geom[3:] == (float(np.float32(0.4) / np.float32(2)), float(np.float32(0.4) / np.float32(2) + np.float32(-40)), float(np.float32(2) + np.float32(-3)))
    with pytest.raises(ValueError, match="PILLAR"):
        refuse_pillar(cfg, "this entry point")
    tall = pillar_car_cfg()
    tall.VOXEL_SIZE = [0.4, 0.4, 8.0]
    with pytest.raises(ValueError, match="z extent"):
        PillarFeatureNet(tall)
    for z in (2.0, 3.0, 3.9, 4.1, 5.0):  # half height; one cell after rounding but short of the extent (the top would be dropped); long
        off = pillar_car_cfg()
        off.VOXEL_SIZE = [0.4, 0.4, z]
        with pytest.raises(ValueError, match="z extent"):
            PillarFeatureNet(off)
    assert pillar_geometry(cases.tiny_cfg()) == (cases.geometry(), (cases.H, cases.W))

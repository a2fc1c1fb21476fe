"""CPU: the dynamic pillar encoder without a GPU.  vision3d_amd/csrc/pillar_device.h -- the text the kernels compile -- built for the
host with g++ (tests/host/pillar_dynamic_host_shim.cpp) and DynamicPillarFeatureNet.forward_torch, both against the float64 restatement
(tests/pillar_dynamic_ref.py) on the committed cases (tests/pillar_dynamic_cases.py); the GPU run of the same header is
tests/test_gpu_pillar_dynamic.py.

Bounds: the project's, from tests/pillar_checks.py.  A value: max |error| over the tensor relative to max(1, largest |reference|), at
most max(2e-6, 4 x the same figure of the fp32 torch statement on the same inputs), measured on every run.  A gradient: max |error|
relative to the tensor's largest |reference| entry, at most max(1e-6, 4 x the figure of the fp32 restatement given the same winners).
Moment identities and the float64 runs of forward_torch are exact up to float64 rounding: 1e-10.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import pillar_dynamic_cases as cases
import pillar_dynamic_ref as ref
from pillar_dynamic_checks import GRAD_BOUND, VALUE_BOUND, grad_error, item_of, module_for, tie_pair, value_error, winner_validity

HERE = os.path.dirname(os.path.abspath(__file__))
EXACT = 1e-10
LIVE = [n for n in cases.CASE_IDS if cases.CASES[n][0] > 0]
_BUILT = {}


def case_of(name):
    """Built once per run, shared and left unchanged."""
    if name not in _BUILT:
        _BUILT[name] = cases.build(name)
    return _BUILT[name]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def host():
    so = os.path.join(HERE, "host", "_build", "libpillar_dynamic_host.so")
    src = os.path.join(HERE, "host", "pillar_dynamic_host_shim.cpp")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-std=c++17", "-o", so, src])
    lib = C.CDLL(so)
    base = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.host_pillar_dynamic_encode.argtypes = base + [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int]
    lib.host_pillar_dynamic_moments.argtypes = base + [C.c_void_p]
    lib.host_pillar_dynamic_bn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 4
    lib.host_pillar_dynamic_bn.restype = None
    lib.host_pillar_dynamic_backward.argtypes = base + [C.c_void_p, C.c_int, C.c_void_p, C.c_float] + [C.c_void_p] * 7

    class Host:
        @staticmethod
        def _base(c):
            return (_p(c["points"]), _p(c["point_voxel"]), c["N"], _p(c["voxel_mean"]), _p(c["coordinates"]), c["M"], c["C"],
                    _p(np.asarray(c["geom"], np.float32)))

        def encode(self, c, scale, shift, reverse=0):
            rows, winner = np.empty((c["M"], c["CH"]), np.float32), np.empty((c["M"], c["CH"]), np.int32)
            geom = np.asarray(c["geom"], np.float32)
            args = self._base(c)[:-1] + (_p(geom),)
            assert lib.host_pillar_dynamic_encode(*args, _p(c["weight"]), c["CH"], _p(scale), _p(shift), _p(rows), _p(winner), reverse) == 0
            return rows, winner

        def moments(self, c):
            K = c["K"]
            S, geom = np.empty(K + K * (K + 1) // 2 + 1, np.float64), np.asarray(c["geom"], np.float32)
            assert lib.host_pillar_dynamic_moments(*self._base(c)[:-1], _p(geom), _p(S)) == 0
            return S

        def bn(self, c, S):
            out = [np.empty(c["CH"], np.float64) for _ in range(4)]
            lib.host_pillar_dynamic_bn(c["K"], _p(S), _p(c["weight"]), c["CH"], _p(c["gamma"]), _p(c["beta"]), c["eps"], *map(_p, out))
            return out  # mean, var, scale, shift

        def backward(self, c, rows, winner, S):
            dW, dg, db = np.empty((c["CH"], c["K"]), np.float64), np.empty(c["CH"], np.float64), np.empty(c["CH"], np.float64)
            geom = np.asarray(c["geom"], np.float32)
            assert lib.host_pillar_dynamic_backward(*self._base(c)[:-1], _p(geom), _p(c["weight"]), c["CH"], _p(c["gamma"]), c["eps"], _p(rows),
                                                    _p(winner), _p(c["d_rows"]), _p(S), _p(dW), _p(dg), _p(db)) == 0
            return dW, dg, db
    return Host()


@pytest.mark.parametrize("name", cases.CASE_IDS)
def test_cases_are_well_formed(name):
    cases.check_well_formed(case_of(name))


def test_cases_cover_the_edges():
    specs = cases.CASES
    assert {1, 5, 37, 9, 41, 0} <= {s[0] for s in specs.values()} and {3, 4, 5} <= {s[1] for s in specs.values()}
    assert {64, 128} == {s[2] for s in specs.values()} and specs["empty_middle"][3] == 3
    assert specs["second_pass"][0] > 4 * 256 and specs["second_pass"][0] % 4, "the backward's 256 workgroups of four pillars"
    assert specs["encode_pass"][0] > 4096 and specs["encode_pass"][0] > 2048, "the encode grid and the offsets scan's rounds"
    assert cases.MANY_POINTS > 256 * 256 and cases.MANY_POINTS % 256, "the moments' 256 workgroups of 256 points"
    assert case_of("many_points")["N"] > cases.MANY_POINTS and 700 in case_of("crowded")["occupancy"]


@pytest.mark.parametrize("name", LIVE)
def test_reference_is_well_posed(name):
    """On the reference alone: shifts of both signs; a share of zero rows strictly between 2 % and 98 % where M >= 5; the tie case ties
    exactly in at least one channel and the rule names the lower index; one kept point gives relu(beta)."""
    c = case_of(name)
    r = ref.encode(c, training=True)
    assert r["n_kept"] == int(c["occupancy"].sum())
    shift = (torch.as_tensor(c["beta"]).double() - r["mean"] * torch.as_tensor(c["gamma"]).double() / torch.sqrt(r["var"] + c["eps"])).numpy()
    assert (shift > 0).any() and (shift < 0).any()
    rows = r["rows"].numpy()
    if c["M"] >= 5:
        share = float((rows == 0).mean())
        print("pillar-dynamic-zero-share", dict(case=name, share=round(share, 3)))
        assert 0.02 < share < 0.98
    pos = rows > 0
    if pos.any():
        a = r["a"].numpy()
        second = np.full_like(rows, -np.inf)
        for m in np.flatnonzero(c["occupancy"] > 1):
            mine = a[r["pillar"] == m]
            top = np.sort(mine, axis=0)
            second[m] = top[-1] - top[-2]
        gaps = second[pos & np.isfinite(second) & (second > 0)]
        if gaps.size:
            print("pillar-dynamic-best-second-gap", dict(case=name, smallest=float(gaps.min())))
    if c["variant"] == "tie":
        lo, hi = tie_pair(c)
        a = r["a"].numpy()
        where = {int(i): k for k, i in enumerate(r["idx"])}
        assert (a[where[lo]] == a[where[hi]]).all()
        won = r["winner"][0] == lo
        print("pillar-dynamic-tie", dict(channels_won_by_the_pair=int(won.sum())))
        assert won.any() and not (r["winner"][0] == hi).any() and (rows[0][won] > 0).any()
    if name == "one_point":
        want = np.maximum(c["beta"].astype(np.float64), 0)
        assert np.abs(rows[0] - want).max() <= EXACT and float(r["var"].abs().max()) == 0.0
        print("pillar-dynamic-one-point", dict(positive=float((want > 0).mean())))


@pytest.mark.parametrize("name", LIVE)
def test_moment_identities(host, name):
    """The header's moments equal the direct sums (the last entry the kept count, exactly), and mean / biased variance from the direct
    moments equal the per-row statistics (float64)."""
    c = case_of(name)
    r = ref.encode(c, training=True)
    S = host.moments(c)
    want = ref.direct_moments(r["f"]).numpy()
    assert S[-1] == want[-1] == r["n_kept"]
    assert np.abs(S - want).max() <= 1e-6 * max(1.0, np.abs(want).max())  # (the header's rows are fp32 rows: 6e-8 each)
    mean, var, _, _ = host.bn(c, want)
    assert value_error(mean, r["mean"].numpy()) <= EXACT and value_error(var, r["var"].numpy()) <= EXACT


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name", LIVE)
def test_header_forward_against_float64(host, name, training):
    c = case_of(name)
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
    back_rows, back_winner = host.encode(c, scale, shift, reverse=1)
    assert np.array_equal(rows, back_rows) and np.array_equal(winner, back_winner), "the order of the points does not matter"
    err = value_error(rows, r["rows"].numpy())
    gap = winner_validity(c, r, winner, bound)
    print("pillar-dynamic-host-forward-figures", dict(case=name, training=training, fp32_torch=own, header=err, winner_gap=gap))
    assert err <= bound
    if c["variant"] == "tie":
        lo, hi = tie_pair(c)
        either = np.isin(winner[0], (lo, hi))
        assert either.any() and (winner[0][either] == lo).all()
        np.testing.assert_array_equal(winner[0][either], r["winner"][0][either])


@pytest.mark.parametrize("name", LIVE)
def test_header_backward_against_float64(host, name):
    c = case_of(name)
    S = host.moments(c)
    _, _, scale, shift = host.bn(c, S)
    rows, winner = host.encode(c, scale.astype(np.float32), shift.astype(np.float32))
    got = host.backward(c, rows, winner, S)
    want = [g.numpy() for g in ref.gradients_given_winner(c, winner)]
    own = [g.numpy() for g in ref.gradients_given_winner(c, winner, torch.float32)]
    for what, g, w, o in zip(("dW", "d_gamma", "d_beta"), got, want, own):
        err, fp32 = grad_error(g, w), grad_error(o, w)
        print("pillar-dynamic-host-backward-figures", dict(case=name, what=what, fp32_statement=fp32, header=err))
        assert err <= max(GRAD_BOUND, 4 * fp32)


@pytest.mark.parametrize("name", LIVE)
def test_forward_torch_against_float64(name):
    """forward_torch in float64 is the restatement to rounding, values and gradients; with the winners given it reads the same rows;
    on CPU tensors forward() is forward_torch."""
    c = case_of(name)
    for training in (False, True):
        r = ref.encode(c, training=training)
        net = module_for(c, torch.float64).train(training)
        out = net.forward_torch(item_of(c))
        assert value_error(out.detach().numpy(), ref.canvas(r["rows"], c, cases.H, cases.W).numpy()) <= EXACT
        if training:
            assert int(net.norm.num_batches_tracked) == 1
            assert value_error(net.norm.running_mean.numpy(), r["running_mean"].numpy()) <= EXACT
            assert value_error(net.norm.running_var.numpy(), r["running_var"].numpy()) <= EXACT
            d = ref.canvas(torch.from_numpy(c["d_rows"]).double(), c, cases.H, cases.W)
            want = ref.gradients_given_winner(c, r["winner"])
            given = module_for(c, torch.float64).train()
            again = given.forward_torch(item_of(c), winner=torch.from_numpy(r["winner"].astype(np.int32)))
            assert value_error(again.detach().numpy(), out.detach().numpy()) <= EXACT
            (again * d).sum().backward()
            for g, w in zip((given.linear.weight.grad, given.norm.weight.grad, given.norm.bias.grad), want):
                assert grad_error(g.numpy(), w.numpy()) <= 1e-9
            (out * d).sum().backward()  # free-running maxima: an exact tie splits its gradient between IDENTICAL rows, the same sums
            for g, w in zip((net.linear.weight.grad, net.norm.weight.grad, net.norm.bias.grad), want):
                assert grad_error(g.numpy(), w.numpy()) <= 1e-9
    net, same = module_for(c).train(), module_for(c).train()
    item = item_of(c)
    out = net(item)  # CPU tensors: forward() IS the torch statement, bit for bit
    assert out.dtype == torch.float32 and out.shape == (c["B"], c["CH"], cases.H, cases.W)
    assert torch.equal(out, same.forward_torch(item_of(c))) and torch.equal(net.norm.running_var, same.norm.running_var)
    assert item["flat_points"].grad is None and not item["flat_points"].requires_grad


def test_empty_batch_and_shape_checks():
    c = case_of("empty")
    for training in (False, True):
        net = module_for(c).train(training)
        before = net.norm.running_mean.clone()
        out = net.forward_torch(item_of(c))
        assert out.shape == (2, 128, cases.H, cases.W) and float(out.abs().max()) == 0.0
        assert torch.equal(net.norm.running_mean, before) and int(net.norm.num_batches_tracked) == 0
    c = case_of("five")
    net = module_for(c)
    for key, bad in (("point_voxel", torch.zeros(c["N"] + 1, dtype=torch.int32)), ("occupancy", torch.ones(c["M"] + 1, dtype=torch.int32)),
                     ("coordinates", torch.zeros((c["M"], 3), dtype=torch.int32)), ("flat_points", torch.zeros((c["N"], c["C"] + 1))),
                     ("voxel_mean", torch.zeros((c["M"], c["C"] + 1)))):
        item = item_of(c)
        item[key] = bad
        with pytest.raises(ValueError, match="DynamicPillarFeatureNet"):
            net(item)


def test_config_helpers():
    from vision3d_amd import detector
    from vision3d_amd.core import config
    from vision3d_amd.detector.pillar import DynamicPillarFeatureNet, PillarFeatureNet, pillar_enabled
    assert detector.DynamicPillarFeatureNet is DynamicPillarFeatureNet and issubclass(DynamicPillarFeatureNet, PillarFeatureNet)
    assert config.cfg.PILLAR.DYNAMIC is False and not config.pillar_dynamic_enabled(config.cfg)
    assert not config.pillar_dynamic_enabled(config.pillar_car_cfg())
    inert = config.second_car_cfg().merge_from_dict(dict(PILLAR=dict(DYNAMIC=True)))
    assert not pillar_enabled(inert) and not config.pillar_dynamic_enabled(inert), "inert unless PILLAR.ENABLED"
    old = config.pillar_car_cfg()
    del old["PILLAR"]["DYNAMIC"]  # a config written before the key existed
    assert pillar_enabled(old) and not config.pillar_dynamic_enabled(old)
    cfg = config.pillar_dynamic_car_cfg()
    assert config.pillar_dynamic_enabled(cfg) and pillar_enabled(cfg) and not config.dynamic_voxel_enabled(cfg)
    assert cfg.VOXEL_SIZE == [0.4, 0.4, 4.0] and cfg.PILLAR.CHANNELS == 128
    both = config.pillar_dynamic_car_cfg().merge_from_dict(dict(DYNAMIC_VOXELIZATION=dict(ENABLED=True)))
    with pytest.raises(ValueError, match="cfg.PILLAR.DYNAMIC"):
        config.refuse_dynamic_with_pillar(both)
    hard, dyn = PillarFeatureNet(config.pillar_car_cfg()), DynamicPillarFeatureNet(cfg)
    assert list(hard.state_dict()) == list(dyn.state_dict()) and dyn.map_shape == hard.map_shape
    dyn.load_state_dict(hard.state_dict())

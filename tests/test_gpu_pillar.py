"""GPU: the pillar feature encoder (csrc/pillar.hip through vision3d_amd/detector/pillar.py) against the float64 restatement
(tests/pillar_ref.py) on the cases of tests/pillar_cases.py, and the SECOND model built on it.  tests/test_host_pillar.py proves the
cases well-posed on the reference alone and states the bounds: a value within max(2e-6, 4 x the fp32 torch statement's error against
float64 on the same inputs) relative to max(1, largest |reference|); a gradient within max(1e-6, 4 x the fp32 restatement's error given
the same winners) of the tensor's largest entry -- both measured again on every run.  The margin is four because the kernel's
summation order (fmaf chain, folded scale / shift, double moments) differs from torch's while the operation count is the same.

The backward is compared GIVEN the kernel's winners: the gap between the best and the second-best candidate goes down to 1e-6 on
these cases, the size of the fp32 forward error, so a free-running float64 argmax may legitimately name another row; the winners
themselves are checked for validity on every (pillar, channel) of every case.

MEASURED_FP32_ERRORS -- largest error over the live cases on an MI355X (profiles/pillar_encoder.txt); the tests measure both columns
again on every run.  Every kernel figure lies below the project bounds 2e-6 / 1e-6; only for dW does the bound come from the
statement (four times 1.39e-6 on one case).

    quantity        fp32 torch statement   kernels
    rows (eval)     2.21e-7                2.17e-7
    rows (train)    3.04e-7                3.04e-7
    batch mean      --                     4.96e-8
    batch var       --                     1.64e-7
    running_mean    8.29e-8                8.29e-8
    running_var     6.70e-8                6.70e-8
    dW              1.39e-6                8.66e-7
    d_gamma         2.96e-7                2.72e-7
    d_beta          1.70e-7                5.75e-8
"""
import copy

import numpy as np
import pytest
import torch

import pillar_cases as cases
import pillar_ref as ref
from pillar_checks import GRAD_BOUND, VALUE_BOUND, grad_error, item_of, module_for, value_error, winner_validity

pytestmark = pytest.mark.gpu

LIVE = [n for n in cases.CASE_IDS if cases.CASES[n][0] > 0]


def _low_level(c):
    from vision3d_amd.detector import pillar as P
    it = item_of(c, "cuda")
    args = (it["features"], it["occupancy"], it["coordinates"], c["geom"])
    w, gamma, beta = (torch.from_numpy(c[k]).cuda() for k in ("weight", "gamma", "beta"))
    return P, args, w, gamma, beta


def _torch_statement(c, training):
    """-> (the fp32 torch statement's canvas on the GPU, its module after the call)."""
    net = module_for(c).cuda().train(training)
    with torch.no_grad():
        return net.forward_torch(item_of(c, "cuda")).cpu().numpy(), net


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name", LIVE)
def test_forward_against_float64(name, training):
    c = cases.build(name)
    r = ref.encode(c, training=training)
    want = ref.canvas(r["rows"], c, cases.H, cases.W).numpy()
    stated, stated_net = _torch_statement(c, training)
    own = value_error(stated, want)
    bound = max(VALUE_BOUND, 4 * own)
    net = module_for(c).cuda().train(training)
    item = item_of(c, "cuda")
    if training:
        out = net(item)
        assert out.requires_grad
    else:
        with torch.no_grad():
            out = net(item)
    got = out.detach().cpu().numpy()
    co = c["coordinates"].astype(np.int64)
    occupied = np.zeros((c["B"], cases.H, cases.W), bool)
    occupied[co[:, 0], co[:, 2], co[:, 3]] = True
    assert got.shape == want.shape and (got.transpose(0, 2, 3, 1)[~occupied] == 0).all(), "zero elsewhere"
    figures = dict(case=name, training=training, rows_fp32_torch=own, rows=value_error(got, want))
    assert figures["rows"] <= bound, figures
    if training:
        P, args, w, gamma, beta = _low_level(c)
        rows, winner, bn, moments = P.pillar_train_forward(*args, w, gamma, beta, c["eps"])
        again = P.pillar_train_forward(*args, w, gamma, beta, c["eps"])
        torch.cuda.synchronize()
        for a, b in zip((rows, winner, bn, moments), again):
            assert torch.equal(a, b), "two runs are bit-identical"
        ci = torch.from_numpy(co).cuda()
        assert torch.equal(rows, out.detach().permute(0, 2, 3, 1)[ci[:, 0], ci[:, 2], ci[:, 3]]) and torch.equal(winner, net.last_winner)
        figures.update(mean=value_error(bn[0].cpu().numpy(), r["mean"].numpy()), var=value_error(bn[1].cpu().numpy(), r["var"].numpy()))
        assert figures["mean"] <= bound and figures["var"] <= bound, figures
        assert value_error(moments.cpu().numpy(), ref.direct_moments(r["f"]).numpy()) <= 1e-6
        figures["winner_gap"] = winner_validity(r["a"], winner.cpu().numpy(), r["real"], bound)
        if c["variant"] == "tie":
            w0 = winner[0].cpu().numpy()
            either = np.isin(w0, (1, 2))
            assert either.any() and (w0[either] == 1).all(), "the lower of two tied rows wins"
            np.testing.assert_array_equal(w0[either], r["winner"][0][either])
        for what in ("running_mean", "running_var"):
            own_r = value_error(getattr(stated_net.norm, what).cpu().numpy(), r[what].numpy())
            figures[what + "_fp32_torch"], figures[what] = own_r, value_error(getattr(net.norm, what).cpu().numpy(), r[what].numpy())
            assert figures[what] <= max(VALUE_BOUND, 4 * own_r), figures
        assert int(net.norm.num_batches_tracked) == 1
    else:
        with torch.no_grad():
            assert torch.equal(net(item), out), "two runs are bit-identical"
    print("pillar-forward-figures", figures)


@pytest.mark.parametrize("name", LIVE)
def test_backward_against_float64_given_the_winners(name):
    c = cases.build(name)
    P, args, w, gamma, beta = _low_level(c)
    rows, winner, bn, moments = P.pillar_train_forward(*args, w, gamma, beta, c["eps"])
    d_rows = torch.from_numpy(c["d_rows"]).cuda()
    got = P.pillar_train_backward(*args, w, gamma, c["eps"], rows, winner, d_rows, moments)
    again = P.pillar_train_backward(*args, w, gamma, c["eps"], rows, winner, d_rows, moments)
    for a, b in zip(got, again):
        assert torch.equal(a, b), "two runs are bit-identical"
    given = winner.cpu().numpy()
    want = [g.numpy() for g in ref.gradients_given_winner(c, given)]
    own = [g.numpy() for g in ref.gradients_given_winner(c, given, torch.float32)]
    figures = dict(case=name)
    for what, g, t, o in zip(("dW", "d_gamma", "d_beta"), got, want, own):
        figures[what + "_fp32_statement"], figures[what] = grad_error(o, t), grad_error(g.cpu().numpy(), t)
    print("pillar-backward-figures", figures)
    for what in ("dW", "d_gamma", "d_beta"):
        assert figures[what] <= max(GRAD_BOUND, 4 * figures[what + "_fp32_statement"]), figures
    # ... and the module hands exactly these to autograd
    net = module_for(c).cuda().train()
    out = net(item_of(c, "cuda"))
    assert _has_node(out.grad_fn, "PillarEncodeFunctionBackward")
    (out * ref.canvas(torch.from_numpy(c["d_rows"]), c, cases.H, cases.W).cuda()).sum().backward()
    for p, g in zip((net.linear.weight, net.norm.weight, net.norm.bias), got):
        assert torch.equal(p.grad, g)


def _has_node(fn, name):
    seen, stack = set(), [fn]
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if type(f).__name__ == name:
            return True
        stack.extend(n for n, _ in f.next_functions)
    return False


def test_empty_batch_and_unsupported_shapes():
    from vision3d_amd import _lib as L
    c = cases.build("empty")
    for training in (False, True):
        net = module_for(c).cuda().train(training)
        out = net(item_of(c, "cuda"))
        assert out.shape == (2, 128, cases.H, cases.W) and float(out.abs().max()) == 0.0 and int(net.norm.num_batches_tracked) == 0
    lib, z = L.lib(), torch.zeros(4, device="cuda")
    geom = L.host_f32(cases.geometry())
    for P_, C_, CH_ in ((65, 4, 128), (0, 4, 128), (8, 2, 128), (8, 9, 128), (8, 4, 96)):
        assert lib.v3d_pillar_encode(L.ptr(z), L.ptr(z), L.ptr(z), 1, P_, C_, geom, L.ptr(z), CH_, L.ptr(z), L.ptr(z), L.ptr(z), 0) == -3
    # ... which the module answers with the torch statement: 96 channels
    d = dict(cases.build("five"), CH=96)
    rng = np.random.default_rng(5)
    for k, shape in (("weight", (96, d["K"])), ("gamma", 96), ("beta", 96), ("running_mean", 96)):
        d[k] = rng.normal(0, 0.3, size=shape).astype(np.float32)
    d["running_var"] = rng.uniform(0.5, 2.0, size=96).astype(np.float32)
    net = module_for(d).cuda().eval()
    with torch.no_grad():
        got, stated = net(item_of(d, "cuda")), net.forward_torch(item_of(d, "cuda"))
    assert torch.equal(got, stated), "forward() beyond the native limits IS the torch statement"
    own = value_error(stated.cpu().numpy(), ref.canvas(ref.encode(d, training=False)["rows"], d, cases.H, cases.W).numpy())
    print("pillar-fallback-figures", dict(channels=96, fp32_torch=own))
    assert own <= VALUE_BOUND  # (the statement itself: a dozen fp32 operations per value, the project's bound on a value)


# --------------------------------------------------------------------------------------------------------------------- voxelizer
def _sequential_voxels(frames, max_pts, max_voxels):
    """The sequential loop the voxelizer reproduces, on the tiny grid: voxels in first-touch order per frame (at most max_voxels, later
    ones dropped), the first max_pts points of a voxel in input order, zero padded; mean = fp32 sum of the slots in order / occupancy."""
    voxels, coords, occ = [], [], []
    lo, vs = np.asarray(cases.BOUNDS[:3], np.float32), np.asarray(cases.VOXEL, np.float32)
    for b, pts in enumerate(frames):
        index, rows = {}, []
        for q in pts:
            c = np.floor((q[:3] - lo) / vs).astype(np.int64)
            if (c < 0).any() or c[0] >= cases.W or c[1] >= cases.H or c[2] >= 1:
                continue
            key = (int(c[2]), int(c[1]), int(c[0]))
            if key not in index:
                index[key] = len(rows)
                rows.append([])
            rows[index[key]].append(q)
        for key, r in list(zip(index, rows))[:max_voxels]:
            slot = np.zeros((max_pts, pts.shape[1]), np.float32)
            slot[:min(len(r), max_pts)] = np.asarray(r[:max_pts], np.float32)
            voxels.append(slot)
            coords.append((b,) + key)
            occ.append(min(len(r), max_pts))
    voxels = np.asarray(voxels, np.float32).reshape(len(occ), max_pts, frames[0].shape[1])
    mean = np.zeros((len(occ), voxels.shape[2]), np.float32)
    for k in range(max_pts):
        mean = mean + voxels[:, k]
    return voxels, np.asarray(coords, np.int32).reshape(-1, 4), np.asarray(occ, np.int32), mean / np.asarray(occ, np.float32)[:, None]


@pytest.mark.parametrize("max_pts,C,sizes,max_voxels", [(32, 4, (3000,), 400), (9, 5, (700, 0, 900), 400), (64, 4, (2500, 300), 37), (8, 4, (700, 0, 900), 400)],
                         ids=["one_frame_32", "empty_middle_9", "clipped_64", "narrow_8"])
def test_voxelizer_with_pillar_occupancies(max_pts, C, sizes, max_voxels):
    """More than eight slots per voxel (the wide path of csrc/voxelize.hip) against the sequential loop, bit for bit; 8 is the
    register path on the same clouds.  Four crowded cells overflow every slot count, the cells far out stay short."""
    from vision3d_amd.spconv.utils import voxelize_batch
    frames = _crowded_frames(max_pts, C, sizes)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    flat = torch.from_numpy(np.concatenate(frames)).cuda()
    voxels, coords, occ, mean, n_vox = voxelize_batch(flat, offsets, cases.VOXEL, cases.BOUNDS, max_pts, max_voxels)
    m = int(n_vox.item())
    want = _sequential_voxels(frames, max_pts, max_voxels)
    assert m == len(want[2]) and (want[2] == max_pts).any() and (want[2] < max_pts).any()
    for got, ref_ in zip((voxels, coords, occ, mean), want):
        np.testing.assert_array_equal(got[:m].cpu().numpy(), ref_)


def _crowded_frames(max_pts, C, sizes):
    rng = np.random.default_rng([7, max_pts])
    frames = []
    for n in sizes:
        pts = rng.uniform(0.0, 1.0, size=(n, C)).astype(np.float32)
        pts[:, 0] = pts[:, 0] * 6.6 - 0.1   # a few points outside the bounds
        pts[:, 1] = pts[:, 1] * 8.2 - 4.1
        pts[:, 2] = pts[:, 2] * 4.2 - 3.1
        crowd = rng.permutation(n)[:2 * n // 5]  # two points in five fall into four cells at the origin, in any input position
        pts[crowd, 0] = rng.uniform(0.0, 0.8, size=len(crowd)).astype(np.float32)
        pts[crowd, 1] = rng.uniform(-0.8, 0.0, size=len(crowd)).astype(np.float32)
        frames.append(pts)
    return frames


# ------------------------------------------------------------------------------------------------------------------------- model
def _clouds(seeds):
    """Synthetic clouds moved into the tiny grid's bounds (x in [0, 6.4), y in [-4, 4))."""
    from vision3d_amd import synth
    out = []
    for s in seeds:
        cloud = synth.make_cloud(s, n_points=4096).copy()
        cloud[:, 0] = cloud[:, 0] / 70.4 * 6.4
        cloud[:, 1] = cloud[:, 1] / 40.0 * 4.0
        out.append(cloud.astype(np.float32))
    return out


def _model(seed=0):
    from gpu_util import randomize_bn
    from vision3d_amd.detector import Second
    cfg = cases.tiny_cfg()
    torch.manual_seed(seed)
    model = Second(cfg).cuda()
    randomize_bn(model, 0)
    return cfg, model


def _case_of(item, net):
    """The tensors of a Preprocessor item and of the encoder as a case of tests/pillar_ref.py."""
    n = net.norm
    return dict(features=item["features"].cpu().numpy(), occupancy=item["occupancy"].cpu().numpy(), coordinates=item["coordinates"].cpu().numpy(),
                batch_size=int(item["batch_size"]), geom=net.geom, weight=net.linear.weight.detach().cpu().numpy(),
                gamma=n.weight.detach().cpu().numpy(), beta=n.bias.detach().cpu().numpy(), running_mean=n.running_mean.cpu().numpy(),
                running_var=n.running_var.cpu().numpy(), eps=n.eps, momentum=n.momentum)


def test_model_eval_equals_the_model_on_the_torch_statement():
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    from vision3d_amd.detector.pillar import PillarFeatureNet
    cfg, model = _model()
    model.eval()
    assert isinstance(model.vfe, PillarFeatureNet) and not hasattr(model, "cnn")
    anchors = AnchorGenerator(cfg).anchors.cuda()
    assert tuple(anchors.shape) == (1, 2, cases.H, cases.W, 7)
    item = Preprocessor(cfg)(dict(points=_clouds((0, 1)), anchors=anchors))
    assert item["features"].shape[1:] == (cfg.MAX_OCCUPANCY, cfg.C_IN) and int(item["coordinates"][:, 1].abs().max()) == 0
    with torch.no_grad():
        bev = model.vfe(item)
        out = model(dict(item))
        boxes, bidx, cidx, scores = model.inference(item)
        assert out["P_cls"].shape == (2, 1, 2, cases.H, cases.W) and out["P_reg"].shape == (2, 1, 2, cases.H, cases.W, 7)
        assert boxes.shape == (len(bidx), 7) and len(bidx) == len(cidx) == len(scores) and "_head_maps" not in out
        model.vfe.native = False
        bev_t = model.vfe(item)
        out_t = model(dict(item))
        # the bound, by measurement: what a perturbation of the torch-statement map of the SAME size does to the model's outputs,
        # times the margin of four; never below the feature bar of the dense plan's arithmetic (gpu_util.FEATURE_RTOL of the largest)
        delta = (bev - bev_t).abs().max()
        want = ref.canvas(ref.encode(_case_of(item, model.vfe), training=False)["rows"], dict(batch_size=2, coordinates=item["coordinates"].cpu().numpy()),
                          cases.H, cases.W).numpy()
        own, native = value_error(bev_t.cpu().numpy(), want), value_error(bev.cpu().numpy(), want)
        print("pillar-model-figures", dict(encoder_fp32_torch=own, encoder=native))
        assert native <= max(VALUE_BOUND, 4 * own)
        sign = torch.where(torch.rand(bev_t.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(1)) < 0.5, -1.0, 1.0)
        moved = model.head(model.rpn(bev_t + sign * delta * (bev_t != 0)))
    for k, m in (("P_cls", moved[0]), ("P_reg", moved[1])):
        scale = float(out_t[k].abs().max())
        measured = float((m - out_t[k]).abs().max())
        got = float((out[k] - out_t[k]).abs().max())
        print("pillar-model-figures", dict(output=k, encoder_delta=float(delta), perturbed=measured, native_vs_statement=got, largest=scale))
        assert got <= max(1e-4 * scale, 4 * measured)


def _train_item(cfg, clouds):
    from vision3d_amd.core import Preprocessor, ProposalTargetAssigner
    assigner = ProposalTargetAssigner(cfg)
    gts = [np.array([[2.2, -1.1, -1.0, 1.6, 3.9, 1.56, 0.05]], np.float32), np.array([[4.1, 0.7, -1.0, 1.6, 3.9, 1.56, 1.5]], np.float32)]
    targets = [assigner(dict(boxes=torch.from_numpy(g), class_idx=torch.zeros(len(g), dtype=torch.long),
                             box_ignore=torch.zeros(len(g), dtype=torch.bool))) for g in gts]
    item = Preprocessor(cfg, seed=0)(dict(points=[torch.from_numpy(c).cuda() for c in clouds]))
    item.update({k: torch.stack([t[k] for t in targets]) for k in ("G_cls", "G_reg", "M_cls", "M_reg")})
    return item


def _train_step(cfg, m, encoder):
    """One training forward + ProposalLoss + backward of model m with its BEV map made by `encoder(item)`; -> (the map, the gradients
    of the encoder's three parameters as float64 numpy, the loss tensor)."""
    from vision3d_amd.detector import ProposalLoss
    seen = {}

    def forward(item):
        seen["bev"] = encoder(item)
        return seen["bev"]
    m.vfe.forward = forward  # (shadows the class's forward for this instance)
    m.train()
    item = _train_item(cfg, _clouds((0, 1)))
    assert int(item["M_reg"].sum()) > 0
    out = m(item)
    assert isinstance(out["_head_maps"], tuple) and out["_head_maps"][0].dtype == torch.float32
    losses = ProposalLoss(cfg)(out)
    assert torch.isfinite(losses["loss"])
    losses["loss"].backward()
    assert m.torch_dense_fallbacks == 0 and int(m.vfe.norm.num_batches_tracked) == 1
    for p in (m.vfe.linear.weight, m.vfe.norm.weight, m.vfe.norm.bias, m.rpn.down_block[1].weight):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
    grads = [p.grad.cpu().numpy().astype(np.float64) for p in (m.vfe.linear.weight, m.vfe.norm.weight, m.vfe.norm.bias)]
    return seen["bev"].detach(), grads, losses["loss"]


def test_model_trains_through_the_native_encoder():
    """One training forward + ProposalLoss + backward: dense train plan -> canvas backward -> PillarEncodeFunction.  The gradients of
    linear.weight, norm.weight and norm.bias against the same model on the torch statement through the same dense plan, the maximum
    READ at the native model's winners (forward_torch(item, winner=...)), so that no near-tied maximum enters the comparison.  What
    is left between the two is the forward difference of the maps, carried through the dense plan and back.  The bound, by
    measurement: a third copy runs the torch statement with its map moved by that very difference (random signs, occupied entries);
    the native model may differ from the statement by four times what that does to each gradient, relative to the tensor's largest
    entry, never less than the feature bar of the dense plan's arithmetic (gpu_util.FEATURE_RTOL = 1e-4)."""
    from gpu_util import FEATURE_RTOL
    cfg, model = _model()
    twin, moved = copy.deepcopy(model), copy.deepcopy(model)
    native_forward = model.vfe.forward
    bev, got, loss = _train_step(cfg, model, native_forward)
    assert _has_node(loss.grad_fn, "PillarEncodeFunctionBackward"), "the encoder's native Function"
    winner = model.vfe.last_winner
    assert winner is not None and bool((winner == -1).any()) and bool((winner >= 0).any())
    bev_t, want, loss_t = _train_step(cfg, twin, lambda item: twin.vfe.forward_torch(item, winner=winner))
    assert not _has_node(loss_t.grad_fn, "PillarEncodeFunctionBackward")
    delta = (bev - bev_t).abs().max()
    sign = torch.where(torch.rand(bev_t.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(2)) < 0.5, -1.0, 1.0)

    def moved_encoder(item):
        b = moved.vfe.forward_torch(item, winner=winner)
        return b + sign * delta * (b.detach() != 0)
    _, pushed, _ = _train_step(cfg, moved, moved_encoder)
    for what, g, t, p in zip(("linear.weight", "norm.weight", "norm.bias"), got, want, pushed):
        err, measured = grad_error(g, t), grad_error(p, t)
        worst_row = float((np.abs(g - t).reshape(len(t), -1).max(axis=1) / np.abs(t).max()).max())
        print("pillar-model-train-figures", dict(grad=what, map_delta=float(delta), perturbed=measured, native_vs_statement=err, worst_row=worst_row))
        assert err <= max(FEATURE_RTOL, 4 * measured), (what, err, measured)


def test_refusals():
    from vision3d_amd.core.config import pillar_car_cfg
    from vision3d_amd.detector import PV_RCNN, Second
    cfg, model = _model()
    model.eval()
    cloud = [torch.zeros((8, 4), device="cuda")]
    anchors = torch.zeros((1, 2, cases.H, cases.W, 7), device="cuda")
    for call in (lambda: model.graphed_inference(anchors, [8]), lambda: model.pipelined_inference(anchors, [8]),
                 lambda: model.inference_points(cloud, anchors), lambda: model.bev_from_points(cloud),
                 lambda: model.head_maps_from_points(cloud), lambda: model.fused_head_from_points(cloud), lambda: model.backbone_plan(1, 16384),
                 lambda: PV_RCNN(cfg)):
        with pytest.raises(ValueError, match="cfg.PILLAR.ENABLED"):
            call()
    model.set_precision("bf16x3")  # the dense part; there is no sparse part to set
    assert model.rpn.precision == "bf16x3"
    narrow = cases.tiny_cfg()
    narrow.PILLAR.CHANNELS = 64
    with pytest.raises(ValueError, match="CHANNELS"):
        Second(narrow)
    tall = pillar_car_cfg()
    tall.VOXEL_SIZE = [0.4, 0.4, 8.0]
    with pytest.raises(ValueError, match="z extent"):
        Second(tall)
    bad = item_of(cases.build("five"), "cuda")
    bad["coordinates"] = bad["coordinates"].clone()
    bad["coordinates"][0, 1] = 1
    model.vfe.check_coordinates(item_of(cases.build("five"), "cuda")["coordinates"])
    with pytest.raises(ValueError, match="z index"):
        model.vfe.check_coordinates(bad["coordinates"])
    # forward() does not stall on that check: it writes the canvas at z = 0 whatever the item holds, every row in its own (b, y, x) column
    c = cases.build("five")
    net = module_for(c).cuda().eval()
    with torch.no_grad():
        out = net(bad)
    torch.cuda.synchronize()
    co = torch.from_numpy(c["coordinates"].astype(np.int64)).cuda()
    occupied = torch.zeros((c["B"], cases.H, cases.W), dtype=torch.bool, device="cuda")
    occupied[co[:, 0], co[:, 2], co[:, 3]] = True
    assert out.shape == (c["B"], c["CH"], cases.H, cases.W) and float(out.permute(0, 2, 3, 1)[~occupied].abs().max()) == 0.0
    assert bool((out.permute(0, 2, 3, 1)[co[0, 0], co[0, 2], co[0, 3]] != 0).any())


def test_full_size_frame():
    from vision3d_amd import synth
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    from vision3d_amd.core.config import pillar_car_cfg
    from vision3d_amd.detector import Second
    cfg = pillar_car_cfg()
    torch.manual_seed(0)
    model = Second(cfg).cuda().eval()
    anchors = AnchorGenerator(cfg).anchors.cuda()
    item = Preprocessor(cfg)(dict(points=[synth.make_cloud(0, n_points=16384)], anchors=anchors))
    assert item["features"].shape[1:] == (32, 4) and item["features"].shape[0] <= 12000
    with torch.no_grad():
        out = model(dict(item))
        boxes, bidx, cidx, scores = model.inference(item)
    torch.cuda.synchronize()
    assert out["P_cls"].shape == (1, 1, 2, 200, 176) and out["P_reg"].shape == (1, 1, 2, 200, 176, 7)
    assert boxes.shape == (len(scores), 7) and torch.isfinite(out["P_cls"]).all()

"""Capture golden input/output vectors from the REFERENCE itself (run in the build container only).

    python tests/golden/make_golden.py

What runs here is the reference's own code, imported/compiled from /root/reference:
  * vision3d._C (CPU): ops/csrc/{vision.cpp, box_iou_rotated/box_iou_rotated_cpu.cpp,
    nms_rotated/nms_rotated_cpu.cpp} are compiled by torch.utils.cpp_extension in a scratch
    directory under /tmp.  nms_rotated_cpu.cpp:67 needs the one-token torch-2.x API spelling
    `dets.type()` -> `dets.scalar_type()`; that edit is applied to the scratch copy only (the
    arithmetic is untouched) and nothing from the scratch directory enters this repository.
  * the standalone-importable Python files (core/box_encode.py, core/anchor_generator.py,
    core/geometry.py, ops/focal_loss.py, ops/matcher.py, ops/iou_nms.py, detector/layers.py,
    detector/proposal.py, detector/second.py::RPN, core/proposal_targets.py) are imported by path
    with stub modules for the third-party packages they import but do not call on these paths.

Only DATA (inputs, seeds and expected outputs) is written, to tests/golden/*.npz.
"""
import importlib.util
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)

import torch  # noqa: E402

from vision3d_amd import synth  # noqa: E402
from vision3d_amd.core.config import second_car_cfg, _defaults  # noqa: E402


def build_ref_C():
    scratch = tempfile.mkdtemp(prefix="v3d_refC_")
    src = os.path.join(scratch, "csrc")
    shutil.copytree(os.path.join(REF, "vision3d/ops/csrc"), src)
    subprocess.check_call(["sed", "-i", "67s/dets.type()/dets.scalar_type()/",
                           os.path.join(src, "nms_rotated/nms_rotated_cpu.cpp")])
    from torch.utils.cpp_extension import load
    mod = load(name="v3d_ref_C", sources=[os.path.join(src, "vision.cpp"),
                                          os.path.join(src, "box_iou_rotated/box_iou_rotated_cpu.cpp"),
                                          os.path.join(src, "nms_rotated/nms_rotated_cpu.cpp")],
               extra_include_paths=[src], build_directory=scratch, verbose=False)
    return mod


def install_stubs(refC):
    """Make `vision3d.<sub>.<file>` importable straight from /root/reference WITHOUT running the
    package __init__ files (they import yacs/spconv/visdom): each package is a bare module object whose
    __path__ points at the reference directory; third-party imports get empty stub modules."""
    for name in ["spconv", "torchsearchsorted", "pointnet2", "pointnet2.pointnet2_modules",
                 "pointnet2.pointnet2_utils", "torchvision", "torchvision.ops", "torchvision.ops.boxes", "yacs",
                 "yacs.config"]:
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision.ops"].boxes = sys.modules["torchvision.ops.boxes"]
    sys.modules["torchvision.ops"].nms = None
    sys.modules["torchsearchsorted"].searchsorted = None
    pkgs = {}
    for name, path in [("vision3d", []), ("vision3d.ops", [REF + "/vision3d/ops"]),
                       ("vision3d.core", [REF + "/vision3d/core"]), ("vision3d.detector", [REF + "/vision3d/detector"])]:
        m = types.ModuleType(name)
        m.__path__ = path
        sys.modules[name] = m
        pkgs[name] = m
    pkgs["vision3d"]._C = refC
    sys.modules["vision3d._C"] = refC
    return pkgs["vision3d.ops"], pkgs["vision3d.core"]


def load_file(name):
    """import a reference module by dotted name (package stubs above resolve it to the real file)."""
    return importlib.import_module(name)


def rand_boxes(rng, n, ang_scale, center=0.0, spread=10.0):
    xy = rng.uniform(-spread, spread, (n, 2)) + center
    wh = rng.uniform(0.5, 5.0, (n, 2))
    a = rng.uniform(-1, 1, (n, 1)) * ang_scale
    return np.concatenate([xy, wh, a], 1).astype(np.float32)


def kitti_like_bev(rng, n):
    """BEV boxes the way vision3d feeds them: (x, y, w, l, yaw in RADIANS)."""
    x = rng.uniform(0, 70.4, (n, 1))
    y = rng.uniform(-40, 40, (n, 1))
    w = rng.normal(1.6, 0.1, (n, 1))
    l = rng.normal(3.9, 0.3, (n, 1))
    yaw = rng.uniform(-np.pi, np.pi, (n, 1))
    return np.concatenate([x, y, w, l, yaw], 1).astype(np.float32)


def main():
    refC = build_ref_C()
    ops_pkg, core_pkg = install_stubs(refC)
    T = torch.from_numpy
    out = {}
    rng = np.random.default_rng(1234)

    # ---------------- G1: rotated IoU ------------------------------------------------------------
    kat1 = np.array([[0, 0, 2, 2, 0], [0, 0, 2, 2, 0], [0, 0, 2, 2, 0], [5, 3, 4, 2, -90]], np.float32)
    kat2 = np.array([[0, 0, 2, 2, 0], [1, 1, 2, 2, 0], [0, 0, 2, 2, 45], [5, 3, 4, 2, 90]], np.float32)
    out["iou_kat_b1"], out["iou_kat_b2"] = kat1, kat2
    out["iou_kat"] = refC.box_iou_rotated(T(kat1), T(kat2)).numpy()
    for tag, b1, b2 in [
        ("deg", rand_boxes(rng, 64, 180.0), rand_boxes(rng, 64, 180.0)),
        ("rad", kitti_like_bev(rng, 64), kitti_like_bev(rng, 64)),
        ("far", rand_boxes(rng, 48, 180.0, center=7.3e3), rand_boxes(rng, 48, 180.0, center=7.3e3)),
    ]:
        out[f"iou_{tag}_b1"], out[f"iou_{tag}_b2"] = b1, b2
        out[f"iou_{tag}"] = refC.box_iou_rotated(T(b1), T(b2)).numpy()
    # dense cluster (many true overlaps) -- boxes packed into a 12 m square
    b1, b2 = rand_boxes(rng, 64, 180.0, spread=6.0), rand_boxes(rng, 64, 180.0, spread=6.0)
    out["iou_dense_b1"], out["iou_dense_b2"], out["iou_dense"] = b1, b2, refC.box_iou_rotated(T(b1), T(b2)).numpy()
    # degenerates: zero area, identical, edge-touching, parallel edges, special angles, tiny offsets
    base = np.array([[0, 0, 4, 2, 0]], np.float32)
    deg = [base, base.copy()]
    for ang in (0, 45, 90, -90, 180, -180, 30, 1.5, 1e-3):
        b = base.copy(); b[0, 4] = ang; deg.append(b)
    for dx, dy in ((4, 0), (0, 2), (2, 0), (4, 2), (1e-4, 0), (0, 1e-4), (3.999, 0), (4.001, 0)):
        b = base.copy(); b[0, 0] += dx; b[0, 1] += dy; deg.append(b)
    z = base.copy(); z[0, 2] = 0.0; deg.append(z)
    z = base.copy(); z[0, 2] = 1e-8; z[0, 3] = 1e-8; deg.append(z)
    for s in (0.5, 2.0, 0.999, 1.001):
        b = base.copy(); b[0, 2:4] *= s; deg.append(b)
    deg = np.concatenate(deg, 0).astype(np.float32)
    out["iou_degen_b"] = deg
    out["iou_degen"] = refC.box_iou_rotated(T(deg), T(deg)).numpy()

    # target-assignment shape: gt (27) x anchors (70400), yaw in radians fed as degrees (H1)
    cfg = second_car_cfg()
    ag = load_file("vision3d.core.anchor_generator")
    anchors = ag.AnchorGenerator(cfg).anchors  # (1,2,200,176,7)
    out["anchors_shape"] = np.array(anchors.shape)
    out["anchors_sum"] = np.array([anchors.double().sum().item(), anchors.double().abs().sum().item()])
    flat = anchors.view(-1, 7)
    probe_idx = np.array([0, 1, 175, 176, 35199, 35200, 35201, 70399])
    out["anchors_probe_idx"], out["anchors_probe"] = probe_idx, flat[probe_idx].numpy()
    gt = synth.make_gt_boxes(0)
    out["ta_gt"] = gt
    bev = [0, 1, 3, 4, 6]
    iou = refC.box_iou_rotated(T(gt[:, bev].copy()), flat[:, bev].contiguous())
    nz = iou.nonzero()
    out["ta_iou_nz_idx"] = nz.numpy().astype(np.int32)
    out["ta_iou_nz_val"] = iou[nz[:, 0], nz[:, 1]].numpy()

    # ---------------- G2: rotated NMS ---------------------------------------------------------------
    sys.path.insert(0, REPO)
    from oracle import oracle as O
    for n in (100, 800, 4096):
        boxes = kitti_like_bev(rng, n)
        boxes[:, :2] = rng.uniform(0, 30 + n / 40.0, (n, 2))  # crowd them so suppression happens
        scores = rng.permutation(n).astype(np.float32) / n + 0.001
        out[f"nms{n}_boxes"], out[f"nms{n}_scores"] = boxes, scores
        for thr in (0.01, 0.5):
            keep = refC.nms_rotated(T(boxes), T(scores), thr).numpy()
            tag = f"nms{n}_t{int(thr * 100):02d}"
            out[tag + "_keep"] = keep
            out[tag + "_margin"] = np.float32(O.nms_margin(boxes, scores, thr))
    # true-degree boxes, moderately crowded
    boxes = rand_boxes(rng, 512, 180.0, spread=12.0)
    scores = rng.permutation(512).astype(np.float32)
    out["nmsdeg_boxes"], out["nmsdeg_scores"] = boxes, scores
    out["nmsdeg_t30_keep"] = refC.nms_rotated(T(boxes), T(scores), 0.3).numpy()
    out["nmsdeg_t30_margin"] = np.float32(O.nms_margin(boxes, scores, 0.3))

    # ---------------- G3: batched_nms_rotated (ops/iou_nms.py:90-134) ------------------------------
    iou_nms = load_file("vision3d.ops.iou_nms")
    for groups in (1, 3, 8):
        n = 240
        boxes = kitti_like_bev(rng, n)
        boxes[:, 0] = rng.uniform(-20, 20, n)  # negative coordinates on purpose
        boxes[:, 1] = rng.uniform(-20, 20, n)
        scores = rng.permutation(n).astype(np.float32) / n
        idxs = rng.integers(0, groups, n).astype(np.int64)
        keep = iou_nms.batched_nms_rotated(T(boxes), T(scores), T(idxs), 0.01).numpy()
        out[f"bnms{groups}_boxes"], out[f"bnms{groups}_scores"], out[f"bnms{groups}_idxs"] = boxes, scores, idxs
        out[f"bnms{groups}_keep"] = keep
    np.savez_compressed(os.path.join(HERE, "iou_nms.npz"), **out)
    print("iou_nms.npz", {k: v.shape for k, v in out.items() if hasattr(v, "shape") and v.size > 64})

    # ---------------- G4: points in cuboids (core/geometry.py) -------------------------------------
    g = {}
    geom = load_file("vision3d.core.geometry")
    cloud = synth.make_cloud(0)
    import hashlib
    g["cloud_sha256"] = np.frombuffer(hashlib.sha256(cloud.tobytes()).digest(), np.uint8)
    boxes = synth.make_gt_boxes(0)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mask3d = geom.PointsInCuboids(cloud)._get_mask(boxes)
        mask2d = geom.PointsNotInRectangles(cloud)._get_mask(boxes)
        corners = geom.box3d_to_bev_corners(boxes)
    g["boxes"] = boxes
    g["mask3d_packed"] = np.packbits(mask3d, axis=None)
    g["mask2d_packed"] = np.packbits(mask2d, axis=None)
    g["mask_shape"] = np.array(mask3d.shape)
    g["corners"] = corners
    np.savez_compressed(os.path.join(HERE, "geometry.npz"), **g)
    print("geometry.npz in-box points:", int(mask3d.sum()), int(mask2d.sum()))

    # ---------------- G5: elementwise / module goldens ---------------------------------------------
    c = {}
    be = load_file("vision3d.core.box_encode")
    torch.manual_seed(7)
    a7 = flat[torch.randint(0, flat.shape[0], (256,))].clone()
    d7 = torch.randn(256, 7) * 0.3
    boxes7 = be.decode(d7, a7)
    c["be_anchors"], c["be_deltas"], c["be_decoded"] = a7.numpy(), d7.numpy(), boxes7.numpy()
    c["be_encoded"] = be.encode(boxes7, a7).numpy()
    fl = load_file("vision3d.ops.focal_loss")
    x = torch.randn(4, 1, 2, 20, 11) * 3
    t = (torch.rand_like(x) > 0.8).float()
    c["focal_x"], c["focal_t"], c["focal_out"] = x.numpy(), t.numpy(), fl.sigmoid_focal_loss(x, t).numpy()
    c["focal_sum_a"] = fl.sigmoid_focal_loss(x, t, alpha=-1, gamma=1.5, reduction="sum").numpy()
    mt = load_file("vision3d.ops.matcher")
    q = torch.rand(9, 500)
    q[:, :7] = torch.tensor([0.45, 0.6, 0.4499, 0.5999, 0.0, 1.0, 0.3])[None]
    for allow in (False, True):
        m, l = mt.Matcher([0.45, 0.60], [0, -1, 1], allow)(q)
        c[f"match_idx_{int(allow)}"], c[f"match_lab_{int(allow)}"] = m.numpy(), l.numpy()
    c["match_q"] = q.numpy()
    m, l = mt.Matcher([0.45, 0.60], [0, -1, 1], False)(torch.zeros(0, 33))
    c["match_empty_idx"], c["match_empty_lab"] = m.numpy(), l.numpy()
    ly = load_file("vision3d.detector.layers")
    feat = torch.randn(300, 5, 4)
    occ = torch.randint(1, 6, (300,)).int()
    for i in range(300):
        feat[i, occ[i]:] = 0
    c["vfe_feat"], c["vfe_occ"], c["vfe_out"] = feat.numpy(), occ.numpy(), ly.VoxelFeatureExtractor()(feat, occ).numpy()
    gat = ly.BEVFeatureGatherer(cfg, torch.tensor(cfg.GRID_BOUNDS[:3]).float(), torch.tensor(cfg.VOXEL_SIZE).float())
    fmap = torch.randn(1, 4, 200, 176)
    kp = torch.stack([torch.rand(1, 64) * 72 - 1, torch.rand(1, 64) * 82 - 41, torch.rand(1, 64) * 4 - 3], -1)
    c["bev_map"], c["bev_kp"], c["bev_out"] = fmap.numpy(), kp.numpy(), gat(fmap, kp).numpy()

    # ProposalLayer / ProposalLoss (detector/proposal.py) with the reference's own ops underneath
    ops_pkg.sigmoid_focal_loss = fl.sigmoid_focal_loss
    ops_pkg.batched_nms_rotated = iou_nms.batched_nms_rotated
    ops_pkg.box_iou_rotated = refC.box_iou_rotated
    ops_pkg.Matcher = mt.Matcher
    prop = load_file("vision3d.detector.proposal")
    torch.manual_seed(11)
    layer = prop.ProposalLayer(cfg)
    with torch.no_grad():
        layer.conv_cls.weight.normal_(0, 0.05)
        layer.conv_reg.weight.normal_(0, 0.02)
        layer.conv_cls.bias.fill_(-1.0)
    # a small BEV map is enough to pin the head semantics (anchors regenerated at matching size)
    small_cfg = second_car_cfg()
    small_cfg.GRID_BOUNDS = [0, -8.0, -3, 12.8, 8.0, 1]  # -> 40 x 32 BEV cells
    small_anchors = ag.AnchorGenerator(small_cfg).anchors
    c["pl_anchor_shape"] = np.array(small_anchors.shape)
    fm = torch.randn(2, 128, small_anchors.shape[2], small_anchors.shape[3])
    with torch.no_grad():
        cls_map, reg_map = layer(fm)
        boxes_o, bidx, cidx, scores_o = layer.inference(fm.clone(), small_anchors)
    c["pl_state"] = np.concatenate([p.detach().numpy().ravel() for p in layer.state_dict().values()])
    c["pl_fm"] = fm.numpy()
    c["pl_cls"], c["pl_reg"] = cls_map.numpy(), reg_map.numpy()
    c["pl_boxes"], c["pl_bidx"], c["pl_cidx"], c["pl_scores"] = boxes_o.numpy(), bidx.numpy(), cidx.numpy(), scores_o.numpy()
    loss = prop.ProposalLoss(cfg)
    G_cls = (torch.rand_like(cls_map) > 0.97).long()
    M_cls = torch.rand_like(cls_map) > 0.1
    M_reg = (G_cls == 1).unsqueeze(-1)
    G_reg = torch.randn_like(reg_map) * M_reg
    item = dict(G_cls=G_cls, M_cls=M_cls, P_cls=cls_map, G_reg=G_reg, M_reg=M_reg, P_reg=reg_map)
    with torch.no_grad():
        losses = loss(item)
    c["loss_G_cls"], c["loss_M_cls"], c["loss_G_reg"], c["loss_M_reg"] = G_cls.numpy(), M_cls.numpy(), G_reg.numpy(), M_reg.numpy()
    c["loss_vals"] = np.array([losses["cls_loss"].item(), losses["reg_loss"].item(), losses["loss"].item()])

    # RPN (detector/second.py:49-94): dense head on a small map, eval mode with non-trivial BN stats
    mod = load_file("vision3d.detector.second")
    torch.manual_seed(21)
    rpn = mod.RPN(C_in=32, C_up=32, C_down=32, blocks=5).eval()  # same graph, 32 channels: small fixture
    with torch.no_grad():
        for m_ in rpn.modules():
            if isinstance(m_, torch.nn.BatchNorm2d):
                m_.running_mean.normal_(0, 0.2); m_.running_var.uniform_(0.5, 1.5)
                m_.weight.uniform_(0.5, 1.5); m_.bias.normal_(0, 0.2)
        xin = torch.randn(1, 32, 24, 20)
        yout = rpn(xin)
    c["rpn_keys"] = np.array(list(rpn.state_dict().keys()))
    c["rpn_state"] = np.concatenate([p.detach().double().numpy().ravel() for p in rpn.state_dict().values()]).astype(np.float32)
    c["rpn_in"], c["rpn_out"] = xin.numpy(), yout.numpy()

    # ProposalTargetAssigner (core/proposal_targets.py) -- the reference moves anchors to .cuda() in
    # __init__ (proposal_targets.py:19); on this CPU-only container .cuda() is patched to identity.
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        pt = load_file("vision3d.core.proposal_targets")
        assigner = pt.ProposalTargetAssigner(cfg)
        gtb = torch.from_numpy(synth.make_gt_boxes(0))
        item = dict(boxes=gtb, class_idx=torch.zeros(gtb.shape[0], dtype=torch.long),
                    box_ignore=torch.zeros(gtb.shape[0], dtype=torch.bool))
        item["box_ignore"][3] = True
        assigner(item)
    finally:
        torch.Tensor.cuda = orig_cuda
    c["pta_G_cls_idx"] = item["G_cls"].nonzero().numpy().astype(np.int32)
    c["pta_M_cls_zero_idx"] = (~item["M_cls"]).nonzero().numpy().astype(np.int32)
    mr = item["M_reg"].squeeze(-1)
    c["pta_M_reg_idx"] = mr.nonzero().numpy().astype(np.int32)
    c["pta_G_reg_vals"] = item["G_reg"][mr].numpy()
    c["pta_shapes"] = np.array([list(item["G_cls"].shape) + [0], list(item["G_reg"].shape)], dtype=object).astype(str)
    sys.path.insert(0, HERE)
    from npz_parts import save_parts
    save_parts(os.path.join(HERE, "core"), c)  # core.npz + core.part*.npz (no committed file above 1 MiB)
    print("core.npz", {k: v.shape for k, v in c.items() if hasattr(v, "shape") and v.size > 64})
    print("detections in pl golden:", c["pl_boxes"].shape, "positives in pta:", c["pta_M_reg_idx"].shape)


if __name__ == "__main__":
    main()

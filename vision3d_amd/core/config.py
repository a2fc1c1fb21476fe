"""Hyper-parameter tree for the hot path.

Mirrors the attribute surface of the reference's yacs global (`vision3d/core/config.py:4-110`:
`cfg.VOXEL_SIZE`, `cfg.PROPOSAL.TOPK`, `cfg.ANCHORS[i]['wlh']`, `cfg.merge_from_file(path)` ...)
without depending on yacs, which is not installed here.  Only the keys the hot path reads are
defaulted; unknown keys in a YAML override are accepted and stored.
"""
import copy
import math

import yaml


class Node(dict):
    """dict with attribute access; nested dicts become Nodes (lists of dicts stay plain dicts,
    because the reference indexes anchors as `anchor['wlh']`)."""

    def __init__(self, init=None):
        super().__init__()
        for k, v in (init or {}).items():
            self[k] = Node(v) if isinstance(v, dict) and not isinstance(v, Node) else v

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        self[name] = value

    def __deepcopy__(self, memo):
        return Node({k: copy.deepcopy(v, memo) for k, v in self.items()})

    def clone(self):
        return copy.deepcopy(self)

    def merge_from_dict(self, other):
        for k, v in other.items():
            if isinstance(v, dict) and isinstance(self.get(k), Node):
                self[k].merge_from_dict(v)
            else:
                self[k] = Node(v) if isinstance(v, dict) else v
        if "ANCHORS" in other and "NUM_CLASSES" not in other:
            self["NUM_CLASSES"] = len(self["ANCHORS"])
        return self

    def merge_from_file(self, path):
        with open(path) as f:
            return self.merge_from_dict(yaml.safe_load(f) or {})


def _defaults():
    half_pi = math.pi / 2
    anchors = [
        dict(names=["Car", "Van"], wlh=[1.6, 3.9, 1.56], yaw=[0, half_pi], iou_thresh=[0.45, 0.60],
             score_thresh=0.3, center_z=-1.0),
        dict(names=["Pedestrian", "Person_sitting"], wlh=[0.6, 0.8, 1.73], yaw=[0, half_pi],
             iou_thresh=[0.20, 0.35], score_thresh=0.3, center_z=-0.6),
        dict(names=["Cyclist"], wlh=[0.6, 1.76, 1.73], yaw=[0, half_pi], iou_thresh=[0.20, 0.35],
             score_thresh=0.3, center_z=-0.6),
    ]
    return Node(dict(
        C_IN=4, NUM_KEYPOINTS=2048, STRIDES=[1, 2, 4, 8], SAMPLES_PN=[16, 32],
        # keypoint sampler of PV-RCNN: "fps" (one farthest-point chain per cloud), "sector" (a chain per azimuth sector) or "spc"
        # (sectorized AND proposal-centric: only points within RADIUS of a stage-1 proposal) -- pointnet2_utils.sector_point_sample
        KEYPOINTS=dict(SAMPLER="fps", NUM_SECTORS=6, RADIUS=1.6),
        # Predicted Keypoint Weighting of PV-RCNN (detector/keypoint_weighting.py), opt-in: a foreground head over the keypoint features
        # (hidden widths MLPS) whose sigmoid scales every keypoint's row before RoI-grid pooling; supervised by a focal loss on
        # "inside a ground-truth box", keypoints inside a box grown by GT_EXTRA_WIDTH (w, l, h) only are ignored
        PKW=dict(ENABLED=False, MLPS=[256], GT_EXTRA_WIDTH=[0.2, 0.2, 0.2], FOCAL_ALPHA=0.25, FOCAL_GAMMA=2.0, LOSS_WEIGHT=1.0),
        # voxel RoI pooling for stage 2 of PV-RCNN (detector/voxel_roi_pool.py), opt-in: the GRID^3 regular grid points of every RoI
        # query the backbone's own voxels of LEVELS (1: the voxelized input, k + 1: the output of stage k -- strides 2, 4, 8 and
        # channels 32, 64, 64 for [2, 3, 4]) inside an index window of half-widths RANGE (rz, ry, rx) and a RADIUS in metres, at most
        # NSAMPLE per point, pooled by a PointNet per level (MLPS after the 3 + C input) and reduced per RoI (MLPS_REDUCTION; None:
        # [GRID^3 * 96, 256, 256], a given list must start with that width); LEVEL_CHANNELS: None = the backbone's channels of LEVELS,
        # else the channel count per level (levels that do not come from this backbone); replaces keypoints, set abstraction, BEV lookup and RoI-grid pooling
        VOXELPOOL=dict(ENABLED=False, GRID=6, LEVELS=[2, 3, 4], RANGE=[[2, 2, 2], [2, 2, 2], [1, 2, 2]], RADIUS=[0.4, 0.8, 1.6],
                       NSAMPLE=16, MLPS=[[32, 32], [32, 32], [32, 32]], MLPS_REDUCTION=None, LEVEL_CHANNELS=None),
        # VectorPool aggregation of PV-RCNN++ (detector/vector_pool.py), opt-in: replaces the set-abstraction modules of the keypoint
        # feature extraction (PSA: one entry per feature source -- raw points, then the four CNN levels) and of RoI-grid pooling
        # (GRIDPOOL).  REDUCED: channels after the grouped sum (must divide the source's channel count), LOCAL: width of every
        # sub-voxel's own linear layer, GROUPS: VOXELS [vx, vy, vz] sub-voxels, the radius (PSA: RADIUS_SCALE times the source's larger
        # cfg.PSA.RADII entry, or an explicit RADIUS; GRIDPOOL: RADIUS in metres) and the group's MLP widths POST; MSG_POST: widths behind
        # the concatenated groups -- the defaults end in the widths of the set-abstraction modules (32, 32, 64, 128, 128 and 192), so the
        # keypoint features stay 512 wide and NUM_GRIDPOINTS * MSG_POST[-1] = GRIDPOOL.MLPS_REDUCTION[0]; refused together with VOXELPOOL
        VECTORPOOL=dict(ENABLED=False,
                        PSA=dict(REDUCED=[1, 4, 16, 32, 32], LOCAL=32, MSG_POST=[[32], [32], [64], [128], [128]],
                                 GROUPS=[dict(VOXELS=[2, 2, 2], RADIUS_SCALE=0.5, POST=[32, 32]),
                                         dict(VOXELS=[3, 3, 3], RADIUS_SCALE=1.0, POST=[32, 32])]),
                        GRIDPOOL=dict(REDUCED=32, LOCAL=32, MSG_POST=[192],
                                      GROUPS=[dict(VOXELS=[3, 3, 3], RADIUS=0.8, POST=[64, 64]), dict(VOXELS=[3, 3, 3], RADIUS=1.6, POST=[64, 64])])),
        # anchor-free centre heatmap head for SECOND (detector/center_head.py, core/center_targets.py), opt-in: a class heat map + eight raw
        # regression channels (dx, dy, z, log w, log l, log h, sin yaw, cos yaw) per BEV cell in place of the anchor head; targets are
        # Gaussian splats of CornerNet radius (MIN_OVERLAP, at least MIN_RADIUS cells), the loss the penalty-reduced focal loss
        # (FOCAL_ALPHA, FOCAL_BETA) + L1 weighted by CODE_WEIGHTS, inference the PROPOSAL.TOPK heat peaks per (frame, class) through
        # rotated NMS at NMS_IOU and the score_thresh of ANCHORS
        CENTERHEAD=dict(ENABLED=False, MIN_OVERLAP=0.1, MIN_RADIUS=2, FOCAL_ALPHA=2.0, FOCAL_BETA=4.0, CODE_WEIGHTS=[1.0] * 8,
                        NMS_IOU=0.01),
        # direction classifier + sine yaw loss of the SECOND paper for the anchor head (detector/proposal.py; not in the reference), opt-in:
        # the encoded yaw residual is right only modulo pi, so one more logit per anchor says which half turn -- target = the bit
        # floor(remainder(yaw - OFFSET, 2 pi) / pi) of the matched ground truth's absolute yaw (core/proposal_targets.py G_dir), loss =
        # BCE-with-logits over the positives times LOSS_WEIGHT; decode = remainder(anchor yaw + residual - OFFSET, pi) + OFFSET + pi * [logit
        # > 0].  SIN_YAW: the yaw column of the box loss takes sin(P_yaw - G_yaw) as its smooth-L1 argument (no cliff between residuals 0
        # and pi).  The default OFFSET puts the bin edges on the diagonals, away from the axis-aligned headings and both anchor yaws
        DIRECTION=dict(ENABLED=False, OFFSET=0.7853981634, SIN_YAW=True, LOSS_WEIGHT=0.2),
        # IoU-aware confidence for the anchor head (detector/proposal.py; the rectified score of CIA-SSD / SE-SSD / SECOND-IoU, not in the
        # reference), opt-in: one more logit per anchor predicts the rotated 3-D IoU of the anchor's decoded box with its object -- target
        # (positives only, a constant) = clamp(IoU3D(decode(P_reg), decode(G_reg)), 0, 1), loss = soft-target BCE-with-logits over the
        # positives / max(#positives, 1) times LOSS_WEIGHT; inference picks the TOPK of a (frame, class) by class score as before, then
        # ranks, suppresses and cuts by score * sigmoid(logit)^POWER (POWER an integer in 0 .. 8; 0: train the head, leave the scores alone)
        IOU_HEAD=dict(ENABLED=False, LOSS_WEIGHT=1.0, POWER=4),
        # IoU-weighted box voting behind the rotated NMS tails (ops/box_voting.py, csrc/box_voting.hip; box voting / weighted NMS / the
        # DI-NMS of CIA-SSD, the step those detectors pair with the rectified score of IOU_HEAD; not in the reference), opt-in: after
        # greedy NMS every surviving box is replaced by the mean of the candidates j of its (frame, class) group with BEV IoU u_j >= IOU
        # with it, weighted by s_j * u_j -- s_j the score the NMS ranked by --, as offsets from the survivor (yaw differences wrapped
        # modulo pi: the survivor keeps its heading half).  Boxes move only: the NMS and the score cut decide on the un-voted boxes, and
        # scores, indices, order and count stay; voted survivors may overlap again.  ProposalLayer's tails (Second; PV_RCNN's final
        # tail, not its stage-1 proposals) apply it; the centre heatmap head refuses it.  IOU in (0, 1]; 0.3 is a hyper-parameter
        # default, not a tuned value (no trained weights: the effect on AP is not measured)
        BOX_VOTING=dict(ENABLED=False, IOU=0.3),
        # pillar feature encoder for SECOND (detector/pillar.py; the PFN layer of PointPillars, not in the reference), opt-in: with a voxel
        # as tall as the grid the voxelizer's slots are pillars; every point becomes [channels | xyz - pillar mean | xyz - pillar centre],
        # linear -> BatchNorm1d over all slots -> ReLU -> maximum per pillar gives CHANNELS numbers per occupied BEV cell, scattered
        # straight into the map the dense RPN reads (no sparse 3-D backbone; the dense plans are 128 wide, so Second takes CHANNELS=128).
        # DYNAMIC (inert unless ENABLED; DynamicPillarFeatureNet, the DynamicPillarVFE of MVF): the Preprocessor voxelizes dynamically and
        # ignores MAX_OCCUPANCY, EVERY point of a pillar enters the maximum and the BatchNorm statistics (no padded rows); same parameters.
        # PLAN (inert unless ENABLED; runtime.PillarPlan, inference only): the raw-point entry points of Second -- inference_points, the
        # captured-graph and pipelined runners, bev / head maps from points -- run on a native plan (voxelizer + an encode kernel that
        # writes the dense head's split planes, occupancy bitmap and range flag itself, no host read) instead of refusing the pillar
        # encoder; forward / inference on a Preprocessor item are untouched; refused together with DYNAMIC (a follow-up)
        PILLAR=dict(ENABLED=False, CHANNELS=128, DYNAMIC=False, PLAN=False),
        # dynamic voxelization (csrc/voxelize.hip "DYNAMIC"; MVF / DynamicScatter, not in the reference), opt-in: a voxel takes EVERY point
        # inside it instead of the first MAX_OCCUPANCY in input order -- same cells, same row order, `occupancy` = the true counts,
        # `voxel_mean` an order-independent mean (integer sums of the values scaled by 2^24), a `point_voxel` map and no `features` slot
        # tensor; values must stay below 2^16 in magnitude, at most 2^22 points per call; refused together with PILLAR (its hard encoder
        # reads the point slots; cfg.PILLAR.DYNAMIC is the way to dynamic pillars)
        DYNAMIC_VOXELIZATION=dict(ENABLED=False),
        MAX_VOXELS=20000, MAX_OCCUPANCY=5, VOXEL_SIZE=[0.05, 0.05, 0.1],
        GRID_BOUNDS=[0, -40, -3, 70.4, 40, 1],
        CNN="SpMiddleFHD",
        ANCHORS=anchors, NUM_PROPOSAL_SAMPLE=-1, ALLOW_LOW_QUALITY_MATCHES=False,
        NUM_CLASSES=len(anchors), NUM_YAW=2, BOX_DOF=7,
        PSA=dict(
            RADII=[[0.4, 0.8], [0.4, 0.8], [0.8, 1.2], [1.2, 2.4], [2.4, 4.8]],
            MLPS=[[[1, 8, 16], [1, 8, 16]], [[4, 8, 16], [4, 8, 16]], [[32, 32, 32], [32, 32, 32]],
                  [[64, 64, 64], [64, 64, 64]], [[64, 64, 64], [64, 64, 64]]],
        ),
        GRIDPOOL=dict(NUM_GRIDPOINTS=16, RADII_PN=[0.8, 1.6], MLPS_PN=[[512, 192, 96], [512, 192, 96]],
                      MLPS_REDUCTION=[16 * 192, 256, 256]),
        PROPOSAL=dict(C_IN=128, TOPK=100),
        REFINEMENT=dict(MLPS=[256, 128]),
        # REFINEMENT_IOU_LOSS: rotated 3-D IoU loss on the DECODED stage-2 boxes (detector/refinement.py RefinementLoss, ops/iou_loss.py;
        # not in the reference), opt-in: refine_iou_loss = mean over M_rreg of 1 - IoU(decode(R_reg, proposal), matched ground truth)
        # (KIND "iou") or of 1 - IoU + centre distance^2 / enclosing diagonal^2 ("diou"), added to the stage-2 loss times WEIGHT
        TRAIN=dict(LR=1e-3, LAMBDA=1.0, EPOCHS=80, BATCH_SIZE=6, REFINEMENT_NUM_NEGATIVES=128,
                   REFINEMENT_IOU_LOSS=dict(ENABLED=False, KIND="iou", WEIGHT=1.0)),
        # OBJECT_NOISE: per-object ground-truth noise (dataset/augmentation.py ObjectNoiseAugmentation; VoxelNet 3.1 / SECOND, not in the
        # reference), opt-in: every box, with the points inside it, tries up to NUM_TRY poses -- translation ~ N(0, TRANSLATION_STD)
        # (x, y, z), yaw + U(ROTATION) -- and takes the first whose BEV IoU with every other box is <= COLLISION_IOU, or stays; runs
        # before GT sampling and the global flip / scale / rotation
        AUG=dict(GLOBAL_SCALE=[0.95, 1.05], GLOBAL_ROTATION=[-math.pi / 4, math.pi / 4], FLIP_HORIZONTAL=True,
                 DATABASE_SAMPLE=True, NUM_SAMPLE_OBJECTS=[15, 10, 10], MIN_NUM_SAMPLE_PTS=8,
                 OBJECT_NOISE=dict(ENABLED=False, NUM_TRY=100, TRANSLATION_STD=[1.0, 1.0, 0.5], ROTATION=[-0.7853981634, 0.7853981634],
                                   COLLISION_IOU=1e-2)),
    ))


# configs/second/car.yaml:1-18 restated as data: the single shipped override (car-only SECOND).
SECOND_CAR = dict(
    MAX_OCCUPANCY=5, MAX_VOXELS=20000, GRID_BOUNDS=[0, -40.0, -3, 70.4, 40.0, 1],
    ANCHORS=[dict(names=["Car", "Van"], wlh=[1.6, 3.9, 1.56], yaw=[0, 1.501], iou_thresh=[0.45, 0.60],
                  score_thresh=0.3, center_z=-1.0)],
    NUM_CLASSES=1,
    TRAIN=dict(BATCH_SIZE=4, LAMBDA=1.0, EPOCHS=60),
    AUG=dict(NUM_SAMPLE_OBJECTS=[15, 0, 0]),
)

# BASELINE.json configs[4]: Waymo-range sweep; MAX_VOXELS lifted.
WAYMO_RANGE = dict(GRID_BOUNDS=[-75.2, -75.2, -2.0, 75.2, 75.2, 4.0], MAX_VOXELS=400000)

# PointPillars' KITTI grid on the bounds above: 0.4 m pillars over the whole z extent, map stride 1 -- the same 200 x 176 map the RPN
# sees behind the sparse backbone (0.05 m voxels, stride 8).
PILLAR_KITTI = dict(VOXEL_SIZE=[0.4, 0.4, 4.0], STRIDES=[1], MAX_OCCUPANCY=32, MAX_VOXELS=12000, PILLAR=dict(ENABLED=True))


DYNAMIC_VOXELIZATION_DEFAULTS = dict(ENABLED=False)


def dynamic_voxel_config(cfg):
    """-> the keys of cfg.DYNAMIC_VOXELIZATION over their defaults (a config written before the key existed means "disabled")."""
    out = dict(DYNAMIC_VOXELIZATION_DEFAULTS)
    out.update(cfg.get("DYNAMIC_VOXELIZATION") or {})
    return out


def dynamic_voxel_enabled(cfg):
    return bool(dynamic_voxel_config(cfg)["ENABLED"])


IOU_HEAD_DEFAULTS = dict(ENABLED=False, LOSS_WEIGHT=1.0, POWER=4)


def iou_head_config(cfg):
    """-> the keys of cfg.IOU_HEAD over their defaults (a config written before the key existed means "disabled")."""
    out = dict(IOU_HEAD_DEFAULTS)
    out.update(cfg.get("IOU_HEAD") or {})
    return out


BOX_VOTING_DEFAULTS = dict(ENABLED=False, IOU=0.3)


def box_voting_config(cfg):
    """-> the keys of cfg.BOX_VOTING over their defaults (a config written before the key existed means "disabled"); an enabled key
    whose IOU is not a finite real in (0, 1] is refused (a disabled one does not read it)."""
    out = dict(BOX_VOTING_DEFAULTS)
    out.update(cfg.get("BOX_VOTING") or {})
    if out["ENABLED"]:
        iou = out["IOU"]
        if isinstance(iou, bool) or not isinstance(iou, (int, float)) or not math.isfinite(iou) or not 0 < iou <= 1:
            raise ValueError(f"cfg.BOX_VOTING.IOU must be a finite real in (0, 1], got {iou!r}")
    return out


def refuse_dynamic_with_pillar(cfg):
    """The pillar encoder reads the point slots of the hard voxelizer, which the dynamic form does not produce."""
    if dynamic_voxel_enabled(cfg) and bool((cfg.get("PILLAR") or {}).get("ENABLED", False)):
        raise ValueError("cfg.DYNAMIC_VOXELIZATION.ENABLED together with cfg.PILLAR.ENABLED: the pillar encoder reads the (M, P, C) point "
                         "slots, which dynamic voxelization does not produce; set cfg.PILLAR.DYNAMIC instead (with DYNAMIC_VOXELIZATION "
                         "off): the dynamic pillar encoder voxelizes dynamically itself and reads point_voxel")


def pillar_dynamic_enabled(cfg):
    """cfg.PILLAR.ENABLED and cfg.PILLAR.DYNAMIC (a config written before the key existed means "hard pillars")."""
    opt = cfg.get("PILLAR") or {}
    return bool(opt.get("ENABLED", False)) and bool(opt.get("DYNAMIC", False))


def pillar_plan_enabled(cfg):
    """cfg.PILLAR.ENABLED and cfg.PILLAR.PLAN (a config written before the key existed means "off": the raw-point entry points refuse
    the pillar encoder).  Together with cfg.PILLAR.DYNAMIC it is refused."""
    opt = cfg.get("PILLAR") or {}
    on = bool(opt.get("ENABLED", False)) and bool(opt.get("PLAN", False))
    if on and bool(opt.get("DYNAMIC", False)):
        raise ValueError("cfg.PILLAR.PLAN together with cfg.PILLAR.DYNAMIC: the plan runs the hard pillar encoder; the dynamic encoder "
                         "is a follow-up -- its encode kernel is the slower of the two (DESIGN.md section 7)")
    return on


def second_car_cfg():
    return _defaults().merge_from_dict(copy.deepcopy(SECOND_CAR))


def pillar_car_cfg():
    return second_car_cfg().merge_from_dict(copy.deepcopy(PILLAR_KITTI))


def pillar_dynamic_car_cfg():
    return pillar_car_cfg().merge_from_dict(dict(PILLAR=dict(DYNAMIC=True)))


def pillar_plan_car_cfg():
    return pillar_car_cfg().merge_from_dict(dict(PILLAR=dict(PLAN=True)))


def waymo_range_cfg():
    return second_car_cfg().merge_from_dict(copy.deepcopy(WAYMO_RANGE))


cfg = _defaults()

"""The pillar encoder's native plan (cfg.PILLAR.PLAN, opt-in): raw points -> the dense head's input with no host read.

`PillarPlan(vfe, cfg)` stands where `runtime.BackbonePlan` stands for the sparse model: it presents the part of that interface which
`Second`'s raw-point entry points and the captured-graph runners (detector/graph.py) drive, with the same meanings, so those run on it
unchanged.  A frame is three launches behind the voxelizer's: v3d_pillar_planes_clear (bitmap, summary word and -- persistent planes --
the previous frame's pixels), v3d_voxelize (hard pillars: MAX_OCCUPANCY slots), v3d_pillar_encode_planes (csrc/pillar.hip "the plan's
front": the encoder writing split NHWC planes, inverted occupancy bitmap and range flag itself).  Inference only; hard pillars only.
"""
import torch

from . import _lib as L
from .runtime import CALIB_HEADROOM_BITS, RangeOverflow, tag_planes
from .stamp import stamp_of

CHANNELS = 128  # the dense plans' width (Second refuses another cfg.PILLAR.CHANNELS)


class PillarPlan(object):
    """Owns, sized by capacity (cap = min(max_points, max_batch * MAX_VOXELS) pillars): the point slots (cap, P, C), the occupancy, TWO
    coordinate lists with their device counts, the voxelizer's workspace, the persistent split planes (max_batch, H, W, 128) hi / lo,
    the inverted occupancy bitmap, one 4-float scale entry {s, 1/s, limit, max} of the planes (f16s) and one summary word.

    The two coordinate lists: list 1 is the one the PERSISTENT planes were last written from -- only forward_split(persistent=True)
    writes it, and its clear launch reads it before the voxelizer overwrites it, so a captured graph (fixed addresses) always zeroes
    exactly the pixels of the frame before; list 0 serves every other call, which therefore never disturbs the persistent planes.

    f16s ("fp32") calibration runs eagerly, never under stream capture, on the first frame and after `recalibrate()` (or new weights):
    the frame's rows go through the existing v3d_pillar_encode into a capacity buffer, v3d_act_scale_from_rows derives the entry from
    them (device count, CALIB_HEADROOM_BITS of margin), then the frame itself runs -- no second pass over the frame.  A later frame
    whose largest row value passes the entry's limit raises the summary word to 2 (RangeOverflow through check_overflow or the
    proposal stage's read).  Underflow (summary word 3, the sparse plan's quiet check) is NOT raised by this plan: its planes hold one
    tensor straight from fp32 rows, and the dense head behind it calibrates its own layers.  "bf16x3" has no entry and no flag.
    Capacities cannot overflow (the voxelizer clips at MAX_VOXELS by definition), so the summary word is never 1."""

    def __init__(self, vfe, cfg, max_batch=1, max_points=None, device=None, precision="bf16x3"):
        from .detector.pillar import MAX_C, MAX_P, MIN_C
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.vfe, self.cfg = vfe, cfg
        self.P, self.C = int(cfg.MAX_OCCUPANCY), int(cfg.C_IN)
        if vfe.channels != CHANNELS or not (1 <= self.P <= MAX_P and MIN_C <= self.C <= MAX_C):
            raise ValueError(f"PillarPlan: CHANNELS {vfe.channels}, MAX_OCCUPANCY {self.P}, C_IN {self.C} are outside the native encoder's "
                             f"limits (128 channels, 1 <= P <= {MAX_P}, {MIN_C} <= C <= {MAX_C})")
        self.max_batch = int(max_batch)
        self.max_points = int(max_points if max_points is not None else 16384 * max_batch)
        self.max_voxels = int(cfg.MAX_VOXELS)
        self.cap = max(1, min(self.max_points, self.max_batch * self.max_voxels))
        self.map_shape = tuple(vfe.map_shape)
        h, w = self.map_shape
        dev, i32 = self.device, torch.int32
        self.slots = torch.zeros((self.cap, self.P, self.C), dtype=torch.float32, device=dev)
        self.occupancy = torch.zeros(self.cap, dtype=i32, device=dev)
        self.coords = torch.zeros((2, self.cap, 4), dtype=i32, device=dev)
        self.counts = torch.zeros(2, dtype=i32, device=dev)
        self.vox_ws = L.workspace(L.lib().v3d_voxelize_workspace(self.max_points), dev)
        self.planes = torch.zeros((2, self.max_batch, h, w, CHANNELS), dtype=torch.int16, device=dev)
        self.bitmap = torch.full((self.max_batch * h, (w + 31) // 32), -1, dtype=i32, device=dev)
        self.entry = torch.tensor([1.0, 1.0, 32768.0, 0.0], dtype=torch.float32, device=dev)
        self.summary = torch.zeros(1, dtype=i32, device=dev)
        self._rows = None  # (cap, 128) f32 of a calibration pass, allocated by the first one
        self._stamp, self._keep = None, None
        self.calibration_generation = 0
        self.precision = None
        self.set_precision(precision)

    # ---- arithmetic and its scale entry (f16s)
    def set_precision(self, precision):
        if precision not in L.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(L.PRECISIONS)}")
        if self.precision is not None and L.PRECISIONS[precision] == L.PRECISIONS[self.precision]:
            return
        self.precision = precision
        self._calib = "need" if self.f16s else "off"

    @property
    def f16s(self):
        return L.PRECISIONS[self.precision] == L.PREC_F16S

    def bev_entry(self):
        """(4,) device entry of the split planes (DenseHeadPlan.forward's `in_entry`); None for bf16x3."""
        return self.entry if self.f16s else None

    def recalibrate(self):
        """f16s: the next eager forward re-derives the scale entry from its own frame (after a RangeOverflow)."""
        if self.f16s:
            self._calib = "need"

    def copy_calibration(self, other):
        """Take another plan's scale entry (the plans of a pipeline's slots share one calibration)."""
        if self.f16s and other.f16s and isinstance(other, PillarPlan):
            self.entry.copy_(other.entry)
            self._calib = other._calib
            if other._calib == "done":
                self.calibration_generation += 1

    def set_throughput_mode(self, on=True):
        """Accepted for PipelinedSecond; no effect: the plan has one kernel per step, none chosen by load."""

    # ---- parameters
    def _param_stamp(self):
        n = self.vfe.norm
        return stamp_of((self.vfe.linear.weight, n.running_mean, n.running_var, n.weight, n.bias))

    def sync_weights(self):
        """Take the encoder's weight and folded BatchNorm (PillarFeatureNet._folded: the tensors vfe(item) multiplies by) if a module
        tensor changed since the last call."""
        stamp = self._param_stamp()
        if stamp == self._stamp:
            return
        if self.vfe.norm.training:
            raise RuntimeError("PillarPlan runs eval-mode BatchNorm only (call model.eval())")
        if self.f16s and self._stamp is not None and self._calib == "done" and not torch.cuda.is_current_stream_capturing():
            self._calib = "need"  # the entry was derived from the OLD weights' rows (as BackbonePlan.sync_weights)
        scale, shift = self.vfe._folded()
        with torch.no_grad():
            self._keep = (L.as_f32("pillar_plan", self.vfe.linear.weight.detach()), L.as_f32("pillar_plan", scale), L.as_f32("pillar_plan", shift))
        self._stamp = stamp

    def weights_changed(self):
        """True when a module tensor changed since the last sync (cheap: pointers and version counters)."""
        return self._stamp is not None and self._param_stamp() != self._stamp

    # ---- the frame
    def _check_frame(self, points, frame_offsets):
        pts = L.as_f32("pillar_plan", points)
        L.require_gpu("pillar_plan", pts)
        b = len(frame_offsets) - 1
        if pts.dim() != 2 or pts.shape[1] != self.C:
            raise RuntimeError(f"pillar_plan: points must be (N, {self.C}), got {tuple(pts.shape)}")
        if not 1 <= b <= self.max_batch or pts.shape[0] > self.max_points:
            raise RuntimeError(f"pillar_plan: {b} frame(s) of {pts.shape[0]} points exceed the plan's capacity ({self.max_batch} frame(s), "
                               f"{self.max_points} points)")
        return pts, b

    def _clear(self, persistent):
        """Bitmap to all ones, summary word to 0; persistent: the pixels list 1 names zeroed in the plan's planes."""
        h, w = self.map_shape
        prev, n = (self.coords[1], self.counts[1:2]) if persistent else (None, None)
        L.check(L.lib().v3d_pillar_planes_clear(L.ptr(prev), L.ptr(n), self.cap, self.max_batch, h, w, CHANNELS, L.ptr(self.planes[0]),
                                                L.ptr(self.planes[1]), L.ptr(self.bitmap), L.ptr(self.summary), L.stream_ptr()),
                "pillar_planes_clear")

    def _voxelize(self, pts, frame_offsets, b, k):
        """v3d_voxelize into the slots, the occupancy and coordinate list k (MAX_OCCUPANCY > 8: its wide path); no mean, no host read.
        Same coords, occupancy and slots as Preprocessor(cfg) on the same clouds."""
        L.check(L.lib().v3d_voxelize(L.ptr(pts), pts.shape[0], self.C, L.host_i32(frame_offsets), b, L.host_f32(self.cfg.VOXEL_SIZE),
                                     L.host_f32(self.cfg.GRID_BOUNDS), self.P, self.max_voxels, L.ptr(self.slots), L.ptr(self.coords[k]),
                                     L.ptr(self.occupancy), None, L.ptr(self.counts[k:k + 1]), L.ptr(self.vox_ws), self.vox_ws.numel(),
                                     L.stream_ptr()), "voxelize")

    def _encode_rows(self, k):
        """v3d_pillar_encode over the whole capacity into the plan's row buffer (rows beyond the device count hold whatever the
        buffers hold there -- readers go by the count)."""
        if self._rows is None:
            self._rows = torch.zeros((self.cap, CHANNELS), dtype=torch.float32, device=self.device)
        weight, scale, shift = self._keep
        L.check(L.lib().v3d_pillar_encode(L.ptr(self.slots), L.ptr(self.occupancy), L.ptr(self.coords[k]), self.cap, self.P, self.C,
                                          L.host_f32(self.vfe.geom), L.ptr(weight), CHANNELS, L.ptr(scale), L.ptr(shift), L.ptr(self._rows),
                                          L.stream_ptr()), "pillar_encode")
        return self._rows

    def _calibrate(self, k):
        rows = self._encode_rows(k)
        L.check(L.lib().v3d_act_scale_from_rows(L.ptr(rows), L.ptr(self.counts[k:k + 1]), self.cap, CHANNELS,
                                                int(self.__dict__.get("calib_headroom", CALIB_HEADROOM_BITS)), L.ptr(self.entry),
                                                L.ptr(L.scale_scratch(self.device)), L.stream_ptr()), "act_scale_from_rows")
        self._calib = "done"
        self.calibration_generation += 1

    def own_planes(self, batch_size):
        """The plan's PERSISTENT split planes as (B, H, W, 128) int16 views: a forward into them clears only the pixels the previous
        persistent frame wrote.  They alias plan memory: valid until the next persistent forward, and nobody else may write them."""
        return self._tag(self.planes[0][:int(batch_size)], self.planes[1][:int(batch_size)])

    def _tag(self, hi, lo):
        tag_planes(hi, self.bev_entry(), self.summary if self.f16s else None)
        return hi, lo

    def forward_split(self, points, frame_offsets, persistent=False):
        """points (sum N, C) float32 cuda (frames concatenated), frame_offsets: host ints (B + 1) -> the BEV map as the dense head's
        input: two NHWC planes (B, H, W, 128) hi / lo of the plan's arithmetic (int16 storage).  persistent: into the plan's own
        planes -- no fill of the map; what the captured graphs use (one plan per graph slot).  Nothing is synchronised."""
        self.sync_weights()
        pts, b = self._check_frame(points, frame_offsets)
        h, w = self.map_shape
        k = 1 if persistent else 0
        with L.device_guard(self.device):
            if persistent:
                hi, lo = self.own_planes(b)
            else:
                both = torch.zeros((2, b, h, w, CHANNELS), dtype=torch.int16, device=self.device)  # (one fill clears both planes)
                hi, lo = self._tag(both[0], both[1])
            self._clear(persistent)  # (reads list 1 BEFORE the voxelizer overwrites it)
            self._voxelize(pts, frame_offsets, b, k)
            if self._calib == "need" and not torch.cuda.is_current_stream_capturing():
                self._calibrate(k)
            weight, scale, shift = self._keep
            L.check(L.lib().v3d_pillar_encode_planes(L.ptr(self.slots), L.ptr(self.occupancy), L.ptr(self.coords[k]), L.ptr(self.counts[k:k + 1]),
                                                     self.cap, self.P, self.C, L.host_f32(self.vfe.geom), L.ptr(weight), CHANNELS,
                                                     L.ptr(scale), L.ptr(shift), b, h, w, L.PRECISIONS[self.precision],
                                                     L.ptr(self.entry) if self.f16s else None, L.ptr(self.summary) if self.f16s else None,
                                                     L.ptr(hi), L.ptr(lo), L.ptr(self.bitmap), L.stream_ptr()), "pillar_encode_planes")
        return hi, lo

    def forward(self, points, frame_offsets):
        """-> the BEV map (B, 128, H, W) float32, bit for bit PillarFeatureNet's on the same clouds.  Through the EXISTING encode
        (v3d_pillar_encode over the capacity) plus a scatter of the counted rows -- not through the split planes, whose hi + lo would
        round the bf16x3 map to 16 bits.  Device-side torch ops behind the kernel, no host read; not a hot path."""
        self.sync_weights()
        pts, b = self._check_frame(points, frame_offsets)
        h, w = self.map_shape
        with L.device_guard(self.device), torch.no_grad():
            self._voxelize(pts, frame_offsets, b, 0)
            rows, co = self._encode_rows(0), self.coords[0].long()
            live = torch.arange(self.cap, device=self.device) < self.counts[0]
            pix = (co[:, 0] * h + co[:, 2]) * w + co[:, 3]
            canvas = torch.zeros((b * h * w + 1, CHANNELS), dtype=torch.float32, device=self.device)  # (the last row takes the rest)
            canvas.index_copy_(0, torch.where(live, pix, b * h * w).clamp_(0, b * h * w), rows)
            return canvas[:-1].view(b, h, w, CHANNELS).permute(0, 3, 1, 2).contiguous()

    def voxels(self, persistent=False):
        """(slots (cap, P, C), occupancy (cap), coordinates (cap, 4), count (1,) device int32) of the last forward of that kind.
        Views of plan memory: valid until the next forward."""
        k = 1 if persistent else 0
        return self.slots, self.occupancy, self.coords[k], self.counts[k:k + 1]

    def bev_occupancy(self, batch_size):
        """(B * H, ceil(W / 32)) int32 view of the inverted occupancy bitmap (0 = occupied) of the LAST forward_split: what
        DenseHeadPlan.forward(occ=...) takes.  Aliases plan memory: valid until the next forward_split."""
        return self.bitmap[:int(batch_size) * self.map_shape[0]]

    def overflow_any(self):
        """(1,) int32 device view of the frame's summary word: 0, or 2 when an f16s tensor of the frame -- the planes, or a layer of
        the dense head run with this word as its range flag -- left its calibrated range."""
        return self.summary

    def check_overflow(self, ignore_range=False):
        """Blocking read of the summary word: 2 raises RangeOverflow (recalibrate() and run the frame again)."""
        if int(self.summary.item()) == 2 and not ignore_range:
            raise RangeOverflow("pillar plan (f16s): a tensor exceeded its calibrated range; recalibrate() and run the frame again")

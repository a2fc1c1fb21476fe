"""VectorPool aggregation (PV-RCNN++, arXiv 2102.00463), opt-in through `cfg.VECTORPOOL.ENABLED`: in place of multi-scale set
abstraction (`PV_RCNN.pnets`, `RoiGridPool.pnet`) the space around a query is cut into sub-voxels, the three nearest support points of
every sub-voxel centre are interpolated into one position-sensitive row, and every sub-voxel has a linear layer of its own.  Upstream
has no statement of it; the definition is this repository's, restated in numpy float64 in tests/vector_pool_ref.py:

  reduced       fr[n, j] = sum_m feat[n, m * Cr + j], m ascending (Cr = REDUCED divides the channel count), once per support row.
  centres       group with VOXELS (vx, vy, vz), radius R: sub-voxel v = (i * vy + j) * vz + k has off_v = (((2 i + 1) / vx - 1) R,
                ((2 j + 1) / vy - 1) R, ((2 k + 1) / vz - 1) R) (double, rounded once to float32) and the centre c_v = q + off_v (float32).
  neighbours    rows of the query's own frame with d^2 = (dx dx + dy dy) + dz dz < R^2 (float32, strict), the three smallest in
                ascending (d^2, row index) order; a row whose coordinates are bit-equal to those of a chosen one is passed over
                (SparseCNNBase.pad_batch tops frames up with resampled rows).  idx (-1: missing), u_k = 1 / (sqrt(d^2_k) + 1e-8),
                w_k = u_k / sum u over the rows found, 0 for the missing ones.
  sub-voxel row [sum_k w_k fr[idx_k] | c_v - p_1 | c_v - p_2 | c_v - p_3] (Cr + 9 columns; a missing neighbour's columns are zeros).
  local layers  sub-voxel v multiplies its row with its own (Cr + 9, LOCAL) weight, no bias; BatchNorm (eps 1e-3) over the nv * LOCAL
                concatenated channels, ReLU (an empty sub-voxel is still moved by the BatchNorm shift).
  tail          per group MLP([nv * LOCAL, *POST]) (Linear + BatchNorm + ReLU), groups concatenated on channels, MLP([sum POST[-1],
                *MSG_POST]) -> (B, MSG_POST[-1], M).

Inference (CUDA, float32, eval, no autograd) runs v3d_vector_pool_reduce once, per group v3d_vector_pool_query and
v3d_vector_pool_embed (csrc/vector_pool.hip), and the tail on v3d_linear_rows with the BatchNorms folded in.  Under autograd the
native query still gives idx / w (constants: coordinates carry no gradient) and the gather, the interpolation, the local layers and
the MLPs are torch operations, differentiable in the features and the parameters.  CPU tensors and sizes beyond the kernels' limits
take `query_torch`, the search in torch chunked over the queries."""
import torch
from torch import nn

from ..stamp import cached
from .layers import MLP

VECTORPOOL_DEFAULTS = dict(
    ENABLED=False,
    PSA=dict(REDUCED=[1, 4, 16, 32, 32], LOCAL=32, MSG_POST=[[32], [32], [64], [128], [128]],
             GROUPS=[dict(VOXELS=[2, 2, 2], RADIUS_SCALE=0.5, POST=[32, 32]), dict(VOXELS=[3, 3, 3], RADIUS_SCALE=1.0, POST=[32, 32])]),
    GRIDPOOL=dict(REDUCED=32, LOCAL=32, MSG_POST=[192],
                  GROUPS=[dict(VOXELS=[3, 3, 3], RADIUS=0.8, POST=[64, 64]), dict(VOXELS=[3, 3, 3], RADIUS=1.6, POST=[64, 64])]))
BN_EPS = 1e-3
# limits of csrc/vector_pool.hip: beyond them the torch statements run
MAX_AXIS, MAX_B, MAX_N, MAX_BN, MAX_CENTRES, MAX_CR, LOCAL_WIDTHS = 3, 64, 1 << 20, 1 << 24, 1 << 22, 32, (16, 32)
QUERY_TORCH_BYTES = 128 << 20  # the distances `query_torch` holds at a time


def vectorpool_config(cfg):
    """-> the keys of cfg.VECTORPOOL over their defaults (a config written before the key existed means "disabled")."""
    given = cfg.get("VECTORPOOL") or {}
    out = dict(ENABLED=bool(given.get("ENABLED", False)))
    for part in ("PSA", "GRIDPOOL"):
        out[part] = dict(VECTORPOOL_DEFAULTS[part])
        out[part].update(given.get(part) or {})
    return out


def subvoxel_offsets(voxels, radius):
    """-> (nv, 3) float32: the centre offsets of a group, computed in double and rounded once."""
    vx, vy, vz = (int(v) for v in voxels)
    r = float(radius)
    rows = [[((2 * i + 1) / vx - 1.0) * r, ((2 * j + 1) / vy - 1.0) * r, ((2 * k + 1) / vz - 1.0) * r]
            for i in range(vx) for j in range(vy) for k in range(vz)]
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32)


def _query_limits_ok(b, n, m, voxels):
    nv = voxels[0] * voxels[1] * voxels[2]
    return max(voxels) <= MAX_AXIS and b <= MAX_B and n <= MAX_N and b * n <= MAX_BN and b * m * nv <= MAX_CENTRES


def vector_pool_query(xyz, new_xyz, voxels, radius):
    """The native search (v3d_vector_pool_query): xyz (B, N, 3), new_xyz (B, M, 3) float32 on the GPU -> idx (B, M, nv, 3) int32
    frame-local rows (-1: missing), w (B, M, nv, 3) float32."""
    from .. import _lib as L
    L.require_gpu("vector_pool_query", xyz, new_xyz)
    p, q = L.as_f32("vector_pool_query", xyz), L.as_f32("vector_pool_query", new_xyz)
    (b, n, _), m = p.shape, q.shape[1]
    vx, vy, vz = (int(v) for v in voxels)
    nv = vx * vy * vz
    idx = torch.empty((b, m, nv, 3), dtype=torch.int32, device=p.device)
    w = torch.empty((b, m, nv, 3), dtype=torch.float32, device=p.device)
    ws = L.workspace(max(int(L.lib().v3d_vector_pool_query_workspace(b, n)), 16), p.device)
    with L.device_guard(p.device):
        L.check(L.lib().v3d_vector_pool_query(L.ptr(p), L.ptr(q), b, n, m, vx, vy, vz, float(radius), L.ptr(idx), L.ptr(w), L.ptr(ws),
                                              ws.numel(), L.stream_ptr()), "vector_pool_query")
    return idx, w


def vector_pool_reduce(features_pm, reduced):
    """The native reduction (v3d_vector_pool_reduce): (B, N, C) float32 with unit channel stride and frames back to back ->
    (B, N, reduced)."""
    from .. import _lib as L
    L.require_gpu("vector_pool_reduce", features_pm)
    b, n, c = features_pm.shape
    f = features_pm
    if f.dtype != torch.float32 or f.stride(2) != 1 or (b > 1 and f.stride(0) != n * f.stride(1)) or c % int(reduced):
        raise RuntimeError("vector_pool_reduce: float32 (B, N, C) with unit channel stride, frames back to back, REDUCED dividing C")
    out = torch.empty((b, n, int(reduced)), dtype=torch.float32, device=f.device)
    ldf = f.stride(1) if b * n > 1 else max(f.stride(1), c)
    with L.device_guard(f.device):
        L.check(L.lib().v3d_vector_pool_reduce(L.ptr(f), ldf, b * n, c, int(reduced), L.ptr(out), L.stream_ptr()), "vector_pool_reduce")
    return out


def vector_pool_embed(fr, xyz, new_xyz, idx, w, voxels, radius, w_local, shift, out):
    """The native embedding (v3d_vector_pool_embed): fr (B, N, Cr) contiguous, idx / w from the query, w_local (nv, Cr + 9, CL) and
    shift (nv * CL) with the BatchNorm folded in; `out` (B * M, nv * CL) a view with unit column stride, written in place."""
    from .. import _lib as L
    L.require_gpu("vector_pool_embed", fr, xyz, new_xyz, idx, w, w_local, shift, out)
    b, n, cr = fr.shape
    m = new_xyz.shape[1]
    vx, vy, vz = (int(v) for v in voxels)
    nv = vx * vy * vz
    cl = w_local.shape[2]
    if (tuple(w_local.shape) != (nv, cr + 9, cl) or shift.numel() != nv * cl or tuple(idx.shape) != (b, m, nv, 3) or tuple(w.shape) != (b, m, nv, 3)
            or idx.dtype != torch.int32 or not idx.is_contiguous() or not w.is_contiguous() or not fr.is_contiguous() or out.dim() != 2
            or tuple(out.shape) != (b * m, nv * cl) or out.stride(1) != 1 or out.dtype != torch.float32):
        raise RuntimeError("vector_pool_embed: mismatched shapes, or `out` is not a float32 (B * M, nv * CL) view with unit column stride")
    ldo = out.stride(0) if b * m > 1 else max(out.stride(0), nv * cl)
    with L.device_guard(out.device):
        L.check(L.lib().v3d_vector_pool_embed(L.ptr(L.as_f32("vector_pool_embed", fr)), cr, L.ptr(L.as_f32("vector_pool_embed", xyz)),
                                              L.ptr(L.as_f32("vector_pool_embed", new_xyz)), L.ptr(idx), L.ptr(L.as_f32("vector_pool_embed", w)),
                                              b, n, m, vx, vy, vz, float(radius), cr, cl, L.ptr(L.as_f32("vector_pool_embed", w_local)),
                                              L.ptr(L.as_f32("vector_pool_embed", shift)), L.ptr(out), ldo, L.stream_ptr()), "vector_pool_embed")
    return out


def canonical_rows(xyz):
    """xyz (B, N, 3) float32 -> (B, N) bool: the row is the lowest-indexed one among those with its coordinates bit for bit."""
    b, n, _ = xyz.shape
    keep = torch.zeros((b, n), dtype=torch.bool, device=xyz.device)
    for f in range(b):
        bits = xyz[f].contiguous().view(torch.int32)
        _, inverse = torch.unique(bits, dim=0, return_inverse=True)
        first = torch.full((int(inverse.max()) + 1 if n else 0,), n, dtype=torch.long, device=xyz.device)
        first.scatter_reduce_(0, inverse, torch.arange(n, device=xyz.device), "amin")
        keep[f] = first[inverse] == torch.arange(n, device=xyz.device)
    return keep


def query_torch(xyz, new_xyz, voxels, radius):
    """The search in torch statements (any device, float32): -> idx (B, M, nv, 3) int64 (-1: missing), w (B, M, nv, 3).  Chunked over
    the queries so that no more than QUERY_TORCH_BYTES of distances exist at a time."""
    b, n, _ = xyz.shape
    m = new_xyz.shape[1]
    off = subvoxel_offsets(voxels, radius).to(xyz.device)
    nv = off.shape[0]
    idx = torch.full((b, m, nv, 3), -1, dtype=torch.long, device=xyz.device)
    d2 = torch.full((b, m, nv, 3), float("inf"), dtype=torch.float32, device=xyz.device)
    if n > 0 and m > 0:
        r2 = torch.tensor(float(radius), dtype=torch.float32, device=xyz.device) ** 2
        skip = ~canonical_rows(xyz)  # (a duplicate never takes a slot: its lowest-indexed twin stands for it)
        step = max(1, QUERY_TORCH_BYTES // (4 * nv * n))
        inf = torch.tensor(float("inf"), dtype=torch.float32, device=xyz.device)
        for f in range(b):
            p = xyz[f]
            for m0 in range(0, m, step):
                c = (new_xyz[f, m0:m0 + step, None, :] + off[None]).reshape(-1, 1, 3)  # (chunk * nv, 1, 3)
                dx, dy, dz = p[None, :, 0] - c[..., 0], p[None, :, 1] - c[..., 1], p[None, :, 2] - c[..., 2]
                d = (dx * dx + dy * dy) + dz * dz
                d = torch.where((d < r2) & ~skip[f][None], d, inf)
                for k in range(3):  # (min returns the first of equal values: the index tie-break)
                    val, arg = d.min(dim=1)
                    found = val < inf
                    idx[f, m0:m0 + step, :, k] = torch.where(found, arg, torch.full_like(arg, -1)).reshape(-1, nv)
                    d2[f, m0:m0 + step, :, k] = val.reshape(-1, nv)
                    d.scatter_(1, arg[:, None], float("inf"))
    found = idx >= 0
    u = torch.where(found, 1.0 / (torch.sqrt(torch.where(found, d2, torch.ones_like(d2))) + 1e-8), torch.zeros_like(d2))
    total = (u[..., 0] + u[..., 1]) + u[..., 2]
    w = torch.where(found, u / torch.where(total > 0, total, torch.ones_like(total))[..., None], torch.zeros_like(u))
    return idx, w


class VectorPoolGroup(nn.Module):
    """One group: its sub-voxel layout, the per-sub-voxel weights, their BatchNorm and the group's MLP."""

    def __init__(self, reduced, local, voxels, radius, post):
        super().__init__()
        self.voxels = tuple(int(v) for v in voxels)
        self.radius = float(radius)
        if len(self.voxels) != 3 or min(self.voxels) < 1 or not self.radius > 0:
            raise ValueError("VECTORPOOL: a group needs VOXELS [vx, vy, vz] >= 1 and a radius > 0")
        self.nv = self.voxels[0] * self.voxels[1] * self.voxels[2]
        self.reduced, self.local = int(reduced), int(local)
        self.local_weight = nn.Parameter(torch.empty(self.nv, self.reduced + 9, self.local))
        nn.init.normal_(self.local_weight, std=0.01)
        self.local_bn = nn.BatchNorm1d(self.nv * self.local, eps=BN_EPS)
        self.post = MLP([self.nv * self.local, *[int(v) for v in post]], bias=False, bn=True, relu=True)
        self.register_buffer("offsets", subvoxel_offsets(self.voxels, self.radius), persistent=False)

    def out_width(self):
        return [m for m in self.post if isinstance(m, nn.Linear)][-1].out_features


def _set_bn_eps(module):
    for m in module.modules():
        if isinstance(m, nn.BatchNorm1d):
            m.eps = BN_EPS


def _fold(linear_weight_t, bn):
    """(K, Nout) weight (the nn.Linear weight transposed) and an eval BatchNorm1d -> (weight * scale, shift)."""
    scale = bn.weight.float() * torch.rsqrt(bn.running_var.float() + bn.eps)
    return linear_weight_t.float() * scale[None, :], bn.bias.float() - bn.running_mean.float() * scale


class VectorPoolAggregationMSG(nn.Module):

    native = True  # False: the torch statements everywhere, the search included (the cross-check of the tests)

    def __init__(self, c_in, reduced, local, groups, msg_post):
        """groups: [dict(VOXELS=[vx, vy, vz], RADIUS=r, POST=[...])]; msg_post: widths behind the concatenated groups."""
        super().__init__()
        self.c_in, self.reduced, self.local = int(c_in), int(reduced), int(local)
        if self.reduced < 1 or self.c_in % self.reduced:
            raise ValueError(f"VECTORPOOL: REDUCED = {self.reduced} must divide the source's channel count {self.c_in}")
        if not groups or not msg_post:
            raise ValueError("VECTORPOOL: at least one group and one MSG_POST width")
        self.groups = nn.ModuleList(VectorPoolGroup(self.reduced, self.local, g["VOXELS"], g["RADIUS"], g["POST"]) for g in groups)
        self.msg_post = MLP([sum(g.out_width() for g in self.groups), *[int(v) for v in msg_post]], bias=False, bn=True, relu=True)
        _set_bn_eps(self)

    # ---- the call surface the two sites use
    def out_channels(self):
        return [[m for m in self.msg_post if isinstance(m, nn.Linear)][-1].out_features]

    def max_radius(self):
        return max(g.radius for g in self.groups)

    def _fusable(self, features):
        """The fused single-matrix paths (PV_RCNN._point_features_fused, RoiGridPool.forward) are written around set-abstraction
        internals: this module is never folded into them."""
        return False

    # ---- the torch statements
    def reduce_torch(self, features_pm):
        b, n, c = features_pm.shape
        parts = features_pm.reshape(b, n, c // self.reduced, self.reduced)
        fr = parts[:, :, 0]
        for k in range(1, c // self.reduced):
            fr = fr + parts[:, :, k]
        return fr

    def query(self, xyz, new_xyz, group):
        """idx (B, M, nv, 3) int64, w (B, M, nv, 3) of one group: the native search where it applies, else `query_torch`."""
        b, n, _ = xyz.shape
        if (self.native and xyz.is_cuda and new_xyz.is_cuda and xyz.dtype == torch.float32 and new_xyz.dtype == torch.float32
                and _query_limits_ok(b, n, new_xyz.shape[1], group.voxels)):
            idx, w = vector_pool_query(xyz.detach(), new_xyz.detach(), group.voxels, group.radius)
            return idx.long(), w
        return query_torch(xyz.detach().float(), new_xyz.detach().float(), group.voxels, group.radius)

    def rows_torch(self, fr, xyz, new_xyz, idx, w, group):
        """-> (B, M, nv, Cr + 9): the sub-voxel rows, differentiable in fr."""
        b, m = new_xyz.shape[:2]
        found = idx >= 0
        safe = idx.clamp(min=0)
        frame = torch.arange(b, device=fr.device).view(b, 1, 1, 1)
        wk = torch.where(found, w, torch.zeros_like(w)).to(fr.dtype)
        g = fr[frame, safe] * wk[..., None]  # (B, M, nv, 3, Cr)
        interp = (g[..., 0, :] + g[..., 1, :]) + g[..., 2, :]
        centre = (new_xyz[:, :, None, :] + group.offsets.to(new_xyz.dtype)[None, None]).to(fr.dtype)  # (the sum in the coordinates' own type)
        rel = (centre[:, :, :, None, :] - xyz.to(fr.dtype)[frame, safe]) * found[..., None].to(fr.dtype)  # (B, M, nv, 3, 3)
        return torch.cat([interp, rel.reshape(b, m, group.nv, 9)], -1)

    def embed_torch(self, fr, xyz, new_xyz, idx, w, group):
        """-> (B * M, nv * CL): rows through the sub-voxels' own layers, BatchNorm, ReLU."""
        rows = self.rows_torch(fr, xyz, new_xyz, idx, w, group)
        y = torch.einsum("bmvk,vkc->bmvc", rows, group.local_weight.to(rows.dtype)).reshape(-1, group.nv * group.local)
        return torch.relu(group.local_bn(y))

    def forward_torch(self, xyz, features_pm, new_xyz):
        """xyz (B, N, 3), features_pm (B, N, C), new_xyz (B, M, 3) -> (B, C_out, M), op by op (under autograd: differentiable in the
        features and the parameters; the coordinates are constants)."""
        b, m = new_xyz.shape[:2]
        fr = self.reduce_torch(features_pm)
        blocks = []
        for group in self.groups:
            idx, w = self.query(xyz, new_xyz, group)
            blocks.append(nn.Sequential.forward(group.post, self.embed_torch(fr, xyz.detach(), new_xyz.detach(), idx, w, group)))
        out = nn.Sequential.forward(self.msg_post, torch.cat(blocks, -1))
        return out.reshape(b, m, -1).transpose(1, 2)

    # ---- the native path
    def native_ok(self, xyz, features_pm, new_xyz):
        if not self.native or self.training or torch.is_grad_enabled():
            return False
        if not all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 for t in (xyz, features_pm, new_xyz)):
            return False
        b, n, _ = xyz.shape
        m = new_xyz.shape[1]
        if b * n == 0 or b * m == 0 or self.reduced > MAX_CR or self.local not in LOCAL_WIDTHS or features_pm.shape[2] != self.c_in:
            return False
        return all(_query_limits_ok(b, n, m, g.voxels) for g in self.groups)

    def _folded(self):
        """The parameters as the kernels take them, eval BatchNorms folded in, cached until a parameter or running statistic changes:
        per group (w_local (nv, Cr + 9, CL), shift (nv * CL), [(W (K, Nout padded to 16), bias, Nout)]), then the MSG_POST layers."""
        tensors = (t for mod in self.modules() for t in list(mod._parameters.values()) + list(mod._buffers.values()))
        return cached(self, "_fold_cache", tensors, self._fold_all)

    def _fold_all(self):
        def layers(mlp, k_in):
            lins = [mod for mod in mlp if isinstance(mod, nn.Linear)]
            bns = [mod for mod in mlp if isinstance(mod, nn.BatchNorm1d)]
            out = []
            for lin, bn in zip(lins, bns):
                wt, shift = _fold(lin.weight.t(), bn)
                npad = -(-lin.out_features // 16) * 16
                full = wt.new_zeros((k_in, npad))  # (a padded predecessor hands over zero columns: zero rows here)
                full[:wt.shape[0], :lin.out_features] = wt
                bias = wt.new_zeros(npad)
                bias[:lin.out_features] = shift
                out.append((full.contiguous(), bias, lin.out_features))
                k_in = npad
            return out

        with torch.no_grad():
            groups = []
            for g in self.groups:
                scale = g.local_bn.weight.float() * torch.rsqrt(g.local_bn.running_var.float() + g.local_bn.eps)
                shift = (g.local_bn.bias.float() - g.local_bn.running_mean.float() * scale).contiguous()
                w_local = (g.local_weight.float() * scale.view(g.nv, 1, g.local)).contiguous()
                groups.append((w_local, shift, layers(g.post, g.nv * g.local)))
            cat_width = -(-sum(g.out_width() for g in self.groups) // 4) * 4
            return groups, layers(self.msg_post, cat_width), cat_width

    def forward_native(self, xyz, features_pm, new_xyz):
        """`native_ok` inputs -> (B, C_out, M), a view of point-major rows.  Only enqueues: no host read."""
        from ..pointnet2.pointnet2_utils import linear_rows
        b, m = new_xyz.shape[:2]
        n = xyz.shape[1]
        xyz, new_xyz = xyz.contiguous(), new_xyz.contiguous()
        f = features_pm
        if f.stride(2) != 1 or (b > 1 and f.stride(0) != n * f.stride(1)):
            f = f.contiguous()
        fr = vector_pool_reduce(f, self.reduced)
        groups, msg_layers, cat_width = self._folded()
        widths = [g.out_width() for g in self.groups]
        alloc = torch.zeros if cat_width != sum(widths) else torch.empty
        cat = alloc((b * m, cat_width), dtype=torch.float32, device=xyz.device)
        col = 0
        for g, (w_local, shift, post), width in zip(self.groups, groups, widths):
            idx, w = vector_pool_query(xyz, new_xyz, g.voxels, g.radius)
            a = torch.empty((b * m, g.nv * g.local), dtype=torch.float32, device=xyz.device)
            vector_pool_embed(fr, xyz, new_xyz, idx, w, g.voxels, g.radius, w_local, shift, a)
            for li, (wt, bias, nout) in enumerate(post):
                if li == len(post) - 1:
                    linear_rows(a, wt, bias, True, out=cat[:, col:col + width], n_store=nout)
                else:
                    a = linear_rows(a, wt, bias, True)
            col += width
        a = cat
        for li, (wt, bias, nout) in enumerate(msg_layers):
            a = linear_rows(a, wt, bias, True, n_store=nout if li == len(msg_layers) - 1 else None)
        return a.view(b, m, -1).transpose(1, 2)

    def forward(self, xyz, features=None, new_xyz=None, features_pm=None):
        """xyz (B, N, 3), features (B, C, N) or features_pm (B, N, C), new_xyz (B, M, 3) -> (new_xyz, (B, C_out, M)): the call
        surface of PointnetSAModuleMSG."""
        if new_xyz is None:
            raise RuntimeError("VectorPoolAggregationMSG: new_xyz is required (the module does not sample its queries)")
        pm = features_pm if features_pm is not None else features.transpose(1, 2)
        if self.native_ok(xyz, pm, new_xyz):
            return new_xyz, self.forward_native(xyz, pm, new_xyz)
        return new_xyz, self.forward_torch(xyz, pm, new_xyz)


# ---- the two sites
def _groups(spec, radius_of):
    return [dict(VOXELS=g["VOXELS"], RADIUS=radius_of(g), POST=g["POST"]) for g in spec["GROUPS"]]


def build_keypoint_modules(cfg):
    """-> nn.Sequential of one VectorPoolAggregationMSG per feature source of cfg.PSA (raw points, then the CNN levels); a group's
    radius is RADIUS_SCALE times the source's larger cfg.PSA.RADII entry (or its own RADIUS)."""
    spec = vectorpool_config(cfg)["PSA"]
    channels = [int(mlps[0][0]) for mlps in cfg.PSA.MLPS]
    reduced, posts = list(spec["REDUCED"]), list(spec["MSG_POST"])
    if not (len(reduced) == len(posts) == len(channels) == len(cfg.PSA.RADII)):
        raise ValueError(f"VECTORPOOL.PSA: REDUCED and MSG_POST need one entry per feature source ({len(channels)})")
    mods = []
    for c, cr, post, radii in zip(channels, reduced, posts, cfg.PSA.RADII):
        big = max(abs(float(r)) for r in radii)
        mods.append(VectorPoolAggregationMSG(c, cr, spec["LOCAL"], _groups(spec, lambda g: g["RADIUS"] if "RADIUS" in g else float(g["RADIUS_SCALE"]) * big),
                                             post))
    return nn.Sequential(*mods)


def build_gridpool_module(cfg):
    """-> the VectorPoolAggregationMSG of RoI-grid pooling over the keypoint features (the keypoint modules' widths + the BEV map)."""
    vp = vectorpool_config(cfg)
    spec = vp["GRIDPOOL"]
    c_in = sum(int(p[-1]) for p in vp["PSA"]["MSG_POST"]) + int(cfg.PROPOSAL.C_IN)
    post = [int(v) for v in spec["MSG_POST"]]
    need = int(cfg.GRIDPOOL.NUM_GRIDPOINTS) * post[-1]
    if need != int(cfg.GRIDPOOL.MLPS_REDUCTION[0]):
        raise ValueError(f"VECTORPOOL.GRIDPOOL: NUM_GRIDPOINTS * MSG_POST[-1] = {need} must equal GRIDPOOL.MLPS_REDUCTION[0] = "
                         f"{int(cfg.GRIDPOOL.MLPS_REDUCTION[0])}")
    return VectorPoolAggregationMSG(c_in, spec["REDUCED"], spec["LOCAL"], _groups(spec, lambda g: g["RADIUS"]), post)

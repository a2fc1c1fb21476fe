"""The rulebook builders (csrc/rulebook.hip, csrc/rb_device.h) and the transposed table against tests/geometry_ref.py, bit for bit, at
the kernel geometries, chunk edges, capacities and key ranges the KITTI-shaped tests do not reach.

  test_subm_kernels                     (3,3,3), (3,1,1), (1,3,3), (3,3,5), (1,1,1), (5,5,1): the generic look-up and its centre rule
  test_subm_refuses_an_even_kernel
  test_subm_offsets_per_thread_switch   40 959 / 40 960 rows: one and nine offsets per thread
  test_strided_geometries               eight (kernel, stride, pad) on an odd grid; out_shape, sites, table, transposed table
  test_ticket_scan_chunk_edges          ticket counts around the 2 048-ticket chunk; 258 chunks (second trip of the predecessor wait)
  test_live_count_below_capacity        *n < cap at both entry points
  test_clipped_output                   cap_out below / at the true count: flag, count, surviving columns, guard rows
  test_rows_without_a_key               batch index 64 and -1
  test_keys_near_the_limit              a grid just under 2^34 cells with batch index 63
  test_grid_of_2_to_the_34_is_refused
"""
import functools

import numpy as np
import pytest
import torch

import geometry_cases as cases
import geometry_ref as ref
from gpu_util import dev

pytestmark = pytest.mark.gpu
eq = np.testing.assert_array_equal
EINVAL, EUNSUPPORTED = -1, -3  # include/vision3d_hip.h
FILL = -77                     # what the raw calls' output buffers hold before the call
GUARD = 64                     # rows / words allocated behind an output buffer


@functools.lru_cache(maxsize=None)
def strided_ref(case, geom, cap_out=None):
    c = cases.build(case)
    n = c.get("n_live", len(c["coords"]))
    return ref.sparse_rulebook(c["coords"], n, c["shape"], *cases.STRIDED_GEOMETRIES[geom], cap_out=cap_out)


def tensor_of(c):
    from vision3d_amd.spconv import SparseConvTensor
    co = np.array(c["coords"])  # (the cases' arrays are read-only)
    return SparseConvTensor(torch.zeros((len(co), 1), dtype=torch.float32).cuda(), dev(co, torch.int32), c["shape"], c["batch"])


def raw_subm(coords, n, shape, ks):
    """v3d_rulebook_subm as build_subm_rulebook calls it, with the capacity (len(coords)) and the live count apart -> rc, nbr (K, cap)"""
    from vision3d_amd import _lib as L
    cap, k = len(coords), ks[0] * ks[1] * ks[2]
    co, n_dev = dev(np.array(coords), torch.int32), torch.tensor([n], dtype=torch.int32).cuda()
    nbr = torch.full((k, cap), FILL, dtype=torch.int32).cuda()
    lib = L.lib()
    ws = L.workspace(lib.v3d_rulebook_workspace(cap, cap, k), co.device)
    rc = lib.v3d_rulebook_subm(L.ptr(co), L.ptr(n_dev), cap, L.host_i32(shape), L.host_i32(ks), L.ptr(nbr), L.ptr(ws), ws.numel(),
                               L.stream_ptr())
    torch.cuda.synchronize()
    return rc, nbr.cpu().numpy()


def raw_sparse(coords, n, shape, ks, stride, pad, cap_out):
    """v3d_rulebook_sparse as build_sparse_rulebook calls it, with cap_in = len(coords), the live count and cap_out chosen freely
    -> rc, n_out, overflow, coords_out (cap_out + GUARD, 4), nbr (K, cap_out), the GUARD words behind nbr"""
    from vision3d_amd import _lib as L
    cap_in, k = len(coords), ks[0] * ks[1] * ks[2]
    co, n_dev = dev(np.array(coords), torch.int32), torch.tensor([n], dtype=torch.int32).cuda()
    coords_out = torch.full((cap_out + GUARD, 4), FILL, dtype=torch.int32).cuda()
    nbr = torch.full((k * cap_out + GUARD,), FILL, dtype=torch.int32).cuda()
    n_out = torch.zeros((1,), dtype=torch.int32).cuda()
    overflow = torch.zeros((1,), dtype=torch.int32).cuda()
    lib = L.lib()
    ws = L.workspace(lib.v3d_rulebook_workspace(cap_in, cap_out, k), co.device)
    rc = lib.v3d_rulebook_sparse(L.ptr(co), L.ptr(n_dev), cap_in, L.host_i32(shape), L.host_i32(ks), L.host_i32(stride), L.host_i32(pad),
                                 L.ptr(coords_out), L.ptr(n_out), cap_out, L.ptr(nbr), L.ptr(overflow), L.ptr(ws), ws.numel(),
                                 L.stream_ptr())
    torch.cuda.synchronize()
    nbr = nbr.cpu().numpy()
    return rc, int(n_out.item()), int(overflow.item()), coords_out.cpu().numpy(), nbr[:k * cap_out].reshape(k, cap_out), nbr[k * cap_out:]


def wrapper_cap_out(n, shape, batch, ks, stride, pad):
    """the capacity build_sparse_rulebook gives the output"""
    out_shape = [(shape[j] + 2 * pad[j] - ks[j]) // stride[j] + 1 for j in range(3)]
    fan = int(np.prod([-(-ks[j] // stride[j]) for j in range(3)]))
    return max(1, min(n * fan, batch * out_shape[0] * out_shape[1] * out_shape[2]))


def check_strided(c, geom, want):
    """build_sparse_rulebook + transpose_rulebook on the case against the reference's (coords_out, nbr, out_shape, overflow)"""
    from vision3d_amd.spconv.conv import build_sparse_rulebook
    from vision3d_amd.spconv.functional import transpose_rulebook
    co, nbr, out_shape, overflow = want
    assert not overflow
    x = tensor_of(c)
    rb = build_sparse_rulebook(x, *cases.STRIDED_GEOMETRIES[geom])
    assert rb.out_shape == out_shape and rb.n == len(co) == int(rb.n_dev.item())
    eq(rb.out_indices.cpu().numpy(), co)
    table = rb.nbr.cpu().numpy()
    eq(table[:, :rb.n], nbr)
    eq(table[:, rb.n:], -1)
    n_in = len(c["coords"])
    rt = transpose_rulebook(rb, n_in, x.features.device)
    got_t = rt.nbr.cpu().numpy()
    assert got_t.shape == (nbr.shape[0], n_in)
    eq(got_t, ref.transpose(nbr, len(co), n_in))
    # the table's definition, entry by entry, on the device's own table: nbrT[k][i] == o iff nbr[k][o] == i, -1 elsewhere
    k, o = np.nonzero(table[:, :rb.n] >= 0)
    eq(got_t[k, table[k, o]], o)
    assert (got_t >= 0).sum() == len(o)


# ------------------------------------------------------------------------------------------------ submanifold
@pytest.mark.parametrize("ks", cases.SUBM_KERNELS, ids=lambda ks: "k%d%d%d" % tuple(ks))
def test_subm_kernels(ks):
    from vision3d_amd.spconv.conv import build_subm_rulebook
    c = cases.build("few_hundred")
    rb = build_subm_rulebook(tensor_of(c), ks)
    eq(rb.nbr.cpu().numpy(), ref.subm_rulebook(c["coords"], len(c["coords"]), c["shape"], ks))


def test_subm_refuses_an_even_kernel():
    c = cases.build("few_hundred")
    for ks in ([2, 3, 3], [3, 3, 2], [2, 2, 2]):
        rc, _ = raw_subm(c["coords"], len(c["coords"]), c["shape"], ks)
        assert rc == EINVAL, (ks, rc)


@pytest.mark.parametrize("name", ["kpt_40959", "kpt_40960"])
def test_subm_offsets_per_thread_switch(name):
    from vision3d_amd.spconv.conv import build_subm_rulebook
    c = cases.build(name)
    rb = build_subm_rulebook(tensor_of(c), [3, 3, 3])
    assert rb.cap == len(c["coords"])  # the switch is on the capacity
    eq(rb.nbr.cpu().numpy(), ref.subm_rulebook(c["coords"], len(c["coords"]), c["shape"], 3))


# ------------------------------------------------------------------------------------------------ strided
@pytest.mark.parametrize("geom", list(cases.STRIDED_GEOMETRIES))
def test_strided_geometries(geom):
    check_strided(cases.build("odd_grid"), geom, strided_ref("odd_grid", geom))


@pytest.mark.parametrize("case,geom,tickets", cases.CHUNK_RUNS, ids=["%s-%s" % r[:2] for r in cases.CHUNK_RUNS])
def test_ticket_scan_chunk_edges(case, geom, tickets):
    check_strided(cases.build(case), geom, strided_ref(case, geom))


def test_live_count_below_capacity():
    c = cases.build("padded")
    co, n, shape = c["coords"], c["n_live"], c["shape"]
    assert len(co) == n + cases.PAD_ROWS
    rc, nbr = raw_subm(co, n, shape, [3, 3, 3])
    assert rc == 0
    eq(nbr[:, :n], ref.subm_rulebook(co, n, shape, 3))
    eq(nbr[:, n:], FILL)  # columns behind the live count are nobody's
    ks, st, pd = cases.STRIDED_GEOMETRIES["k3s2p1"]
    want_co, want_nbr, _, _ = strided_ref("padded", "k3s2p1")
    cap_out = wrapper_cap_out(len(co), shape, c["batch"], ks, st, pd)
    rc, n_out, overflow, got_co, got_nbr, tail = raw_sparse(co, n, shape, ks, st, pd, cap_out)
    assert (rc, n_out, overflow) == (0, len(want_co), 0)
    eq(got_co[:n_out], want_co)
    eq(got_co[n_out:], FILL)
    eq(got_nbr[:, :n_out], want_nbr)
    eq(got_nbr[:, n_out:], -1)
    eq(tail, FILL)


@pytest.mark.parametrize("short", [0, 1, 257, "all_but_one"])
def test_clipped_output(short):
    """cap_out = T - short (T: the true output count, at most cap_in, so the output table never fills): the first cap_out outputs
    survive with their columns complete, nothing is written for the others, and the flag says so."""
    c = cases.build("odd_grid")
    ks, st, pd = cases.STRIDED_GEOMETRIES["k3s2p1"]
    full_co, full_nbr, _, _ = strided_ref("odd_grid", "k3s2p1")
    T = len(full_co)
    assert 258 < T <= len(c["coords"])
    cap_out = 1 if short == "all_but_one" else T - short
    want_co, want_nbr, _, want_overflow = strided_ref("odd_grid", "k3s2p1", cap_out)
    assert want_overflow == (cap_out < T) and len(want_co) == cap_out
    rc, n_out, overflow, got_co, got_nbr, tail = raw_sparse(c["coords"], len(c["coords"]), c["shape"], ks, st, pd, cap_out)
    assert (rc, n_out, overflow) == (0, cap_out, int(cap_out < T))
    eq(got_co[:cap_out], want_co)
    eq(got_co[:cap_out], full_co[:cap_out])
    eq(got_nbr, want_nbr)
    eq(got_nbr, full_nbr[:, :cap_out])
    eq(got_co[cap_out:], FILL)  # the guard rows behind coords_out
    eq(tail, FILL)              # and behind the table


def test_rows_without_a_key():
    c = cases.build("bad_batch")
    co, shape, bad = c["coords"], c["shape"], c["bad_rows"]
    assert set(co[bad, 0].tolist()) == {64, -1}
    rc, nbr = raw_subm(co, len(co), shape, [3, 3, 3])
    assert rc == 0
    eq(nbr, ref.subm_rulebook(co, len(co), shape, 3))
    ks, st, pd = cases.STRIDED_GEOMETRIES["k3s2p1"]
    want_co, want_nbr, _, want_overflow = ref.sparse_rulebook(co, len(co), shape, ks, st, pd)
    assert want_overflow and not np.isin(want_nbr, bad).any()
    rc, n_out, overflow, got_co, got_nbr, tail = raw_sparse(co, len(co), shape, ks, st, pd, wrapper_cap_out(len(co), shape, c["batch"], ks, st, pd))
    assert (rc, n_out, overflow) == (0, len(want_co), 1)
    eq(got_co[:n_out], want_co)
    eq(got_co[n_out:], FILL)
    eq(got_nbr[:, :n_out], want_nbr)
    eq(got_nbr[:, n_out:], -1)
    eq(tail, FILL)


# ------------------------------------------------------------------------------------------------ key range
def test_keys_near_the_limit():
    from vision3d_amd.spconv.conv import build_subm_rulebook
    c = cases.build("key_range")
    rb = build_subm_rulebook(tensor_of(c), [3, 3, 3])
    eq(rb.nbr.cpu().numpy(), ref.subm_rulebook(c["coords"], len(c["coords"]), c["shape"], 3))
    check_strided(c, "k3s2p1", strided_ref("key_range", "k3s2p1"))


def test_grid_of_2_to_the_34_is_refused():
    c = cases.build("key_range")
    co = c["coords"]
    rc, _ = raw_subm(co, len(co), cases.REFUSED_SHAPE, [3, 3, 3])
    assert rc == EUNSUPPORTED
    rc, n_out, _, got_co, _, _ = raw_sparse(co, len(co), cases.REFUSED_SHAPE, [1, 1, 1], [1, 1, 1], [0, 0, 0], len(co))
    assert rc == EUNSUPPORTED and n_out == 0
    eq(got_co, FILL)
    # the input grid passes, the OUTPUT grid of a padded 1x1x1 layer does not
    rc, _, _, _, _, _ = raw_sparse(co, len(co), cases.KEY_RANGE_SHAPE, [1, 1, 1], [1, 1, 1], [0, 0, 1], len(co))
    assert rc == EUNSUPPORTED

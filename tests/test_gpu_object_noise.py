"""GPU: per-object ground-truth noise (cfg.AUG.OBJECT_NOISE; csrc/object_noise.hip, ObjectNoiseAugmentation) against the float64
restatement tests/object_noise_ref.py and against the class's own torch statement, on the seeded cases of tests/object_noise_cases.py
(whose margins tests/test_host_object_noise.py asserts): chosen equal; boxes that stay bit-identical; moved boxes and moved points
within 4 float32 ulps of the float64 value.  Largest errors observed on the MI355X over the seven seeded cases:
0.50 ulp on a moved box, 1.25 ulp on a moved point (the tests print theirs)."""
import functools
import os

import numpy as np
import pytest
import torch

import object_noise_cases as K
import object_noise_ref as R
from vision3d_amd.core.config import second_car_cfg

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

LIMIT_CASES = [(129, 3, 300, 4, dict(seed=0)), (3, 257, 200, 4, dict(seed=0, pairs=1, stuck=1))]  # beyond the native limits


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def make_noise(T, rng=None):
    from vision3d_amd.dataset import ObjectNoiseAugmentation
    cfg = second_car_cfg()
    cfg.AUG.OBJECT_NOISE.NUM_TRY = T
    return ObjectNoiseAugmentation(cfg, rng)


@functools.lru_cache(maxsize=None)
def case(kind, index):
    """inputs and the float64 restatement of a seeded case (computed once, shared, never written to)."""
    n, T, N, C, kw = (K.GPU_CASES if kind == "gpu" else LIMIT_CASES)[index]
    inputs = K.make_case(n, T, N, C, **kw)
    return inputs, R.object_noise(*inputs)


def check_against_restatement(inputs, ref, out_p, out_b, chosen, what):
    from vision3d_amd.core.geometry import points_in_boxes_mask
    points, boxes, trans, rot = inputs
    assert ref["iou_margin"] >= 1e-4 and ref["face_margin"] >= 1e-4, "the case decides nothing for implementations in different arithmetic"
    out_p, out_b, chosen = out_p.cpu().numpy(), out_b.cpu().numpy(), chosen.cpu().numpy()
    assert out_p.dtype == np.float32 and out_b.dtype == np.float32 and out_p.shape == points.shape and out_b.shape == boxes.shape
    np.testing.assert_array_equal(chosen, ref["chosen"])
    stay = ref["chosen"] < 0
    np.testing.assert_array_equal(bits(out_b[stay]), bits(boxes[stay]))
    np.testing.assert_array_equal(bits(out_b[:, 3:6]), bits(boxes[:, 3:6]))
    ok, worst_box = R.within_ulps(out_b[~stay], ref["boxes"][~stay])
    print(f"[object_noise] {what}: moved boxes, largest error {worst_box:.2f} ulp")
    assert ok.all()
    # the moved rows: those of v3d_points_in_boxes(use_z = 1) on the ORIGINAL boxes, lowest box index first, whose box moved
    if len(points) and len(boxes):
        inside = points_in_boxes_mask(dev(points), dev(boxes), True).cpu().numpy()
        owner = np.where(inside.any(1), inside.argmax(1), -1)
    else:
        owner = np.full(len(points), -1)
    np.testing.assert_array_equal(owner, ref["owner"])
    moved = (owner >= 0) & (np.append(ref["chosen"], -1)[owner] >= 0)  # (owner -1 reads the appended -1)
    np.testing.assert_array_equal(bits(out_p[~moved]), bits(points[~moved]))
    np.testing.assert_array_equal(bits(out_p[:, 3:]), bits(points[:, 3:]))
    displaced = (ref["points"][moved][:, :3] != points[moved][:, :3]).any(1)  # (a try of zero translation and rotation displaces nothing)
    assert (bits(out_p[moved][:, :3]) != bits(points[moved][:, :3])).any(1)[displaced].all(), "a row of a moved box did not move"
    ok, worst = R.within_ulps(out_p[moved][:, :3], ref["points"][moved][:, :3])
    print(f"[object_noise] {what}: {int(moved.sum())} moved points, largest error {worst:.2f} ulp")
    assert ok.all(), f"{int((~ok).sum())} coordinates beyond 4 ulp, largest {worst:.2f}"


@pytest.mark.parametrize("index", range(len(K.GPU_CASES)), ids=[f"n{c[0]}_T{c[1]}_N{c[2]}_C{c[3]}" for c in K.GPU_CASES])
def test_native_against_float64_restatement(index):
    inputs, ref = case("gpu", index)
    points, boxes, trans, rot = inputs
    noise = make_noise(rot.shape[1])
    assert noise.native_ok([boxes.shape[0]], rot.shape[1])
    out_p, out_b = noise(dev(points), dev(boxes), draws=(trans, rot))
    assert out_p.is_cuda and out_b.is_cuda and noise.last_chosen.is_cuda and noise.last_chosen.dtype == torch.int32
    check_against_restatement(inputs, ref, out_p, out_b, noise.last_chosen, f"case {K.GPU_CASES[index][:4]}")
    if index == 0:  # two overlapping boxes share points: the lower index owns them
        both = np.stack([R.inside_distance(points, b) > 0 for b in boxes], 1).all(1)
        assert both.sum() > 10 and (ref["owner"][both] == 0).all()
    # numpy in -> numpy out, same bits
    np_p, np_b = noise(points, boxes, draws=(trans, rot))
    assert isinstance(np_p, np.ndarray) and isinstance(np_b, np.ndarray)
    np.testing.assert_array_equal(bits(np_p), bits(out_p))
    np.testing.assert_array_equal(bits(np_b), bits(out_b))


@pytest.mark.parametrize("name", sorted(K.hand_cases()))
def test_native_hand_cases(name):
    points, boxes, trans, rot, want = K.hand_cases()[name]
    noise = make_noise(rot.shape[1])
    out_p, out_b = noise(dev(points), dev(boxes), draws=(trans, rot))
    np.testing.assert_array_equal(noise.last_chosen.cpu().numpy(), want)
    check_against_restatement((points, boxes, trans, rot), R.object_noise(points, boxes, trans, rot), out_p, out_b, noise.last_chosen, name)


@pytest.mark.parametrize("index", range(len(K.GPU_CASES)), ids=[f"n{c[0]}_T{c[1]}_N{c[2]}_C{c[3]}" for c in K.GPU_CASES])
def test_native_against_torch_statement(index):
    """Same predicate, same candidate arithmetic: chosen and boxes bit for bit; points within 4 ulp (torch.cos against cosf)."""
    (points, boxes, trans, rot), _ = case("gpu", index)
    noise = make_noise(rot.shape[1])
    p, b, tr, ro = dev(points), dev(boxes), dev(trans), dev(rot)
    out_p, out_b = noise(p, b, draws=(tr, ro))
    ts_p, ts_b, ts_chosen = noise.torch_statement(p, b, tr, ro)
    assert torch.equal(noise.last_chosen, ts_chosen)
    np.testing.assert_array_equal(bits(out_b), bits(ts_b))
    ok, worst = R.within_ulps(out_p.cpu().numpy(), ts_p.double().cpu().numpy())
    same = float((bits(out_p) == bits(ts_p)).mean())
    print(f"[object_noise] native against torch_statement, case {K.GPU_CASES[index][:4]}: largest difference {worst:.2f} ulp, {same:.4f} of the words equal")
    assert ok.all()


def test_batch_equals_single_calls_bit_for_bit():
    """B = 3: a frame of 27 boxes, a frame without boxes, a frame without points -- one native call against three."""
    T = 9
    a = K.make_case(27, T, 700, 4, seed=3, pairs=1)
    b = K.make_case(0, T, 300, 4, seed=4)
    c = K.make_case(65, T, 0, 4, seed=5, pairs=1, stuck=1)
    noise = make_noise(T)
    frames = [a, b, c]
    single, single_chosen = [], []
    for p, bx, tr, ro in frames:
        single.append(noise(dev(p), dev(bx), draws=(tr, ro)))
        single_chosen.append(noise.last_chosen)
    out_p, out_b = noise.batch([dev(f[0]) for f in frames], [dev(f[1]) for f in frames], draws=[(f[2], f[3]) for f in frames])
    assert torch.equal(noise.last_chosen, torch.cat(single_chosen)) and (noise.last_chosen >= 0).any() and (noise.last_chosen < 0).any()
    for (sp, sb), bp, bb, f in zip(single, out_p, out_b, frames):
        assert bp.shape == f[0].shape and bb.shape == f[1].shape
        np.testing.assert_array_equal(bits(bp), bits(sp))
        np.testing.assert_array_equal(bits(bb), bits(sb))
    np.testing.assert_array_equal(bits(out_p[1]), bits(b[0]))  # no boxes: the points are copied
    assert not np.array_equal(bits(out_p[0]), bits(a[0]))


def test_deterministic():
    (points, boxes, trans, rot), _ = case("gpu", 2)
    noise = make_noise(rot.shape[1])
    p, b, tr, ro = dev(points), dev(boxes), dev(trans), dev(rot)
    first = noise(p, b, draws=(tr, ro)) + (noise.last_chosen,)
    second = noise(p, b, draws=(tr, ro)) + (noise.last_chosen,)
    for x, y in zip(first, second):
        assert torch.equal(x, y) and x.data_ptr() != y.data_ptr()


@pytest.mark.parametrize("index", range(len(LIMIT_CASES)), ids=["n129", "T257"])
def test_beyond_the_limits_the_entry_refuses_and_the_class_takes_the_torch_statement(index, monkeypatch):
    from vision3d_amd import _lib as L
    inputs, ref = case("limit", index)
    points, boxes, trans, rot = inputs
    n, T = rot.shape
    p, b, tr, ro = dev(points), dev(boxes), dev(trans), dev(rot)
    out_p, out_b, chosen = torch.empty_like(p), torch.empty_like(b), torch.empty(n, dtype=torch.int32, device="cuda")
    work = L.workspace(n * T * 16 + 256, "cuda")
    code = L.lib().v3d_object_noise(L.ptr(p), L.host_i32([0, len(points)]), L.ptr(b), L.host_i32([0, n]), 1, 4, L.ptr(tr), L.ptr(ro), T, 0.01,
                                    L.ptr(out_p), L.ptr(out_b), L.ptr(chosen), L.ptr(work), work.numel(), L.stream_ptr())
    assert code == -3  # V3D_EUNSUPPORTED
    noise = make_noise(T)
    assert not noise.native_ok([n], T)
    called = []
    statement = noise.torch_statement
    monkeypatch.setattr(noise, "torch_statement", lambda *a: called.append(1) or statement(*a))
    got_p, got_b = noise(p, b, draws=(tr, ro))
    assert called == [1]
    check_against_restatement(inputs, ref, got_p, got_b, noise.last_chosen, f"torch statement, case {LIMIT_CASES[index][:4]}")


def test_no_host_synchronisation_graph_replay_follows_new_draws():
    """The native call captured on a side stream into one single-stream graph; the draw tensors overwritten in place; the replay must
    equal an eager call on the new draws."""
    (points, boxes, trans, rot), _ = case("gpu", 2)
    n, T = rot.shape
    noise = make_noise(T)
    p, b, tr, ro = dev(points), dev(boxes), dev(trans), dev(rot)
    rng = np.random.RandomState(9)
    new_tr, new_ro = dev(rng.normal(0, [1.0, 1.0, 0.5], (n, T, 3)).astype(np.float32)), dev(rng.uniform(-0.78, 0.78, (n, T)).astype(np.float32))
    want_p, want_b = noise(p, b, draws=(new_tr, new_ro))  # (also the warm-up outside the capture)
    want_chosen = noise.last_chosen
    old_chosen = (noise(p, b, draws=(tr, ro)), noise.last_chosen)[1]
    assert not torch.equal(old_chosen, want_chosen)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out_p, out_b = noise(p, b, draws=(tr, ro))
        out_chosen = noise.last_chosen
    tr.copy_(new_tr)
    ro.copy_(new_ro)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_chosen, want_chosen) and torch.equal(out_p, want_p) and torch.equal(out_b, want_b)


@pytest.fixture(scope="module")
def golden_aug():
    return np.load(os.path.join(HERE, "golden", "augmentation.npz"))


def _database(g, tag):
    db = {}
    for c in range(3):
        sizes = g[f"{tag}_db{c}_sizes"]
        pts = np.split(g[f"{tag}_db{c}_points"], np.cumsum(sizes)[:-1]) if len(sizes) else []
        db[c] = [dict(points=q, box=bx) for q, bx in zip(pts, g[f"{tag}_db{c}_boxes"])]
    return db


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "chain"])
def test_chain_runs_the_noise_first_on_the_shared_generator(golden_aug, fused):
    """Enabled: ChainedAugmentation == the noise class, then today's chain, on twin generators.  Disabled (default, or a config without
    the key): today's chain, bit for bit, and the generator in the same state."""
    from vision3d_amd.dataset import ChainedAugmentation, ObjectNoiseAugmentation, SampleDatabase
    g, tag = golden_aug, "car"
    off = second_car_cfg()
    old = second_car_cfg()
    del old.AUG["OBJECT_NOISE"]
    on = second_car_cfg()
    on.AUG.OBJECT_NOISE.ENABLED = True
    on.AUG.OBJECT_NOISE.NUM_TRY = 20
    db = SampleDatabase(_database(g, tag), off.NUM_CLASSES)
    pts, boxes, cls = dev(g[f"{tag}_points"]), dev(g[f"{tag}_boxes"]), dev(g[f"{tag}_class_idx"])
    rng, twin = np.random.RandomState(5), np.random.RandomState(5)
    got = ChainedAugmentation(on, database=db, rng=rng, fused=fused)(pts, boxes, cls)
    noise = ObjectNoiseAugmentation(on, twin)
    noisy_p, noisy_b = noise(pts, boxes)
    assert (noise.last_chosen >= 0).any() and not torch.equal(noisy_b, boxes) and not torch.equal(noisy_p, pts)
    want = ChainedAugmentation(off, database=db, rng=twin, fused=fused)(noisy_p, noisy_b, cls)
    for x, y in zip(got, want):
        assert x.dtype == y.dtype and torch.equal(x, y)
    for a, b in zip(rng.get_state(), twin.get_state()):
        np.testing.assert_array_equal(a, b)
    rng, twin = np.random.RandomState(6), np.random.RandomState(6)
    today = ChainedAugmentation(old, database=db, rng=rng, fused=fused)(pts, boxes, cls)
    default = ChainedAugmentation(off, database=db, rng=twin, fused=fused)(pts, boxes, cls)
    for x, y in zip(today, default):
        assert torch.equal(x, y)
    for a, b in zip(rng.get_state(), twin.get_state()):
        np.testing.assert_array_equal(a, b)

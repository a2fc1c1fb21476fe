"""CPU: the pillar plan (cfg.PILLAR.PLAN) without a GPU -- the key's gating, the refusals that stay, the new C-ABI entries in the
built library, and vision3d_amd/csrc/pillar_plane_device.h (where a row lands in the planes and the bitmap) compiled for the host as
a stand-alone program under the address and undefined-behaviour sanitizers (tests/host/pillar_plan_host_shim.cpp).  The GPU runs are
tests/test_gpu_pillar_plan.py."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_key_gating():
    from vision3d_amd.core import config
    from vision3d_amd.core.config import pillar_plan_enabled
    assert config.cfg.PILLAR.PLAN is False and not pillar_plan_enabled(config.cfg)
    assert not pillar_plan_enabled(config.second_car_cfg()) and not pillar_plan_enabled(config.pillar_car_cfg())
    inert = config.second_car_cfg().merge_from_dict(dict(PILLAR=dict(PLAN=True)))  # PLAN without ENABLED: inert
    assert not pillar_plan_enabled(inert)
    inert.PILLAR.DYNAMIC = True  # ... and nothing to refuse
    assert not pillar_plan_enabled(inert)
    old = config.pillar_car_cfg()
    del old["PILLAR"]["PLAN"]  # a pillar config written before the key existed
    assert not pillar_plan_enabled(old)
    older = config.second_car_cfg()
    del older["PILLAR"]
    assert not pillar_plan_enabled(older)
    cfg = config.pillar_plan_car_cfg()
    assert pillar_plan_enabled(cfg)
    want = config.pillar_car_cfg()
    want.PILLAR.PLAN = True
    assert cfg == want and cfg.PILLAR == dict(ENABLED=True, CHANNELS=128, DYNAMIC=False, PLAN=True)
    assert cfg.VOXEL_SIZE == [0.4, 0.4, 4.0] and cfg.MAX_OCCUPANCY == 32 and cfg.MAX_VOXELS == 12000 and cfg.STRIDES == [1]
    both = config.pillar_plan_car_cfg()
    both.PILLAR.DYNAMIC = True
    with pytest.raises(ValueError, match="follow-up.*slower of the two"):
        pillar_plan_enabled(both)


def test_refusals_without_the_key_stay():
    from vision3d_amd.core.config import pillar_car_cfg, pillar_plan_car_cfg, second_car_cfg
    from vision3d_amd.detector.pillar import PILLAR_DEFAULTS, pillar_config, refuse_pillar
    old = second_car_cfg()
    del old["PILLAR"]
    assert pillar_config(old) == dict(ENABLED=False, CHANNELS=128) == PILLAR_DEFAULTS
    with pytest.raises(ValueError, match="does not support the pillar encoder yet"):
        refuse_pillar(pillar_car_cfg(), "this entry point")
    with pytest.raises(ValueError, match="does not support the pillar encoder yet"):
        refuse_pillar(pillar_plan_car_cfg(), "an entry point that has no plan (PV_RCNN)")  # the function itself knows no key


def test_model_reads_the_key():
    """Construction needs no GPU: the model remembers the key, and refuses it together with DYNAMIC."""
    import pillar_cases as cases
    from vision3d_amd.detector import Second
    plain, cfg = cases.tiny_cfg(), cases.tiny_cfg()
    cfg.PILLAR.PLAN = True
    assert Second(plain).pillar_plan is False and Second(cfg).pillar_plan is True
    cfg.PILLAR.DYNAMIC = True
    with pytest.raises(ValueError, match="follow-up"):
        Second(cfg)
    with pytest.raises(ValueError, match="cfg.PILLAR.ENABLED"):
        Second(plain).backbone_plan(1, 16384)


def test_symbols_in_the_built_library():
    from vision3d_amd import _lib as L
    handle = ctypes.CDLL(L.LIB_PATH)
    for name in ("v3d_pillar_encode_planes", "v3d_pillar_planes_clear"):
        assert hasattr(handle, name), f"{name} is not exported by the built library"
        assert name in L.exported_symbols()
    # the limits are answered before any launch (and before any pointer is looked at): no GPU needed
    lib = L.lib()
    geom = L.host_f32([0.4, 0.4, 4.0, 0.2, -3.8, -1.0])
    for P, C, CH in ((65, 4, 128), (0, 4, 128), (8, 2, 128), (8, 9, 128), (8, 4, 64), (8, 4, 96)):
        assert lib.v3d_pillar_encode_planes(None, None, None, None, 4, P, C, geom, None, CH, None, None, 1, 20, 16, 0, None, None, None, None, None,
                                            None) == -3, (P, C, CH)
    assert lib.v3d_pillar_encode_planes(None, None, None, None, 0, 8, 4, geom, None, 128, None, None, 1, 20, 16, 0, None, None, None, None, None,
                                        None) == 0  # an empty capacity launches nothing
    assert lib.v3d_pillar_encode_planes(None, None, None, None, 4, 8, 4, geom, None, 128, None, None, 1, 20, 16, 0, None, None, None, None, None,
                                        None) == -1  # ... and null buffers are refused
    assert lib.v3d_pillar_encode_planes(None, None, None, None, 4, 8, 4, geom, None, 128, None, None, 1, 20, 16, 1, None, None, None, None, None,
                                        None) == -1  # f16s without an entry
    assert lib.v3d_pillar_planes_clear(None, None, 4, 1, 20, 16, 64, None, None, None, None, None) in (-1, -3)


def test_plane_header_under_the_sanitizers():
    """Out-of-map rows on every side, device counts below / at / above the capacity (0 and negative among them), W = 16, 33, 65 and 1:
    every store of the two kernels' loops stays inside buffers of exactly the plan's sizes, and planes and bitmap hold the definition."""
    src = os.path.join(HERE, "host", "pillar_plan_host_shim.cpp")
    exe = os.path.join(HERE, "host", "_build", "pillar_plan_host_shim")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.strip().endswith("ok") and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr

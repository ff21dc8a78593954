"""CPU suite: the ABI of rdx_generate_rays / rdx_accumulate (the two ends of a frame on device memory) and the COMPARAND of their
GPU tests: the numpy restatement of the running mean in tests/raygen_cases.py (running_mean), driven by the CPU oracle's per-sample
colours, is held to the oracle's own imageScratch, bit for bit, before test_gpu_raygen.py holds rd.Accumulate to it."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import golden_cases as gc
import oracle_bind as ob
import raygen_cases as rc
import shade_cases as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mods(built):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import _lib, rd, scenes
    return _lib, rd, scenes


def test_the_library_exports_both_calls(mods):
    _lib, _, _ = mods
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "rdx.h")).read()
    for name in ("rdx_generate_rays", "rdx_accumulate"):
        assert name in _lib.SIGNATURES and getattr(L, name)
        assert re.search(r"\b%s\(" % name, hdr)
    P, Z, U, Fl = C.c_void_p, C.c_size_t, C.c_uint32, C.c_float
    assert _lib.SIGNATURES["rdx_generate_rays"] == (C.c_int, [P, U, U, P, Z, U, U, P, Z, Fl, Fl, P, Z, P, Z])
    assert _lib.SIGNATURES["rdx_accumulate"] == (C.c_int, [P, Z, U, U, P, Z, U, P, P, U, C.POINTER(U)])
    assert re.search(r"typedef struct rdx_raygen_seed\s*\{\s*uint32_t in\[3\];\s*uint32_t _0;\s*\}\s*rdx_raygen_seed;", hdr)
    build = open(os.path.join(ROOT, "radiance-ray-tracing_amd", "build.py")).read()
    assert '"raygen.hip"' in build and '"raygen.h"' in build and '"raygen_device.h"' in build


def test_rd_exposes_the_calls_and_the_seed_record(mods):
    _lib, rd, scenes = mods
    for name in ("GenerateRays", "GenerateRaysTorch", "Accumulate", "AccumulateTorch"):
        assert callable(getattr(rd, name)), name
    assert rd.RAYGEN_SEED_DTYPE.itemsize == 16 == C.sizeof(_lib.rdx_raygen_seed) and rd.RAYGEN_SEED_DTYPE == rc.RAYGEN_SEED_DTYPE
    assert [(n, rd.RAYGEN_SEED_DTYPE.fields[n][1]) for n in ("in", "_0")] == [("in", 0), ("_0", 12)]
    assert hasattr(scenes.DeviceScene, "frame_buffers")
    facade = open(os.path.join(ROOT, "include", "radiance.h")).read()
    assert "GenerateRays" in facade and "Accumulate" in facade


def test_running_mean_reproduces_the_oracles_own_frames(mods):
    """the oracle's per-sample colours (its seams under shade_cases.oracle_callables) folded by the restated running mean give the
    imageScratch of the oracle's own raygen for both progressive frames of c0, bit for bit"""
    _, rd, scenes = mods
    s = gc.small_scene(scenes, "c0")
    blob = gc.scene_blob(rd, s)
    osc = ob.OracleScene(s, blob)
    p = osc.rtprop[0]
    assert int(p["batchSize"]) == 2 and int(p["totalSamples"]) == 0
    generate, bounce = sh.oracle_callables(ob.OracleScene(s, blob), blob)
    got = rc.frames_of(s.width * s.height, 0, 2, int(p["depth"]), 2, generate, bounce)
    for f in range(2):
        osc.frame()
        want = osc.scratch.reshape(-1, 4)
        same = (sh.bits(got[f]) == sh.bits(want)).all(1)
        assert same.all(), "frame %d: %d of %d pixels differ" % (f, int((~same).sum()), same.shape[0])
    assert not np.array_equal(got[0], got[1]) and got[1][:, :3].any()


def test_running_mean_by_hand():
    """frame 0 overwrites rgb, later frames are ((frame * mean) + colour) / (frame + 1) rounded after every operation; w and the
    pixels not named stay"""
    F = np.float32
    scratch = np.full((4, 4), 9.0, F)
    rc.running_mean(scratch, np.array([[0.1, 0.2, 0.3, 5.0], [1.5, -2.0, 0.0, 5.0]], F), 0, pixels=[2, 0])
    assert np.array_equal(scratch[2], np.array([0.1, 0.2, 0.3, 9.0], F)) and np.array_equal(scratch[0], np.array([1.5, -2.0, 0.0, 9.0], F))
    assert (scratch[[1, 3]] == 9.0).all()
    rc.running_mean(scratch, np.array([[0.7, 0.7, 0.7, 0.0]], F), 3, pixels=[2])
    want = [F(F(F(3.0) * F(v)) + F(0.7)) / F(4.0) for v in (0.1, 0.2, 0.3)]
    assert np.array_equal(sh.bits(scratch[2, :3]), sh.bits(np.array(want, F))) and scratch[2, 3] == 9.0
    with pytest.raises(AssertionError):
        rc.running_mean(scratch, np.zeros((2, 4), F), 1, pixels=[1, 1])
    assert np.array_equal(rc.debug_rgba8(np.array([[0.0, 0.5, 0.999]], F)), np.array([[0, 127, 254, 255]], np.uint8))


def test_both_calls_on_an_uninitialised_library_name_rdx_init(mods):
    """(a fresh process: the suite's other tests may have initialised the library in this one)"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import rrt_amd\n"
            "from radiance_ray_tracing_amd import _lib\n"
            "L = _lib.lib()\n"
            "rc = L.rdx_generate_rays(None, 0, 0, None, 0, 0, 0, None, 0, 0.001, 1000.0, None, 0, None, 0)\n"
            "print(rc, _lib.last_error())\n"
            "rc = L.rdx_accumulate(None, 0, 0, 0, None, 0, 0, None, None, 0, None)\n"
            "print(rc, _lib.last_error())\n") % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 2
    for line in lines:
        rcode, msg = line.split(None, 1)
        assert int(rcode) < 0 and "rdx_init" in msg, out.stdout

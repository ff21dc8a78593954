"""CPU suite: the ABI of rdx_trace_paths (radiance along the caller's own rays), the argument checks of its Python wrappers, and
the COMPARAND of its GPU tests: paths_cases.fold, the numpy restatement of the raygen loop's fold, checked on hand-made shade
records before test_gpu_paths.py drives it with rd.QueryRays / rd.ShadeHits and holds rd.TracePaths to it."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import paths_cases as pc
import shade_cases as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def mods(built):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import _lib, rd, scenes
    return _lib, rd, scenes


def test_the_library_exports_the_call(mods):
    _lib, rd, _ = mods
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "rdx.h")).read()
    assert "rdx_trace_paths" in _lib.SIGNATURES and L.rdx_trace_paths
    assert re.search(r"\brdx_trace_paths\(rdx_buffer tlas,", hdr) and hdr.index("rdx_trace_paths(") > hdr.index("rdx_accumulate(")
    P, Z, U = C.c_void_p, C.c_size_t, C.c_uint32
    assert _lib.SIGNATURES["rdx_trace_paths"] == (C.c_int, [P, P, Z, P, Z, U, U, C.POINTER(_lib.rdx_shading_buffers), P, Z, P, Z])
    assert L.rdx_trace_paths.argtypes == _lib.SIGNATURES["rdx_trace_paths"][1] and L.rdx_trace_paths.restype is C.c_int
    build = open(os.path.join(ROOT, "radiance-ray-tracing_amd", "build.py")).read()
    assert '"paths.hip"' in build and '"paths.h"' in build
    for name in ("TracePaths", "TracePathsTorch"):
        assert callable(getattr(rd, name)), name
    assert "TracePaths" in open(os.path.join(ROOT, "include", "radiance.h")).read()


def test_an_uninitialised_library_refuses_and_names_the_call(mods):
    """(a fresh process: the suite's other tests may have initialised the library in this one)"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import rrt_amd\n"
            "from radiance_ray_tracing_amd import _lib\n"
            "L = _lib.lib()\n"
            "rc = L.rdx_trace_paths(None, None, 0, None, 0, 0, 4, None, None, 0, None, 0)\n"
            "print(rc, _lib.last_error())\n") % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rcode, msg = out.stdout.strip().split(None, 1)
    assert int(rcode) < 0 and "rdx_trace_paths" in msg and "rdx_init" in msg, out.stdout


def test_the_wrappers_refuse_wrong_arguments_before_the_library(mods, monkeypatch):
    """neither wrapper reaches rdx_trace_paths with an argument of the wrong kind: the library is not initialised here, and a call
    that got through would fail with its message instead of the wrapper's"""
    _lib, rd, _ = mods
    reached = []
    real = _lib.lib

    class Spy:
        def __getattr__(self, name):
            if name == "rdx_trace_paths":
                reached.append(name)
            return getattr(real(), name)
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    buf = rd.Buffer(1234, 4096)
    sb = rd.ShadingBuffers(buf, buf, buf, None, buf, buf)
    bad = [dict(tlas=None), dict(rays=7), dict(keys=np.zeros(4)), dict(scene_buffers=(buf, buf)), dict(scene_buffers=rd.ShadingBuffers(buf, buf, None, None, buf, buf)),
           dict(scene_buffers=rd.ShadingBuffers(buf, buf, buf, 5, buf, buf)), dict(scene_buffers=rd.ShadingBuffers(buf, buf, buf, None, buf, buf, None, "s")),
           dict(radiance=np.zeros(4)), dict(hits=7), dict(hits=[1]), dict(n=-1), dict(n=2.5), dict(max_depth=-1), dict(max_depth="4")]
    for kw in bad:
        a = dict(tlas=buf, rays=buf, keys=buf, n=4, max_depth=4, scene_buffers=sb, radiance=buf, hits=None)
        a.update(kw)
        with pytest.raises(rd.RadianceError, match="TracePaths"):
            rd.TracePaths(a.pop("tlas"), a.pop("rays"), a.pop("keys"), a.pop("n"), a.pop("max_depth"), a.pop("scene_buffers"), **a)
    import torch
    r, k = torch.zeros((5, 8), dtype=torch.float32), torch.zeros((5, 4), dtype=torch.int32)
    for rays, keys in ((r, k), (r.numpy(), k), (None, k)):       # CPU tensors, arrays, nothing: refused before any CUDA call
        with pytest.raises(rd.RadianceError, match="TracePathsTorch: rays"):
            rd.TracePathsTorch(buf, rays, keys, 4, sb)
    assert not reached


# ---- the fold on hand-made shade records ---------------------------------------------------------------------------------------
def _records(rows):
    """rows: (hit, color, colorOccluded, nextFactor)"""
    s = np.zeros(len(rows), sh.SHADE_DTYPE)
    for i, (hit, c, co, nf) in enumerate(rows):
        s[i]["hit"], s[i]["color"], s[i]["colorOccluded"], s[i]["nextFactor"] = hit, c, co, nf
        s[i]["slot"] = 0 if hit else sh.NO_SLOT
    return s


ENV = tuple(sh.ENVIRONMENT)
MISS = (0, ENV, ENV, (0, 0, 0))


def test_fold_by_hand():
    """five paths, depth 3: 0 misses at once (the miss colour shows), 1 hits lit and misses at depth 1 (the miss colour does NOT
    show), 2 hits occluded, then lit, then lit at the last depth, 3 hits lit three times, 4 hits occluded twice and misses at the last depth; the
    survivors come back in another order each time -- every path's colour is (colour + contribution * payload colour) rounded after each
    operation, the contribution the running product of the nextFactors"""
    A, B, Cc = (0.3, 0.5, 0.7), (0.11, 0.13, 0.17), (1.25, 0.0, 2.0)
    f1, f2 = (0.9, 0.8, 0.7), (0.333, 1.5, 0.01)
    calls = []

    def bounce(depth, path):
        calls.append((depth, path.tolist()))
        if depth == 0:
            assert path.tolist() == [0, 1, 2, 3, 4]
            s = _records([MISS, (1, A, B, f1), (1, A, B, f2), (1, Cc, B, f1), (1, B, A, f2)])
            return s, np.array([False, False, True, False, True]), [4, 2, 1, 3]          # survivors in another order
        if depth == 1:
            assert path.tolist() == [4, 2, 1, 3]
            s = _records([(1, A, Cc, f1), (1, Cc, A, f1), MISS, (1, B, A, f2)])
            return s, np.array([True, False, True, False]), [3, 0, 1]
        assert depth == 2 and path.tolist() == [3, 4, 2]
        s = _records([(1, A, B, f1), MISS, (1, B, Cc, f2)])
        return s, np.array([False, False, False]), [2, 0]
    rad, counts = pc.fold(5, 3, bounce)
    assert [c[0] for c in calls] == [0, 1, 2] and counts == [5, 4, 3, 2]
    v = lambda t: np.array(t, F)
    one = np.ones(3, F)
    want = np.zeros((5, 4), F)
    want[0, :3] = v(ENV)
    want[1, :3] = np.zeros(3, F) + one * v(A)                                           # the later miss adds nothing
    c2 = np.zeros(3, F) + one * v(B); t2 = one * v(f2)                                   # occluded
    c2 = c2 + t2 * v(Cc); t2 = t2 * v(f1)                                                # lit
    c2 = c2 + t2 * v(B)                                                                  # the last depth
    want[2, :3] = c2
    c3 = np.zeros(3, F) + one * v(Cc); t3 = one * v(f1)
    c3 = c3 + t3 * v(B); t3 = t3 * v(f2)
    c3 = c3 + t3 * v(A)
    want[3, :3] = c3
    c4 = np.zeros(3, F) + one * v(A); t4 = one * v(f2)                                   # occluded at depth 0
    c4 = c4 + t4 * v(Cc)                                                                 # occluded at depth 1, then a miss
    want[4, :3] = c4
    assert np.array_equal(sh.bits(rad), sh.bits(want)), (rad, want)
    assert not sh.bits(rad[:, 3]).any()


def test_fold_depths():
    """max_depth 0 traces nothing and gives zeros; depth 1 calls the bounce once; a batch whose paths all end stops early"""
    rad, counts = pc.fold(3, 0, lambda d, p: pytest.fail("bounce called at depth 0"))
    assert rad.shape == (3, 4) and not rad.any() and counts == []
    seen = []

    def once(depth, path):
        seen.append(depth)
        return _records([(1, (0.5, 0.5, 0.5), (0.1, 0.1, 0.1), (1, 1, 1)), MISS]), np.array([True, False]), [0]
    rad, counts = pc.fold(2, 1, once)
    assert seen == [0] and counts == [2, 1]
    assert np.array_equal(sh.bits(rad[:, :3]), sh.bits(np.array([[0.1, 0.1, 0.1], ENV], F)))
    seen.clear()
    rad, counts = pc.fold(2, 8, lambda d, p: (seen.append(d), (_records([MISS] * p.size), np.zeros(p.size, bool), []))[1])
    assert seen == [0] and counts == [2, 0] and np.array_equal(sh.bits(rad[:, :3]), sh.bits(np.tile(sh.ENVIRONMENT, (2, 1))))


def test_arbitrary_batch_has_the_stated_shape(mods):
    """the batch generator of the GPU tests: n = 1037, every interval kind, distinct frameIDs with 0 and 0xffffffff, repeated
    pixels, non-unit and axis-aligned directions, origins on both sides of the box"""
    _, rd, _ = mods
    lo, hi = np.array([-2.0, 0.0, -3.0]), np.array([2.0, 4.0, 3.0])
    first = lambda rays: (np.arange(rays.shape[0]) % 3 != 0, np.full(rays.shape[0], 2.0, F))
    rays, keys, kind = pc.arbitrary_batch(rd, lo, hi, first, 7)
    n = pc.N_BATCH
    assert rays.shape == (n,) and n == 1037 and n % 256 and n % 64
    assert all(int((kind == k).sum()) >= 20 for k in range(len(pc.KINDS)))
    assert np.unique(keys["frameID"]).size == n and {0, 0xffffffff} <= set(keys["frameID"].tolist())
    assert np.unique(keys["pixel"]).size < n and keys["depth"].any() and keys["_0"].any()
    o, d = rays["origin"].astype(np.float64), rays["direction"].astype(np.float64)
    inside = ((o >= lo) & (o <= hi)).all(1)
    assert inside.sum() > 300 and (~inside).sum() > 100
    length = np.linalg.norm(d, axis=1)
    assert (np.abs(length - 1) > 0.05).mean() > 0.8 and int(((d == 0).sum(1) == 2).sum()) >= n // 8
    assert np.isnan(rays["tmin"]).sum() >= 10 and np.isnan(rays["tmax"]).sum() >= 10 and int((rays["tmax"] == 0).sum()) >= 20
    assert (rays["tmax"][kind == 1] == F(1.0)).all() and (rays["tmin"][kind == 2] == F(3.01)).all()
    stock = kind == 0
    assert (sh.bits(rays["tmin"][stock]) == sh.bits(F(0.001))).all() and (sh.bits(rays["tmax"][stock]) == sh.bits(F(1000.0))).all()

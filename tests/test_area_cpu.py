"""CPU suite: the ABI of rdx_area_light_hits / rdx_trace_paths_area (quad and triangle area lights from a second caller-owned light
table), the argument checks of their Python wrappers, the rows the two calls hand to the range rule, rd.QuadLight / rd.TriangleLight,
the rule that keeps the random streams apart, area_cases.emitted_area -- the numpy restatement of what an area record emits at a
point -- on hand-made rows, and the convergence of the estimator to an analytic form factor, before test_gpu_area.py holds the
calls to it."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import area_cases as ar
import shade_cases as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def mods(built):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import _lib, rd, scenes
    return _lib, rd, scenes


def test_the_record_is_four_float4(mods):
    _lib, rd, _ = mods
    want = dict(corner=0, type=12, edgeU=16, flags=28, edgeV=32, _0=44, radiance=48, _1=60)
    assert rd.AREA_LIGHT_DTYPE.itemsize == C.sizeof(_lib.rdx_area_light) == 64
    for name, off in want.items():
        assert rd.AREA_LIGHT_DTYPE.fields[name][1] == off == getattr(_lib.rdx_area_light, name).offset, name
    assert rd.AREA_LIGHT_DTYPE.fields["type"][0] == rd.AREA_LIGHT_DTYPE.fields["flags"][0] == np.dtype("<u4")
    assert rd.AREA_LIGHT_DTYPE.fields["corner"][0].shape == (3,)
    assert (rd.AREA_QUAD, rd.AREA_TRIANGLE, rd.AREA_TWO_SIDED, rd.MAX_PATH_LIGHTS) == (0, 1, 1, 16)
    hdr = open(os.path.join(ROOT, "include", "rdx.h")).read()
    for text in ("#define RDX_AREA_QUAD      0u", "#define RDX_AREA_TRIANGLE  1u", "#define RDX_AREA_TWO_SIDED 1u", "typedef struct rdx_area_light {"):
        assert text in hdr, text
    unit = open(os.path.join(ROOT, "radiance-ray-tracing_amd", "csrc", "area.h")).read()
    assert "struct AreaLight" in unit and "sizeof(AreaLight) == 64" in unit


def test_the_library_exports_the_calls(mods):
    _lib, rd, _ = mods
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "rdx.h")).read()
    P, Z, U = C.c_void_p, C.c_size_t, C.c_uint32
    want = {"rdx_area_light_hits": (C.c_int, [P, Z, P, Z, U, P, Z, P, Z, U, P, Z, P, Z, P, Z]),
            "rdx_trace_paths_area": (C.c_int, [P, P, Z, P, Z, U, U, P, Z, U, P, Z, U, C.POINTER(_lib.rdx_shading_buffers), P, Z, C.POINTER(U)])}
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig and getattr(L, name).argtypes == sig[1] and getattr(L, name).restype is C.c_int, name
        assert re.search(r"\b%s\(rdx_buffer " % name, hdr), name
    assert hdr.index("rdx_trace_paths_area(") > hdr.index("rdx_trace_paths_punctual(")
    build = open(os.path.join(ROOT, "radiance-ray-tracing_amd", "build.py")).read()
    assert '"area.hip"' in build and '"area.h"' in build
    for name in ("AreaLightHits", "AreaLightHitsTorch", "TraceAreaPaths", "TraceAreaPathsTorch", "QuadLight", "TriangleLight"):
        assert callable(getattr(rd, name)), name
    cxx = open(os.path.join(ROOT, "include", "radiance.h")).read()
    assert re.search(r"\bAreaLightHits\(", cxx) and re.search(r"\bTraceAreaPaths\(", cxx)
    assert "rdx_area_light_hits(" in cxx and "rdx_trace_paths_area(" in cxx


def test_an_uninitialised_library_refuses_and_names_the_call(mods):
    """(a fresh process: the suite's other tests may have initialised the library in this one)"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import rrt_amd\n"
            "from radiance_ray_tracing_amd import _lib\n"
            "L = _lib.lib()\n"
            "rc = L.rdx_area_light_hits(None, 0, None, 0, 0, None, 0, None, 0, 0, None, 0, None, 0, None, 0)\n"
            "print(rc, _lib.last_error())\n"
            "rc = L.rdx_trace_paths_area(None, None, 0, None, 0, 0, 4, None, 0, 3, None, 0, 2, None, None, 0, None)\n"
            "print(rc, _lib.last_error())\n") % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == 2, out.stdout
    for line, name in zip(lines, ("rdx_area_light_hits", "rdx_trace_paths_area")):
        rcode, msg = line.split(None, 1)
        assert int(rcode) < 0 and name in msg and "rdx_init" in msg, out.stdout


def test_the_wrappers_refuse_wrong_arguments_before_the_library(mods, monkeypatch):
    """no wrapper reaches the library with 17 records over the two tables, both or neither of keys and randoms, a stream above
    0xfffe, a table of a wrong dtype or shape, or an argument of the wrong kind: the library is not initialised here, and a call
    that got through would fail with its message instead of the wrapper's"""
    _lib, rd, _ = mods
    reached = []
    real = _lib.lib

    class Spy:
        def __getattr__(self, name):
            if name in ("rdx_area_light_hits", "rdx_trace_paths_area"):
                reached.append(name)
            return getattr(real(), name)
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    buf = rd.Buffer(1234, 4096)
    sb = rd.ShadingBuffers(buf, buf, buf, None, buf, buf)
    bad = [dict(tlas=None), dict(rays=7), dict(keys=np.zeros(4)), dict(lights=None), dict(area=None), dict(area=np.zeros(2, rd.AREA_LIGHT_DTYPE)),
           dict(lights=np.zeros(2, rd.PUNCTUAL_LIGHT_DTYPE)), dict(scene_buffers=(buf, buf)), dict(radiance=np.zeros(4)), dict(n=-1), dict(n=2.5),
           dict(max_depth=-1), dict(max_depth="4"), dict(light_count=-1), dict(area_count=-1), dict(light_count=15), dict(area_count=14), dict(light_count=17, area_count=0),
           dict(light_count=0, area_count=17), dict(area_count=2.5), dict(area_count="3"), dict(area_count=True), dict(area_count=None), dict(light_count=None)]
    for kw in bad:
        a = dict(tlas=buf, rays=buf, keys=buf, n=4, max_depth=4, lights=buf, light_count=3, area=buf, area_count=2, scene_buffers=sb, radiance=buf)
        a.update(kw)
        with pytest.raises(rd.RadianceError, match="TraceAreaPaths"):
            rd.TraceAreaPaths(a.pop("tlas"), a.pop("rays"), a.pop("keys"), a.pop("n"), a.pop("max_depth"), a.pop("lights"), a.pop("light_count"), a.pop("area"),
                              a.pop("area_count"), a.pop("scene_buffers"), **a)
    for kw in (dict(rays=None), dict(materials=7), dict(lights=np.zeros((2, 16), F)), dict(index=-1), dict(index=1.5), dict(index=True), dict(lit=7),
               dict(shadow=7), dict(keys=None), dict(randoms=buf), dict(keys=7), dict(keys=None, randoms=np.zeros(4)), dict(stream=-1), dict(stream=0xffff),
               dict(stream=1.5), dict(stream=True), dict(index=0x10000)):
        a = dict(rays=buf, materials=buf, n=4, lights=buf, index=1, keys=buf, randoms=None, stream=None, lit=buf, shadow=buf)
        a.update(kw)
        with pytest.raises(rd.RadianceError, match="AreaLightHits"):
            rd.AreaLightHits(a.pop("rays"), a.pop("materials"), a.pop("n"), a.pop("lights"), a.pop("index"), **a)
    import torch
    r, k, m = torch.zeros((5, 8), dtype=torch.float32), torch.zeros((5, 4), dtype=torch.int32), torch.zeros((5, 16), dtype=torch.float32)
    t3 = torch.zeros((3, 16), dtype=torch.float32)
    for rays in (r, r.numpy(), None):       # CPU tensors, arrays, nothing: refused before any CUDA call
        with pytest.raises(rd.RadianceError, match="TraceAreaPathsTorch: (rays|lights|area lights)"):
            rd.TraceAreaPathsTorch(buf, rays, k, 4, None, t3, sb)
        with pytest.raises(rd.RadianceError, match="TraceAreaPathsTorch: rays"):
            rd.TraceAreaPathsTorch(buf, rays, k, 4, None, None, sb)
        with pytest.raises(rd.RadianceError, match="AreaLightHitsTorch: (rays|area lights)"):
            rd.AreaLightHitsTorch(rays, m, t3, 0, keys=k)
    # a table of a wrong dtype or shape, or no tensor at all: the table is looked at first, so the refusal names it
    for tab in (t3.double(), t3[:, :15], t3.reshape(-1), torch.zeros((3, 32))[:, ::2], t3.numpy()):
        with pytest.raises(rd.RadianceError, match="TraceAreaPathsTorch: area lights"):
            rd.TraceAreaPathsTorch(buf, r, k, 4, None, tab, sb)
        with pytest.raises(rd.RadianceError, match="TraceAreaPathsTorch: lights"):
            rd.TraceAreaPathsTorch(buf, r, k, 4, tab, None, sb)
        with pytest.raises(rd.RadianceError, match="AreaLightHitsTorch: area lights"):
            rd.AreaLightHitsTorch(r, m, tab, 0, keys=k)
    with pytest.raises(rd.RadianceError, match="AreaLightHitsTorch: area lights"):
        rd.AreaLightHitsTorch(r, m, None, 0, keys=k)
    assert not reached


def test_quad_and_triangle_light(mods):
    _, rd, _ = mods
    q = rd.QuadLight((-1, 1, -1), (2, 0, 0), (0, 0, 2), (3.0, 2.0, 1.0))
    assert q.dtype == rd.AREA_LIGHT_DTYPE and q.shape == () and int(q["type"]) == rd.AREA_QUAD and int(q["flags"]) == 0
    assert q["corner"].tolist() == [-1, 1, -1] and q["edgeU"].tolist() == [2, 0, 0] and q["edgeV"].tolist() == [0, 0, 2] and q["radiance"].tolist() == [3, 2, 1]
    assert float(q["_0"]) == 0 and float(q["_1"]) == 0 and np.array(q).tobytes()[44:48] == b"\0\0\0\0"
    t = rd.TriangleLight((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1), two_sided=True)
    assert int(t["type"]) == rd.AREA_TRIANGLE and int(t["flags"]) == rd.AREA_TWO_SIDED
    assert int(rd.QuadLight((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1), two_sided=True)["flags"]) == 1
    tab = ar.table(rd, [q, t])
    assert tab.shape == (2,) and tab.nbytes == 128 and tab[1]["type"] == 1
    # the record as the (A, 16) float32 tensor rows the torch route takes: type in column 3, flags in column 7
    words = tab.view(np.uint32).reshape(2, 16)
    assert words[:, 3].tolist() == [0, 1] and words[:, 7].tolist() == [0, 1]


def test_the_streams_do_not_collide():
    """for depth 0 .. 62 and stream 0 .. 15 every depth + ((stream + 1) << 16) is distinct, and distinct from every bare depth, which
    is what rdx_scatter_hits draws from; the largest stream the call accepts does not wrap"""
    depth, stream = np.meshgrid(np.arange(63), np.arange(16), indexing="ij")
    words = ar.stream_word(depth, stream).reshape(-1)
    assert words.dtype == np.uint32 and np.unique(words).shape[0] == 63 * 16
    assert not np.isin(words, np.arange(63, dtype=np.uint32)).any() and words.min() == 0x10000
    assert int(ar.stream_word(62, 0xfffe)) == 0xffff0000 + 62
    # pcg3d on distinct third words gives distinct pairs here (a spot check that the streams are not merely distinct inputs)
    r = ar.pcg3d(7, 11, np.concatenate([np.arange(63, dtype=np.uint32), words]))
    assert np.unique(sh.bits(r[:, :2]), axis=0).shape[0] == r.shape[0]
    assert r.dtype == F and (r >= 0).all() and (r <= 1).all()


def test_numpy_pcg3d_is_the_oracles():
    """area_cases.pcg3d, on which randoms_of rests, has the bits of oracle_bind.pcg3d, which tests/test_cpu_oracle.py holds to the
    reference's: on seeded triples, on the edges of uint32 and on the words of the streams"""
    import oracle_bind as ob
    rng = np.random.default_rng(3)
    x = rng.integers(0, 2**32, size=(4096, 3), dtype=np.uint64).astype(np.uint32)
    edges = np.array([[0, 0, 0], [0xffffffff] * 3, [7, 65535, 0x10000], [0xffffffff, 0, 0xffff003e], [1, 2, 3]], np.uint32)
    depth, stream = np.meshgrid(np.arange(63), np.arange(16), indexing="ij")
    words = ar.stream_word(depth, stream).reshape(-1)
    streams = np.stack([np.full(words.shape, 7, np.uint32), np.arange(words.shape[0], dtype=np.uint32), words], 1)
    for t in (x, edges, streams):
        assert np.array_equal(sh.bits(ar.pcg3d(t[:, 0], t[:, 1], t[:, 2])), sh.bits(ob.pcg3d(t))), t[:2]
    r = ar.randoms_of(np.full(8, 7, np.uint32), np.arange(8, dtype=np.uint32), 3, 2)
    assert np.array_equal(sh.bits(r["xyz"]), sh.bits(ob.pcg3d(np.stack([np.full(8, 7), np.arange(8), np.full(8, 3 + (3 << 16))], 1)))) and not r["w"].any()


def refusal(rd, rows, first_out, n=8):
    return rd.DebugCheckRanges(rows, first_out, n)


def test_the_rows_of_the_two_calls(mods):
    """the rows rdx_area_light_hits and rdx_trace_paths_area build (csrc/rdx_runtime.cpp), through the seam of the one rule"""
    _, rd, _ = mods
    n, base = 8, 0x10000
    def hits(light_off, light_size=4 * 64, lit=(0x50000, 16 * 8, 0), keys=(0x70000, 16 * 8, 0, 1), randoms=(0x80000, 16 * 8, 0, 0)):
        return [("ray", base, 32 * n, 0, 32 * n, 16, 1), ("material-record", 0x20000, 64 * n, 0, 64 * n, 16, 1), ("area-light", 0x30000, light_size, light_off, 64, 16, 1),
                ("key", keys[0], keys[1], keys[2], 16 * n, 16, keys[3]), ("randoms", randoms[0], randoms[1], randoms[2], 16 * n, 16, randoms[3]),
                ("lit", lit[0], lit[1], lit[2], 16 * n, 16, 1), ("shadow-ray", 0x60000, 32 * n, 0, 32 * n, 16, 1)]
    assert refusal(rd, hits(64), 5) is None and refusal(rd, hits(192), 5) is None
    msg = refusal(rd, hits(72), 5)
    assert msg and "area-light" in msg and "16" in msg and "72" in msg, msg
    msg = refusal(rd, hits(256), 5)           # record 4 of a table of 4
    assert msg and "area-light buffer" in msg, msg
    msg = refusal(rd, hits(64, lit=(0x30000, 4096, 112)), 5)          # lit begins inside record 1
    assert msg and "lit" in msg and "area-light" in msg and "overlap" in msg, msg
    assert refusal(rd, hits(64, lit=(0x30000, 4096, 128)), 5) is None
    msg = refusal(rd, hits(64, keys=(0x70000, 16 * 8, 8, 1)), 5)
    assert msg and "key" in msg and "16" in msg, msg
    msg = refusal(rd, hits(64, keys=(0x70000, 16 * 7, 0, 1)), 5)
    assert msg and "key buffer" in msg, msg
    msg = refusal(rd, hits(64, keys=(0x50000, 4096, 16 * 8 - 16, 1)), 5)     # the last key lies under lit
    assert msg and "lit" in msg and "key" in msg and "overlap" in msg, msg
    assert refusal(rd, hits(64, keys=(0x50000, 4096, 16 * 8 - 16, 0)), 5) is None        # an absent row overlaps nothing
    msg = refusal(rd, hits(64, keys=(0, 0, 0, 0), randoms=(0x50000, 4096, 16, 1)), 5)
    assert msg and "lit" in msg and "randoms" in msg and "overlap" in msg, msg
    msg = refusal(rd, hits(64, keys=(0, 0, 0, 0), randoms=(0x80000, 16 * 8, 4, 1)), 5)
    assert msg and "randoms" in msg and "16" in msg, msg

    def paths(lcount, acount, aoff=0, asize=16 * 64, rad=(0x50000, 16 * n, 0), lpresent=1, apresent=1):
        return [("ray", base, 32 * n, 0, 32 * n, 16, 1), ("key", 0x20000, 16 * n, 0, 16 * n, 16, 1), ("light-table", 0x30000, 16 * 64, 0, 64 * lcount, 16, lpresent),
                ("area-light-table", 0x38000, asize, aoff, 64 * acount, 16, apresent), ("scene (SceneProperties)", 0x40000, 176, 0, 176, 4, 1),
                ("radiance", rad[0], rad[1], rad[2], 16 * n, 16, 1)]
    assert refusal(rd, paths(8, 8), 5) is None and refusal(rd, paths(0, 16), 5) is None and refusal(rd, paths(0, 0, aoff=1024), 5) is None
    assert refusal(rd, paths(0, 3, lpresent=0), 5) is None and refusal(rd, paths(3, 0, apresent=0), 5) is None
    msg = refusal(rd, paths(0, 16, aoff=64), 5)
    assert msg and "area-light-table buffer" in msg, msg
    msg = refusal(rd, paths(2, 3, aoff=8), 5)
    assert msg and "area-light-table" in msg and "16" in msg, msg
    msg = refusal(rd, paths(2, 5, rad=(0x38000, 4096, 256)), 5)      # radiance begins inside area record 4
    assert msg and "radiance" in msg and "area-light-table" in msg and "overlap" in msg, msg
    assert refusal(rd, paths(2, 4, rad=(0x38000, 4096, 256)), 5) is None
    msg = refusal(rd, paths(5, 2, rad=(0x30000, 4096, 256)), 5)      # ... and inside punctual record 4
    assert msg and "radiance" in msg and "light-table" in msg and "overlap" in msg, msg
    assert refusal(rd, paths(0, 0, rad=(0x38000, 4096, 0)), 5) is None           # an empty table overlaps nothing
    src = open(os.path.join(ROOT, "radiance-ray-tracing_amd", "csrc", "rdx_runtime.cpp")).read()
    for name in ('"area-light"', '"area-light-table"', '"randoms"'):
        assert name in src[src.index('extern "C" int rdx_area_light_hits'):], name


# ---- emitted_area on hand-made rows ----------------------------------------------------------------------------------------------------
ORIGIN = np.zeros((1, 3), F)
UP = np.array([0.0, 1.0, 0.0], F)
DOWN = np.array([0.0, -1.0, 0.0], F)


def quad_down(rd, **kw):
    """the lamp of the convergence test: 2 x 2 at y = 1 over the origin, facing down: n = cross(edgeU, edgeV) = (0, -4, 0) points out
    of the emitting face, so g = -(n . L) = 4 L.y > 0 for a receiver below (L.y > 0)"""
    return rd.QuadLight((-1, 1, -1), (2, 0, 0), (0, 0, 2), (1.0, 2.0, 0.5), **kw)


def test_emitted_area_by_hand(mods):
    _, rd, _ = mods
    q = quad_down(rd)
    # the centre of the quad, straight up: p = (0, 1, 0), d2 = 1, g = -(n . L) = 4, E = radiance * 4, tmax = 0.999
    e = ar.emitted_area(q, ORIGIN, 0.5, 0.5, UP)
    assert not e["dark"][0] and np.array_equal(e["p"][0], np.array([0, 1, 0], F)) and e["d2"][0] == 1 and e["g"][0] == 4
    assert np.array_equal(e["E"][0], np.array([4.0, 8.0, 2.0], F)) and sh.bits(e["tmax"][0]) == sh.bits(F(0.999))
    assert all(e[k].dtype == F for k in ("E", "tmax", "d2", "g", "p", "w"))
    # d2 == 0: the sampled point IS the hit
    e = ar.emitted_area(q, np.array([[0, 1, 0]], F), 0.5, 0.5, UP)
    assert e["dark"][0] and e["d2"][0] == 0
    # g exactly 0: a hit in the emitter's plane
    e = ar.emitted_area(q, np.array([[5, 1, 0]], F), 0.5, 0.5, np.array([-1.0, 0.0, 0.0], F))
    assert e["dark"][0] and e["g"][0] == 0 and e["d2"][0] == 25
    two = quad_down(rd, two_sided=True)
    assert ar.emitted_area(two, np.array([[5, 1, 0]], F), 0.5, 0.5, np.array([-1.0, 0.0, 0.0], F))["dark"][0]       # fabsf(0) is not > 0
    # the back face: dark one-sided, lit two-sided with the bits of the front at the mirrored point
    front = ar.emitted_area(q, np.array([[0.25, -1, 0.5]], F), 0.25, 0.75, np.array([-0.6, 0.8, 0.0], F))
    back = ar.emitted_area(q, np.array([[0.25, 3, 0.5]], F), 0.25, 0.75, np.array([-0.6, -0.8, 0.0], F))
    back2 = ar.emitted_area(two, np.array([[0.25, 3, 0.5]], F), 0.25, 0.75, np.array([-0.6, -0.8, 0.0], F))
    assert not front["dark"][0] and back["dark"][0] and back["g"][0] < 0 and not back2["dark"][0]
    assert back2["d2"][0] == front["d2"][0] and np.array_equal(sh.bits(back2["E"]), sh.bits(front["E"])) and sh.bits(back2["tmax"][0]) == sh.bits(front["tmax"][0])
    assert np.array_equal(sh.bits(ar.emitted_area(two, np.array([[0.25, -1, 0.5]], F), 0.25, 0.75, np.array([-0.6, 0.8, 0.0], F))["E"]), sh.bits(front["E"]))
    # an unknown type is dark everywhere, whatever the flags
    for t in (2, 3, 0xffffffff):
        bad = np.array(two).copy()
        bad["type"] = t
        assert ar.emitted_area(bad, np.array([[0, 0, 0], [0.25, 3, 0.5]], F), 0.5, 0.5, UP)["dark"].all(), t
    # a degenerate emitter (edgeU parallel to edgeV): n = 0, g = 0, dark from everywhere, also two-sided
    flat = rd.QuadLight((-1, 1, -1), (2, 0, 0), (4, 0, 0), (1, 1, 1), two_sided=True)
    assert ar.emitted_area(flat, ORIGIN, 0.5, 0.5, UP)["dark"][0]
    # NaN and infinite fields: dark (d2 not finite, or g not > 0)
    for field, val in (("corner", np.nan), ("corner", np.inf), ("corner", 3e20), ("edgeU", np.nan), ("edgeV", np.inf)):
        bad = np.array(q).copy()
        bad[field][1] = val
        assert ar.emitted_area(bad, ORIGIN, 0.5, 0.5, UP)["dark"][0], (field, val)
    # d2 is (x * x + y * y) + z * z in this order: with x * x = 2^24 and y * y = z * z = 1 the first sum loses y * y, the second z * z
    e = ar.emitted_area(rd.QuadLight((4096, 1, 1), (0, 0, 1), (1, 0, 0), (1, 1, 1)), ORIGIN, 0.0, 0.0, UP)
    assert e["d2"][0] == F(2.0 ** 24)
    e = ar.emitted_area(rd.QuadLight((1, 1, 4096), (0, 0, 1), (1, 0, 0), (1, 1, 1)), ORIGIN, 0.0, 0.0, UP)
    assert e["d2"][0] == F(2.0 ** 24 + 2.0)
    # p is (corner + edgeU * u) + edgeV * v with every operation rounded: 1 + 2^-24 is lost in the first sum, then 2^-24 again
    e = ar.emitted_area(rd.QuadLight((1, 1, 0), (2.0 ** -24, 0, 1), (2.0 ** -24, 0, 0), (1, 1, 1)), ORIGIN, 1.0, 1.0, UP)
    assert e["p"][0, 0] == 1
    # rows are independent
    above = np.array([[0, 0, 0], [1, -2, 3], [-5, 3.5, 9]], F)
    u, v = np.array([0.1, 0.9, 0.4], F), np.array([0.7, 0.8, 0.2], F)
    Ls = np.array([[0, 1, 0], [0, 1, 0], [0, -1, 0]], F)
    e = ar.emitted_area(q, above, u, v, Ls)
    for i in range(3):
        ei = ar.emitted_area(q, above[i:i + 1], u[i], v[i], Ls[i])
        assert e["dark"][i] == ei["dark"][0] and np.array_equal(sh.bits(e["E"][i]), sh.bits(ei["E"][0])) and sh.bits(e["tmax"][i]) == sh.bits(ei["tmax"][0])
    assert e["dark"].tolist() == [False, False, True]


def test_the_triangle_fold(mods):
    _, rd, _ = mods
    t = rd.TriangleLight((-1, 1, -1), (2, 0, 0), (0, 0, 2), (1, 1, 1))
    q = quad_down(rd)
    # u + v exactly 1: not folded
    e = ar.emitted_area(t, ORIGIN, 0.25, 0.75, UP)
    assert e["u"][0] == F(0.25) and e["v"][0] == F(0.75) and np.array_equal(e["p"][0], np.array([-0.5, 1, 0.5], F))
    # one ulp above: u + v = 1 + 2^-23, the next float above 1, and the pair is folded to (1 - u, 1 - v)
    v1 = F(0.75 + 2.0 ** -23)
    assert F(F(0.25) + v1) == np.nextafter(F(1.0), F(2.0))
    e = ar.emitted_area(t, ORIGIN, 0.25, v1, UP)
    assert e["u"][0] == F(0.75) and e["v"][0] == F(0.25 - 2.0 ** -23) and np.array_equal(e["p"][0], np.array([0.5, 1, F(-1.0) + F(2.0) * e["v"][0]], F))
    # a sum that is above 1 in exact arithmetic but rounds to 1.0f is NOT folded: the rule is the float32 sum's.  0.25 + (0.75 +
    # 2^-24) is a tie that rounds to even
    v0 = np.nextafter(F(0.75), F(1))
    assert F(F(0.25) + v0) == F(1.0)
    e = ar.emitted_area(t, ORIGIN, 0.25, v0, UP)
    assert e["u"][0] == F(0.25) and e["v"][0] == v0
    u2 = F(2.0 ** -26)
    assert F(u2 + F(1.0)) == F(1.0)
    e = ar.emitted_area(t, ORIGIN, u2, 1.0, UP)
    assert e["u"][0] == u2 and e["v"][0] == F(1.0)
    # the quad never folds, and the triangle's g is half the quad's at the same point and direction
    eq = ar.emitted_area(q, ORIGIN, 0.9, 0.8, UP)
    assert eq["u"][0] == F(0.9) and eq["v"][0] == F(0.8)
    et, eq = ar.emitted_area(t, ORIGIN, 0.25, 0.5, UP), ar.emitted_area(q, ORIGIN, 0.25, 0.5, UP)
    assert et["g"][0] == F(eq["g"][0] * F(0.5)) == 2 and np.array_equal(et["p"], eq["p"])
    # all folded pairs lie in the triangle
    rng = np.random.default_rng(5)
    u, v = rng.random(4096).astype(F), rng.random(4096).astype(F)
    e = ar.emitted_area(t, np.zeros((4096, 3), F), u, v, UP)
    assert ar.in_emitter(t, e["u"], e["v"]).all() and ((u + v).astype(F) > 1).sum() > 1024


# ---- the estimator converges to the form factor -------------------------------------------------------------------------------------
def _estimate(light, frames, pixels, depth, stream):
    """per sample (N . L) * g / d2 for the receiver at the origin with normal +y, float64 on the float32 random pairs; L is
    numpy's w / |w| (the device's differs from it by 2^-20, far below the standard error)"""
    r = ar.randoms_of(frames, pixels, depth, stream)["xyz"]
    n = r.shape[0]
    e = ar.emitted_area(light, np.zeros((n, 3), F), r[:, 0], r[:, 1], UP)         # p, w and the fold; its g is for L = UP and is not used
    w = e["w"].astype(np.float64)
    d2 = (w * w).sum(1)
    L = w / np.sqrt(d2)[:, None]
    eu, ev = np.ascontiguousarray(light["edgeU"], np.float64), np.ascontiguousarray(light["edgeV"], np.float64)
    g = -(L @ np.cross(eu, ev)) * (0.5 if int(light["type"]) == ar.TRIANGLE else 1.0)
    assert (g > 0).all()
    return L[:, 1] * g / d2


def test_the_estimator_converges_to_the_form_factor(mods):
    """receiver at the origin, normal +y; the 2 x 2 quad at height 1, facing down; frame 7, pixels 0 .. 65535, depth 0.  The integral
    of cos cos / r^2 over the quad is 4 a / sqrt(a^2 + h^2) atan(a / sqrt(a^2 + h^2)) with a = h = 1: 1.74084.  The mean of the
    one-sample estimator must lie within 4 standard errors (computed from the same samples) of it: as one quad on stream 0, and as
    two RDX_AREA_TRIANGLE records on streams 1 and 2, summed.  Deterministic: the keys are fixed.
    Measured: quad 1.73887, s.e. 0.0034; triangles 1.73946 summed, s.e. 0.0017 each."""
    _, rd, _ = mods
    a = h = 1.0
    s = a / np.sqrt(a * a + h * h)
    exact = 4.0 * s * np.arctan(s)
    assert abs(exact - 1.74084) < 1e-5
    pixels = np.arange(65536, dtype=np.uint32)
    x = _estimate(quad_down(rd), 7, pixels, 0, 0)
    mean, se = x.mean(), x.std(ddof=1) / np.sqrt(x.shape[0])
    print("quad: mean %.5f, s.e. %.5f, exact %.5f" % (mean, se, exact))
    assert abs(mean - exact) <= 4.0 * se and 0.001 < se < 0.01
    # the quad split along its diagonal from corner + edgeU to corner + edgeV: (corner, edgeU, edgeV) and the opposite corner with
    # the edges reversed, which keeps n's direction
    t1 = rd.TriangleLight((-1, 1, -1), (2, 0, 0), (0, 0, 2), (1, 1, 1))
    t2 = rd.TriangleLight((1, 1, 1), (-2, 0, 0), (0, 0, -2), (1, 1, 1))
    x1, x2 = _estimate(t1, 7, pixels, 0, 1), _estimate(t2, 7, pixels, 0, 2)
    m1, m2 = x1.mean(), x2.mean()
    se1, se2 = x1.std(ddof=1) / np.sqrt(x1.shape[0]), x2.std(ddof=1) / np.sqrt(x2.shape[0])
    x12 = x1 + x2                                   # what a hit sums: both records, each on its stream, under the same key
    se12 = x12.std(ddof=1) / np.sqrt(x12.shape[0])
    print("triangles: means %.5f + %.5f = %.5f, s.e. %.5f, %.5f (of the sum %.5f)" % (m1, m2, m1 + m2, se1, se2, se12))
    assert abs(x12.mean() - exact) <= 4.0 * se12 and 0.0005 < se1 < 0.005 and 0.0005 < se2 < 0.005

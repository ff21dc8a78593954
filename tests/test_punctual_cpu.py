"""CPU suite: the ABI of rdx_punctual_light_hits / rdx_trace_paths_punctual (point and spot lights from a caller-owned light table),
the argument checks of their Python wrappers, the rows the two calls hand to the range rule, rd.SpotCone, and
punctual_cases.emitted -- the numpy restatement of what a table record emits at a point -- on hand-made rows, before
test_gpu_punctual.py holds the calls to it."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import punctual_cases as pu
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
    want = dict(position=0, type=12, direction=16, range=28, color=32, _0=44, coneScale=48, coneOffset=52, _1=56, _2=60)
    assert rd.PUNCTUAL_LIGHT_DTYPE.itemsize == C.sizeof(_lib.rdx_punctual_light) == 64
    for name, off in want.items():
        assert rd.PUNCTUAL_LIGHT_DTYPE.fields[name][1] == off == getattr(_lib.rdx_punctual_light, name).offset, name
    assert rd.PUNCTUAL_LIGHT_DTYPE.fields["type"][0] == np.dtype("<u4") and rd.PUNCTUAL_LIGHT_DTYPE.fields["position"][0].shape == (3,)
    assert (rd.LIGHT_DIRECTIONAL, rd.LIGHT_POINT, rd.LIGHT_SPOT, rd.MAX_PATH_LIGHTS) == (0, 1, 2, 16)
    hdr = open(os.path.join(ROOT, "include", "rdx.h")).read()
    for text in ("#define RDX_LIGHT_DIRECTIONAL 0u", "#define RDX_LIGHT_POINT       1u", "#define RDX_LIGHT_SPOT        2u", "#define RDX_MAX_PATH_LIGHTS 16u",
                 "typedef struct rdx_punctual_light {"):
        assert text in hdr, text
    types = open(os.path.join(ROOT, "radiance-ray-tracing_amd", "csrc", "rdx_types.h")).read()
    assert "struct PunctualLight" in types and "sizeof(PunctualLight) == 64" in types


def test_the_library_exports_the_calls(mods):
    _lib, rd, _ = mods
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "rdx.h")).read()
    P, Z, U = C.c_void_p, C.c_size_t, C.c_uint32
    want = {"rdx_punctual_light_hits": (C.c_int, [P, Z, P, Z, U, P, Z, P, Z, P, Z]),
            "rdx_trace_paths_punctual": (C.c_int, [P, P, Z, P, Z, U, U, P, Z, U, C.POINTER(_lib.rdx_shading_buffers), P, Z, C.POINTER(U)])}
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig and getattr(L, name).argtypes == sig[1] and getattr(L, name).restype is C.c_int, name
        assert re.search(r"\b%s\(rdx_buffer " % name, hdr), name
    assert hdr.index("rdx_trace_paths_punctual(") > hdr.index("rdx_trace_paths_lights(")
    build = open(os.path.join(ROOT, "radiance-ray-tracing_amd", "build.py")).read()
    assert '"punctual.hip"' in build and '"punctual.h"' in build
    for name in ("PunctualLightHits", "PunctualLightHitsTorch", "TracePunctualPaths", "TracePunctualPathsTorch", "SpotCone"):
        assert callable(getattr(rd, name)), name
    cxx = open(os.path.join(ROOT, "include", "radiance.h")).read()
    assert re.search(r"\bPunctualLightHits\(", cxx) and re.search(r"\bTracePunctualPaths\(", cxx)
    assert "rdx_punctual_light_hits(" in cxx and "rdx_trace_paths_punctual(" in cxx


def test_an_uninitialised_library_refuses_and_names_the_call(mods):
    """(a fresh process: the suite's other tests may have initialised the library in this one)"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import rrt_amd\n"
            "from radiance_ray_tracing_amd import _lib\n"
            "L = _lib.lib()\n"
            "rc = L.rdx_punctual_light_hits(None, 0, None, 0, 0, None, 0, None, 0, None, 0)\n"
            "print(rc, _lib.last_error())\n"
            "rc = L.rdx_trace_paths_punctual(None, None, 0, None, 0, 0, 4, None, 0, 3, None, None, 0, None)\n"
            "print(rc, _lib.last_error())\n") % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == 2, out.stdout
    for line, name in zip(lines, ("rdx_punctual_light_hits", "rdx_trace_paths_punctual")):
        rcode, msg = line.split(None, 1)
        assert int(rcode) < 0 and name in msg and "rdx_init" in msg, out.stdout


def test_the_wrappers_refuse_wrong_arguments_before_the_library(mods, monkeypatch):
    """no wrapper reaches the library with light_count 17, a table of a wrong dtype or shape, or an argument of the wrong kind: the
    library is not initialised here, and a call that got through would fail with its message instead of the wrapper's"""
    _lib, rd, _ = mods
    reached = []
    real = _lib.lib

    class Spy:
        def __getattr__(self, name):
            if name in ("rdx_punctual_light_hits", "rdx_trace_paths_punctual"):
                reached.append(name)
            return getattr(real(), name)
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    buf = rd.Buffer(1234, 4096)
    sb = rd.ShadingBuffers(buf, buf, buf, None, buf, buf)
    bad = [dict(tlas=None), dict(rays=7), dict(keys=np.zeros(4)), dict(lights=None), dict(lights=np.zeros(2, rd.PUNCTUAL_LIGHT_DTYPE)), dict(scene_buffers=(buf, buf)),
           dict(radiance=np.zeros(4)), dict(n=-1), dict(n=2.5), dict(max_depth=-1), dict(max_depth="4"),
           dict(light_count=-1), dict(light_count=17), dict(light_count=2.5), dict(light_count="3"), dict(light_count=True), dict(light_count=None)]
    for kw in bad:
        a = dict(tlas=buf, rays=buf, keys=buf, n=4, max_depth=4, lights=buf, light_count=3, scene_buffers=sb, radiance=buf)
        a.update(kw)
        with pytest.raises(rd.RadianceError, match="TracePunctualPaths"):
            rd.TracePunctualPaths(a.pop("tlas"), a.pop("rays"), a.pop("keys"), a.pop("n"), a.pop("max_depth"), a.pop("lights"), a.pop("light_count"),
                                  a.pop("scene_buffers"), **a)
    for kw in (dict(rays=None), dict(materials=7), dict(lights=np.zeros((2, 16), F)), dict(index=-1), dict(index=1.5), dict(index=True), dict(lit=7),
               dict(shadow=7)):
        a = dict(rays=buf, materials=buf, n=4, lights=buf, index=1, lit=buf, shadow=buf)
        a.update(kw)
        with pytest.raises(rd.RadianceError, match="PunctualLightHits"):
            rd.PunctualLightHits(a.pop("rays"), a.pop("materials"), a.pop("n"), a.pop("lights"), a.pop("index"), **a)
    import torch
    r, k, m = torch.zeros((5, 8), dtype=torch.float32), torch.zeros((5, 4), dtype=torch.int32), torch.zeros((5, 16), dtype=torch.float32)
    t3 = torch.zeros((3, 16), dtype=torch.float32)
    for rays in (r, r.numpy(), None):       # CPU tensors, arrays, nothing: refused before any CUDA call
        with pytest.raises(rd.RadianceError, match="TracePunctualPathsTorch: (rays|lights)"):
            rd.TracePunctualPathsTorch(buf, rays, k, 4, t3, sb)
        with pytest.raises(rd.RadianceError, match="PunctualLightHitsTorch: (rays|lights)"):
            rd.PunctualLightHitsTorch(rays, m, t3, 0)
    # a table of a wrong dtype or shape, or no tensor at all: the table is looked at first, so the refusal names it
    for table in (t3.double(), t3[:, :15], t3.reshape(-1), torch.zeros((3, 32))[:, ::2], t3.numpy(), None):
        with pytest.raises(rd.RadianceError, match="TracePunctualPathsTorch: lights"):
            rd.TracePunctualPathsTorch(buf, r, k, 4, table, sb)
        with pytest.raises(rd.RadianceError, match="PunctualLightHitsTorch: lights"):
            rd.PunctualLightHitsTorch(r, m, table, 0)
    assert not reached


def test_spot_cone(mods):
    _, rd, _ = mods
    scale, offset = rd.SpotCone(np.radians(15.0), np.radians(35.0))
    assert isinstance(scale, F) and isinstance(offset, F)
    ci, co = F(np.cos(F(np.radians(15.0)))), F(np.cos(F(np.radians(35.0))))
    assert scale == F(1.0) / F(ci - co) and offset == F(F(-co) * scale)
    assert abs(float(scale) - 1.0 / (np.cos(np.radians(15.0)) - np.cos(np.radians(35.0)))) < 1e-5 * float(scale)
    # f = cos * scale + offset is 0 at the outer angle and 1 at the inner one, to rounding
    assert abs(float(co) * float(scale) + float(offset)) < 1e-6 and abs(float(ci) * float(scale) + float(offset) - 1.0) < 1e-6
    # inner == outer (and inner > outer): the difference is held to 0.001
    scale, offset = rd.SpotCone(0.5, 0.5)
    assert scale == F(1.0) / F(0.001) and offset == F(F(-np.cos(F(0.5))) * scale)
    assert rd.SpotCone(0.6, 0.5)[0] == scale
    # exact cosines: acos(0.75) / acos(0.5) round to (4, -2) within an ulp of the cosines
    s, o = rd.SpotCone(np.arccos(0.75), np.arccos(0.5))
    assert abs(float(s) - 4.0) < 1e-5 and abs(float(o) + 2.0) < 1e-5


def refusal(rd, rows, first_out, n=8):
    return rd.DebugCheckRanges(rows, first_out, n)


def test_the_rows_of_the_two_calls(mods):
    """the rows rdx_punctual_light_hits and rdx_trace_paths_punctual build (csrc/rdx_runtime.cpp), through the seam of the one rule:
    a misaligned light offset, a table that overruns its buffer, `lit` / radiance overlapping the light"""
    _, rd, _ = mods
    n, base = 8, 0x10000
    hits = lambda light_off, light_size=4 * 64, lit=(0x50000, 16 * 8, 0), light_at=0x30000: [
        ("ray", base, 32 * n, 0, 32 * n, 16, 1), ("material-record", 0x20000, 64 * n, 0, 64 * n, 16, 1), ("light", light_at, light_size, light_off, 64, 16, 1),
        ("lit", lit[0], lit[1], lit[2], 16 * n, 16, 1), ("shadow-ray", 0x60000, 32 * n, 0, 32 * n, 16, 1)]
    assert refusal(rd, hits(64), 3) is None and refusal(rd, hits(192), 3) is None
    msg = refusal(rd, hits(72), 3)
    assert msg and "light" in msg and "16" in msg and "72" in msg, msg
    msg = refusal(rd, hits(256), 3)           # record 4 of a table of 4
    assert msg and "light buffer" in msg, msg
    msg = refusal(rd, hits(200, light_size=256), 3)   # misaligned AND past the end: the offset is named first
    assert msg and "multiple" in msg, msg
    msg = refusal(rd, hits(64, lit=(0x30000, 4096, 112)), 3)          # lit begins inside record 1
    assert msg and "lit" in msg and "light" in msg and "overlap" in msg, msg
    assert refusal(rd, hits(64, lit=(0x30000, 4096, 128)), 3) is None        # ... and right behind it
    paths = lambda count, off=0, size=16 * 64, rad=(0x50000, 16 * n, 0): [
        ("ray", base, 32 * n, 0, 32 * n, 16, 1), ("key", 0x20000, 16 * n, 0, 16 * n, 16, 1), ("light-table", 0x30000, size, off, 64 * count, 16, 1),
        ("scene (SceneProperties)", 0x40000, 176, 0, 176, 4, 1), ("radiance", rad[0], rad[1], rad[2], 16 * n, 16, 1)]
    assert refusal(rd, paths(16), 4) is None and refusal(rd, paths(0, off=1024), 4) is None
    msg = refusal(rd, paths(16, off=64), 4)
    assert msg and "light-table buffer" in msg, msg
    msg = refusal(rd, paths(3, off=8), 4)
    assert msg and "light-table" in msg and "16" in msg, msg
    msg = refusal(rd, paths(5, rad=(0x30000, 4096, 256)), 4)      # radiance begins inside record 4
    assert msg and "radiance" in msg and "light-table" in msg and "overlap" in msg, msg
    assert refusal(rd, paths(4, rad=(0x30000, 4096, 256)), 4) is None
    assert refusal(rd, paths(0, rad=(0x30000, 4096, 0)), 4) is None           # an empty table overlaps nothing


# ---- emitted on hand-made rows ------------------------------------------------------------------------------------------------------
ORIGIN = np.zeros((1, 3), F)
UP = np.array([0.0, 1.0, 0.0], F)


def test_emitted_range_edges(mods):
    _, rd, _ = mods
    color = (1.0, 2.0, 0.5)
    e = pu.emitted(pu.light(rd, pu.POINT, (0, 0, 0), range=0.5, color=color), ORIGIN, UP)
    assert e["dark"][0] and e["d2"][0] == 0          # d2 == 0: the light sits on the point
    e = pu.emitted(pu.light(rd, pu.POINT, (0, 0.5, 0), range=0.5, color=color), ORIGIN, UP)
    assert e["dark"][0] and e["d2"][0] == F(0.25)    # d2 == range * range exactly: !(d2 < range * range)
    e = pu.emitted(pu.light(rd, pu.POINT, (0, 0.5, 0), range=0.0, color=color), ORIGIN, UP)
    assert not e["dark"][0] and np.array_equal(e["E"][0], np.array(color, F) * F(4.0)) and e["tmax"][0] == F(0.5)     # unlimited
    # one ulp inside: y = 0.5 - 2^-25, d2 = y * y = 0.25 - 2^-25 (+ 2^-50, rounded away), att = 1 / d2 = 4 + 2^-21, tmax = sqrt(d2) = y
    y = np.nextafter(F(0.5), F(0))
    e = pu.emitted(pu.light(rd, pu.POINT, (0, y, 0), range=0.5, color=color), ORIGIN, UP)
    assert not e["dark"][0] and e["d2"][0] == F(0.25 - 2.0 ** -25)
    assert np.array_equal(sh.bits(e["E"][0]), sh.bits(np.array(color, F) * F(4.0 + 2.0 ** -21)))
    assert e["tmax"][0] == y and e["E"].dtype == F and e["tmax"].dtype == F
    # ... and one ulp outside
    e = pu.emitted(pu.light(rd, pu.POINT, (0, np.nextafter(F(0.5), F(1)), 0), range=0.5, color=color), ORIGIN, UP)
    assert e["dark"][0]
    # a position at infinity, a NaN position: dark
    for y in (np.inf, 3e20, np.nan):
        assert pu.emitted(pu.light(rd, pu.POINT, (0, y, 0), color=color), ORIGIN, UP)["dark"][0], y
    # d2 is (x * x + y * y) + z * z in this order: with x * x = 2^24 and y * y = z * z = 1 the first sum loses y * y, the second z * z
    e = pu.emitted(pu.light(rd, pu.POINT, (4096.0, 1.0, 1.0)), ORIGIN, UP)
    assert e["d2"][0] == F(2.0 ** 24)
    e = pu.emitted(pu.light(rd, pu.POINT, (1.0, 1.0, 4096.0)), ORIGIN, UP)
    assert e["d2"][0] == F(2.0 ** 24 + 2.0)


def test_emitted_cone_edges(mods):
    """a spot whose axis points down, cosInner 0.75, cosOuter 0.5: coneScale = 1 / 0.25 = 4, coneOffset = -0.5 * 4 = -2, all exact.
    With S = (0, -1, 0) the cosine is L.y"""
    _, rd, _ = mods
    spot = pu.light(rd, pu.SPOT, (0, 0.5, 0), (0, -1, 0), 0.0, (1.0, 2.0, 0.5), (4.0, -2.0))
    S = np.array([0.0, -1.0, 0.0], F)
    at = lambda c: pu.emitted(spot, ORIGIN, np.array([np.sqrt(1.0 - c * c), c, 0.0], F), S)
    e = at(0.5)
    assert e["f"][0] == 0 and e["dark"][0]                     # exactly 0 at cosOuter: dark
    e = at(0.75)
    assert e["f"][0] == 1 and not e["dark"][0]                 # exactly 1 at cosInner: the point light's E
    assert np.array_equal(sh.bits(e["E"][0]), sh.bits(np.array([4.0, 8.0, 2.0], F)))
    e = at(1.0)
    assert e["f"][0] == 1 and not e["dark"][0]                 # clamped inside the inner cone
    e = at(0.625)                                              # halfway: f = 0.5, E = E * (f * f)
    assert e["f"][0] == F(0.5) and not e["dark"][0] and np.array_equal(e["E"][0], np.array([1.0, 2.0, 0.5], F))
    e = at(np.nextafter(F(0.5), F(1)))
    assert 0 < e["f"][0] < 1e-6 and not e["dark"][0]           # one ulp inside the outer cone: lit, barely
    assert at(0.25)["dark"][0] and at(-1.0)["dark"][0]         # outside, and behind the spot
    # a ranged spot: the range rule comes first
    ranged = spot.copy()
    ranged["range"] = 0.5
    assert pu.emitted(ranged, ORIGIN, np.array([0.0, 1.0, 0.0], F), S)["dark"][0]


def test_emitted_types(mods):
    _, rd, _ = mods
    above = np.array([[0, 0, 0], [1, 2, 3], [-5, 0.5, 9]], F)
    e = pu.emitted(pu.light(rd, 3, (0, 0.25, 0), color=(1, 1, 1)), above, UP)
    assert e["dark"].all()                                     # an unknown type is dark everywhere
    assert pu.emitted(pu.light(rd, 0xffffffff, (0, 0.25, 0)), above, UP)["dark"].all()
    e = pu.emitted(pu.light(rd, pu.DIRECTIONAL, (7, 7, 7), (0.3, -1, 0.2), 0.001, (5.0, 4.5, 4.0)), above, UP)
    assert not e["dark"].any() and (e["tmax"] == F(1000.0)).all() and np.array_equal(e["E"], np.tile(np.array([5.0, 4.5, 4.0], F), (3, 1)))
    # rows are independent
    pt = pu.light(rd, pu.POINT, (0.5, 4.0, -1.0), range=6.0, color=(3.0, 2.0, 1.0))
    e = pu.emitted(pt, above, UP)
    for i in range(3):
        ei = pu.emitted(pt, above[i:i + 1], UP)
        assert e["dark"][i] == ei["dark"][0] and np.array_equal(sh.bits(e["E"][i]), sh.bits(ei["E"][0])) and e["tmax"][i] == ei["tmax"][0]
    assert e["dark"].tolist() == [False, False, True]


def test_tables(mods):
    _, rd, _ = mods
    import light_paths_cases as lp
    sp = lp.five_lights(rd)
    t = pu.directional_table(rd, sp)
    assert t.shape == (5,) and not t["type"].any() and np.array_equal(t["direction"][3], np.array(sp["lights"][3]["direction"][:3]))
    m = pu.mixed_table(rd, (-3, 0, -3), (3, 6, 3), sp, 7)
    assert m.shape == (rd.MAX_PATH_LIGHTS,) and m["type"][:5].tolist() == [1, 2, 0, 3, 1] and m["range"][0] > 0 and m["range"][4] == 0
    assert set(m["type"].tolist()) == {0, 1, 2, 3} and (m["type"] == 3).sum() == 1
    assert m.tobytes() == pu.mixed_table(rd, (-3, 0, -3), (3, 6, 3), sp, 7).tobytes()

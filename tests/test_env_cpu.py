"""CPU suite: the ABI of the environment calls (rdx_env_table_size, rdx_env_build, rdx_env_light_hits, rdx_env_lookup,
rdx_trace_paths_env), the table's layout, the argument checks of the wrappers of radiance_ray_tracing_amd.env, env.ProceduralSky,
the rule that keeps the random streams apart, env_cases.sampled_env -- the numpy restatement of what the environment emits for a
random triple -- on hand-made images, and the convergence of the estimator to a quadrature of the image, before test_gpu_env.py
holds the calls to it."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import area_cases as ar
import env_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def mods(built):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import _lib, env, rd
    return _lib, rd, env


def table_of(image):
    """the table a device would build, with numpy's rowCos"""
    H, W = image.shape[:2]
    return ec.parts(ec.build_table(image, ec.row_cos(H)), W, H)


def randoms(n, frame=7, depth=0, stream=0):
    r = ar.pcg3d(np.full(n, frame, np.uint32), np.arange(n, dtype=np.uint32), ar.stream_word(np.full(n, depth), stream))
    return r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy()


# ---- layout, symbols, header -------------------------------------------------------------------------------------------------------------
def test_layout_and_size_function(mods):
    _lib, rd, env = mods
    L = _lib.lib()
    for W, H in ((1, 1), (8, 4), (37, 19), (64, 32), (257, 3), (1024, 512), (16384, 1), (16384, 8192), (3, 8192)):
        lay, mine = env.TableLayout(W, H), ec.layout(W, H)
        assert lay["size"] == mine["size"] == L.rdx_env_table_size(W, H) == env.TableSize(W, H), (W, H)
        assert (lay["rowCos"], lay["C"], lay["M"]) == (mine["rowCos"], mine["C"], mine["M"]) and lay["header"] == 0
        assert all(lay[k] % 16 == 0 for k in lay)
        assert lay["C"] - 64 >= 4 * (H + 1) and lay["M"] - lay["C"] >= 4 * W * H and lay["size"] - lay["M"] >= 8 * H
        assert lay["size"] < 64 + 4 * (H + 1) + 4 * W * H + 8 * H + 48
    for W, H in ((0, 1), (1, 0), (16385, 1), (1, 8193), (0xffffffff, 0xffffffff)):
        assert L.rdx_env_table_size(W, H) == 0 == env.TableSize(W, H) and env.TableLayout(W, H) is None, (W, H)
    assert env.HEADER_DTYPE == ec.HEADER_DTYPE and env.HEADER_DTYPE.fields["total"][1] == 32 and env.HEADER_DTYPE.fields["wmax"][1] == 16
    assert (env.MAGIC, env.VERSION, env.MAX_WIDTH, env.MAX_HEIGHT, env.MAX_STREAM) == (ec.MAGIC, 1, 16384, 8192, 0xfffe)
    unit = open(os.path.join(ROOT, "radiance-ray-tracing_amd", "csrc", "env.h")).read()
    assert "sizeof(EnvHeader) == 64" in unit and "0x%08xu" % ec.MAGIC in unit


def test_the_library_exports_the_calls(mods):
    _lib, rd, env = mods
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "rdx.h")).read()
    P, Z, U = C.c_void_p, C.c_size_t, C.c_uint32
    want = {"rdx_env_table_size": (Z, [U, U]),
            "rdx_env_build": (C.c_int, [P, Z, U, U, P, Z]),
            "rdx_env_light_hits": (C.c_int, [P, Z, P, Z, U, P, Z, P, Z, U, U, P, Z, U, P, Z, P, Z, P, Z]),
            "rdx_env_lookup": (C.c_int, [P, Z, U, P, Z, P, Z, U, U, P, Z]),
            "rdx_trace_paths_env": (C.c_int, [P, P, Z, P, Z, U, U, P, Z, U, P, Z, U, P, Z, P, Z, U, U, C.POINTER(_lib.rdx_shading_buffers), P, Z, C.POINTER(U)])}
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig and getattr(L, name).argtypes == sig[1] and getattr(L, name).restype is sig[0], name
        assert re.search(r"\b%s\(" % name, hdr), name
    assert hdr.index("rdx_trace_paths_env(rdx_buffer") > hdr.index("rdx_trace_paths_area(rdx_buffer")
    for text in ("X = min((uint64)((double)u * (double)total), total - 1)", "fy = ((float)(X - lo) + 0.5f) / (float)rowSum",
                 "q = 0 where w == 0, else max(1, min(65535, (uint32)(w * (65535.0f / wmax))))", "tmax = 1000.0f",
                 "E = image[y][x].rgb * ((((float)total / (float)q) * twoPiOverW) * (rowCos[y] - rowCos[y + 1]))"):
        assert text in hdr, text
    from radiance_ray_tracing_amd import build
    assert "env.hip" in build.SOURCES and "env.h" in build.HEADERS
    for name in ("TableSize", "BuildEnvironment", "BuildEnvironmentTorch", "CreateEnvironment", "EnvLightHits", "EnvLightHitsTorch", "EnvLookup", "EnvLookupTorch",
                 "TraceEnvPaths", "TraceEnvPathsTorch", "ProceduralSky", "Environment"):
        assert callable(getattr(env, name)), name
    cxx = open(os.path.join(ROOT, "include", "radiance.h")).read()
    for name, sym in (("EnvTableSize", "rdx_env_table_size"), ("BuildEnvironment", "rdx_env_build"), ("EnvLightHits", "rdx_env_light_hits"),
                      ("EnvLookup", "rdx_env_lookup"), ("TraceEnvPaths", "rdx_trace_paths_env")):
        assert re.search(r"\b%s\(" % name, cxx) and sym + "(" in cxx, name
    emit = open(os.path.join(ROOT, "radiance-ray-tracing_amd", "csrc", "light_emit.h")).read()
    assert "bool env_emit(" in emit and "env_emit(" in open(os.path.join(ROOT, "radiance-ray-tracing_amd", "csrc", "path_shade.h")).read()


def test_an_uninitialised_library_refuses_and_names_the_call(mods):
    """(a fresh process: the suite's other tests may have initialised the library in this one)"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import rrt_amd\n"
            "from radiance_ray_tracing_amd import _lib\n"
            "L = _lib.lib()\n"
            "print(L.rdx_env_build(None, 0, 4, 4, None, 0), _lib.last_error())\n"
            "print(L.rdx_env_light_hits(None, 0, None, 0, 0, None, 0, None, 0, 4, 4, None, 0, 0, None, 0, None, 0, None, 0), _lib.last_error())\n"
            "print(L.rdx_env_lookup(None, 0, 0, None, 0, None, 0, 4, 4, None, 0), _lib.last_error())\n"
            "print(L.rdx_trace_paths_env(None, None, 0, None, 0, 0, 4, None, 0, 0, None, 0, 0, None, 0, None, 0, 4, 4, None, None, 0, None), _lib.last_error())\n"
            "print(L.rdx_env_table_size(64, 32))\n") % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == 5, out.stdout
    for line, name in zip(lines, ("rdx_env_build", "rdx_env_light_hits", "rdx_env_lookup", "rdx_trace_paths_env")):
        rcode, msg = line.split(None, 1)
        assert int(rcode) < 0 and name in msg and "rdx_init" in msg, out.stdout
    assert int(lines[4]) == ec.layout(64, 32)["size"]


def test_the_wrappers_refuse_wrong_arguments_before_the_library(mods, monkeypatch):
    """no wrapper reaches the library with 16 records beside the environment, both or neither of keys and randoms, a stream above
    0xfffe, something that is no Environment, a size outside the limits or an argument of the wrong kind"""
    _lib, rd, env = mods
    reached = []
    real = _lib.lib

    class Spy:
        def __getattr__(self, name):
            if name.startswith("rdx_env_") and name != "rdx_env_table_size" or name == "rdx_trace_paths_env":
                reached.append(name)
            return getattr(real(), name)
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    buf = rd.Buffer(1234, 1 << 20)
    sb = rd.ShadingBuffers(buf, buf, buf, None, buf, buf)
    e = env.Environment(buf, buf, 64, 32)
    assert (e.width, e.height, e.image_offset, e.table_offset) == (64, 32, 0, 0)
    for kw in (dict(image=None), dict(table=7), dict(width=0), dict(height=0), dict(width=16385), dict(height=8193), dict(width=2.5), dict(width=True), dict(height="4")):
        a = dict(image=buf, table=buf, width=64, height=32)
        a.update(kw)
        with pytest.raises(rd.RadianceError, match="Environment"):
            env.Environment(**a)
    for kw in (dict(image=None), dict(width=0), dict(height=8193), dict(table=7), dict(width=-1)):
        a = dict(image=buf, width=64, height=32, table=buf)
        a.update(kw)
        with pytest.raises(rd.RadianceError, match="BuildEnvironment"):
            env.BuildEnvironment(a.pop("image"), a.pop("width"), a.pop("height"), **a)
    for array in (np.zeros((4, 4)), np.zeros((4, 4, 2)), np.zeros((0, 4, 3)), np.zeros((4, 4, 5)), np.zeros((1, 16385, 3), F)):
        with pytest.raises(rd.RadianceError, match="CreateEnvironment"):
            env.CreateEnvironment(None, array)
    bad = [dict(tlas=None), dict(rays=7), dict(keys=np.zeros(4)), dict(lights=None), dict(area=None), dict(area=np.zeros(2, rd.AREA_LIGHT_DTYPE)),
           dict(scene_buffers=(buf, buf)), dict(radiance=np.zeros(4)), dict(n=-1), dict(n=2.5), dict(max_depth=-1), dict(max_depth="4"), dict(light_count=-1),
           dict(area_count=-1), dict(light_count=14), dict(area_count=13), dict(light_count=16, area_count=0), dict(light_count=0, area_count=16), dict(area_count=2.5),
           dict(area_count=True), dict(light_count=None), dict(environment=None), dict(environment=buf), dict(environment=(buf, buf, 64, 32))]
    for kw in bad:
        a = dict(tlas=buf, rays=buf, keys=buf, n=4, max_depth=4, lights=buf, light_count=3, area=buf, area_count=2, environment=e, scene_buffers=sb, radiance=buf)
        a.update(kw)
        with pytest.raises(rd.RadianceError, match="TraceEnvPaths"):
            env.TraceEnvPaths(a.pop("tlas"), a.pop("rays"), a.pop("keys"), a.pop("n"), a.pop("max_depth"), a.pop("lights"), a.pop("light_count"), a.pop("area"),
                              a.pop("area_count"), a.pop("environment"), a.pop("scene_buffers"), **a)
    for kw in (dict(rays=None), dict(materials=7), dict(environment=buf), dict(environment=None), dict(lit=7), dict(shadow=7), dict(keys=None), dict(randoms=buf),
               dict(keys=7), dict(keys=None, randoms=np.zeros(4)), dict(stream=-1), dict(stream=0xffff), dict(stream=1.5), dict(stream=True), dict(stream=None)):
        a = dict(rays=buf, materials=buf, n=4, environment=e, keys=buf, randoms=None, stream=0, lit=buf, shadow=buf)
        a.update(kw)
        with pytest.raises(rd.RadianceError, match="EnvLightHits"):
            env.EnvLightHits(a.pop("rays"), a.pop("materials"), a.pop("n"), a.pop("environment"), **a)
    for kw in (dict(rays=None), dict(environment=buf), dict(radiance=7), dict(radiance=True)):
        a = dict(rays=buf, n=4, environment=e, radiance=buf)
        a.update(kw)
        with pytest.raises(rd.RadianceError, match="EnvLookup"):
            env.EnvLookup(a.pop("rays"), a.pop("n"), a.pop("environment"), **a)
    import torch
    r, k, m = torch.zeros((5, 8), dtype=torch.float32), torch.zeros((5, 4), dtype=torch.int32), torch.zeros((5, 16), dtype=torch.float32)
    for rays in (r, r.numpy(), None):       # CPU tensors, arrays, nothing: refused before any CUDA call
        with pytest.raises(rd.RadianceError, match="EnvLightHitsTorch"):
            env.EnvLightHitsTorch(rays, m, e, keys=k)
        with pytest.raises(rd.RadianceError, match="EnvLookupTorch"):
            env.EnvLookupTorch(rays, e)
        with pytest.raises(rd.RadianceError, match="TraceEnvPathsTorch"):
            env.TraceEnvPathsTorch(buf, rays, k, 4, None, None, e, sb)
    with pytest.raises(rd.RadianceError, match="TraceEnvPathsTorch"):
        env.TraceEnvPathsTorch(buf, r, k, 4, None, None, buf, sb)
    for image in (torch.zeros((4, 4, 4)), np.zeros((4, 4, 4), F), None):
        with pytest.raises(rd.RadianceError, match="BuildEnvironmentTorch"):
            env.BuildEnvironmentTorch(image)
    assert reached == [], reached
    with pytest.raises(rd.RadianceError, match="TableSize"):
        env.TableSize(-1, 4)


def test_the_procedural_sky_is_deterministic(mods):
    _lib, rd, env = mods
    a, b = env.ProceduralSky(64, 32, (0.3, 0.8, 0.52)), env.ProceduralSky(64, 32, (0.3, 0.8, 0.52))
    assert a.dtype == F and a.shape == (32, 64, 4) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isfinite(a).all() and (a >= 0).all() and not a[..., 3].any()
    sun = a[..., 0] > 1000.0
    assert 1 <= sun.sum() <= 4
    # the sun's texel is the one the library's convention gives its direction, and the ground is darker than the sky
    s = np.array([0.3, 0.8, 0.52]) / np.linalg.norm([0.3, 0.8, 0.52])
    y, x = ec.lookup_texel(table_of(a), 64, 32, s[None, :])
    assert sun[y[0], x[0]]
    assert a[:16, :, :3][~sun[:16]].min() > 2 * a[16:, :, :3].max() and a[16:, :, :3].max() < 0.1
    assert not np.array_equal(a, env.ProceduralSky(64, 32, (-0.3, 0.8, 0.52)))
    tiny = env.ProceduralSky(1, 1, (0, 1, 0))
    assert tiny.shape == (1, 1, 4) and tiny[0, 0, 0] > 1000.0
    with pytest.raises(rd.RadianceError):
        env.ProceduralSky(0, 4)


def test_the_stream_rule_keeps_the_random_numbers_apart():
    """the environment draws on stream A of a path of up to 62 bounces beside A <= 15 area records: no third word of pcg3d is the bare
    depth the scatter draws from, or another stream's"""
    depth = np.arange(63)
    words = np.stack([ar.stream_word(depth, s) for s in range(16)])
    assert np.unique(words).size == words.size and words.min() > 62
    assert int(ar.stream_word(62, 0xfffe)) == 62 + (0xffff << 16) < 2 ** 32


# ---- sampled_env by hand -------------------------------------------------------------------------------------------------------------
def test_u_of_exactly_one_chooses_the_last_lit_texel():
    img = np.zeros((4, 8, 4), F)
    img[..., :3] = 1.0
    img[3, 6:, :3] = 0.0            # the last two texels of the last row are dark
    p = table_of(img)
    s = ec.sampled_env(img, p, F(1.0), F(1.0), F(0.999))
    assert not s["dark"][0] and (int(s["y"][0]), int(s["x"][0])) == (3, 5) and s["X"][0] == p["header"]["total"] - 1
    assert 0 < s["fy"][0] < 1 and s["q"][0] >= 1
    lo = ec.sampled_env(img, p, F(0.0), F(0.0), F(0.0))
    assert (int(lo["y"][0]), int(lo["x"][0])) == (0, 0) and lo["fy"][0] > 0
    # pcg3d does give exactly 1.0: (float)0xffffffff / (float)0xffffffff
    assert F(0xffffffff) / F(0xffffffff) == F(1.0)
    # a caller's randoms outside [0, 1], or NaN, are held to the ends
    for u in (F(-3.0), F(np.nan), F(7.0), F(np.inf)):
        t = ec.sampled_env(img, p, u, u, F(0.5))
        assert 0 <= t["y"][0] < 4 and 0 <= t["x"][0] < 8


def test_a_single_hot_texel_takes_every_sample():
    img = np.zeros((19, 37, 4), F)
    img[5, 11] = (3.0, 9.0, 1.0, 0.7)
    p = table_of(img)
    assert p["header"]["total"] == 65535 and p["C"][5, 11] == 65535 and p["C"][5, 10] == 0 and p["M"][4] == 0 and p["M"][5] == 65535
    u, v, z = randoms(4096)
    s = ec.sampled_env(img, p, u, v, z)
    assert not s["dark"].any() and (s["y"] == 5).all() and (s["x"] == 11).all() and (s["q"] == 65535).all()
    rc = p["rowCos"]
    omega = np.float64(p["header"]["twoPiOverW"]) * (np.float64(rc[5]) - np.float64(rc[6]))
    assert np.allclose(s["E"], np.array([3.0, 9.0, 1.0]) * omega, rtol=1e-6)
    assert (s["ct"] <= rc[5]).all() and (s["ct"] >= rc[6]).all() and np.abs((s["L"] ** 2).sum(1) - 1).max() < 1e-6
    y, x = ec.lookup_texel(p, 37, 19, s["L"])
    inner = (s["fx"] > 0.01) & (s["fx"] < 0.99) & (s["fy"] > 0.01) & (s["fy"] < 0.99)
    assert (y[inner] == 5).all() and (x[inner] == 11).all() and inner.sum() > 3800


def test_a_zero_row_and_bad_texels_are_never_chosen():
    img = ec.hostile_sky(37, 19, 5)
    p = table_of(img)
    w = ec.weights(img, p["rowCos"])
    bad = ~np.isfinite(img[..., :3]).all(2) & np.isnan(img[..., :3]).any(2) | np.isinf(img[..., :3].max(2)) | (np.nan_to_num(img[..., :3], nan=-1.0).max(2) <= 0)
    assert bad.sum() >= 16 and (w[bad] == 0).all() and (w[9] == 0).all() and (w[~bad] > 0).all()
    q = np.diff(np.concatenate([np.zeros((19, 1), np.uint32), p["C"]], 1).astype(np.int64), axis=1)
    assert (q[bad] == 0).all() and (q[~bad] >= 1).all() and q.max() == 65535
    assert p["M"][9] == p["M"][8] and p["header"]["total"] == q.sum()
    u, v, z = randoms(65536)
    s = ec.sampled_env(img, p, u, v, z)
    assert not s["dark"].any() and not bad[s["y"], s["x"]].any() and (s["y"] != 9).all()
    assert np.isfinite(s["E"]).all() and np.array_equal(s["q"], q[s["y"], s["x"]].astype(np.uint32))
    # every texel with any light in it can be sampled: the dimmest still has q >= 1
    assert (q[(w > 0) & (w < p["header"]["wmax"] / 65535.0)] == 1).all()


def test_a_black_image_is_dark():
    for img in (np.zeros((4, 8, 4), F), np.full((4, 8, 4), -1.0, F), np.full((4, 8, 4), np.nan, F)):
        p = table_of(img)
        assert p["header"]["total"] == 0 and p["header"]["wmax"] == 0 and not p["C"].any() and not p["M"].any()
        s = ec.sampled_env(img, p, *randoms(64))
        assert s["dark"].all()


# ---- convergence ---------------------------------------------------------------------------------------------------------------------
def estimate(img, n=65536):
    p = table_of(img)
    u, v, z = randoms(n, frame=7, depth=0, stream=0)
    s = ec.sampled_env(img, p, u, v, z)
    f = np.maximum(s["L"][:, 1], 0.0)[:, None] * s["E"].astype(np.float64)         # receiver normal +y
    f[s["dark"]] = 0.0
    return f.mean(0), f.std(0, ddof=1) / np.sqrt(n), ec.quadrature(img, p), s, p


def test_the_estimator_converges_to_the_quadrature():
    """frame 7, pixels 0 .. 65535, depth 0, stream 0; receiver normal +y: the mean of max(N . L, 0) E per channel lies within 4
    standard errors of sum(radiance x solid angle x cosine), 8 sub-bands per row"""
    img = ec.sun_sky(64, 32)
    mean, se, want, s, p = estimate(img)
    print("sun sky: mean %s, s.e. %s, quadrature %s, %.2f s.e.; the sun takes %.1f %% of the samples"
          % (mean, se, want, np.abs(mean - want).max() / se.max(), 100.0 * (img[s["y"], s["x"], 0] > 1000).mean()))
    assert (np.abs(mean - want) <= 4 * se).all() and (se < 0.005 * want).all()
    assert (img[s["y"], s["x"], 0] > 1000).mean() > 0.8


def test_the_uniform_sky_gives_pi():
    img = np.ones((32, 64, 4), F)
    mean, se, want, s, p = estimate(img)
    print("uniform sky: mean %s, s.e. %s, quadrature %s" % (mean, se, want))
    assert np.abs(want - np.pi).max() < 1e-3
    assert (np.abs(mean - np.pi) <= 4 * se).all() and (se < 0.02).all()

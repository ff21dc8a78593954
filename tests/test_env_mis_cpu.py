"""CPU suite: multiple-importance sampling of the environment against the scatter sample (rdx_env_mis_weights,
rdx_trace_paths_env_mis; env.EnvMisWeights, env.TraceEnvMisPaths) -- the estimator of include/rdx.h as env_mis_cases restates it in
numpy, before test_gpu_env_mis.py holds the device to that restatement:

  1. env_pdf is a density: it sums to one over the texels;
  2. scatter_pdf is the density of the stock sampler's two reflective lobes (the float64 sampler of env_mis_cases.sample64);
  3. the weight rule, case by case, and the lobe boundaries of sample_brdf_transm;
  4. the estimator is unbiased at one point and has less variance than next-event estimation on a glossy surface under a broad sky;
  5. the ABI: symbols, prototypes, the record, the wrappers' refusals.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import area_cases as ar
import env_cases as ec
import env_mis_cases as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
N_SAMPLES = 1 << 18


@pytest.fixture(scope="module")
def mods(built):
    """the package; the lobe numbers and the record of the restatement are the library's"""
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import _lib, env, rd
    assert (env.LOBE_DIFFUSE, env.LOBE_SPECULAR, env.LOBE_TRANSMISSION, env.LOBE_NONE) == (em.LOBE_DIFFUSE, em.LOBE_SPECULAR, em.LOBE_TRANSMISSION, em.LOBE_NONE)
    assert env.MIS_WEIGHT_DTYPE == em.MIS_WEIGHT_DTYPE
    return _lib, rd, env


def table_of(image):
    H, W = image.shape[:2]
    return ec.parts(ec.build_table(image, ec.row_cos(H)), W, H)


def triples(n, frame, stream=0):
    return ar.pcg3d(np.full(n, frame, np.uint32), np.arange(n, dtype=np.uint32), ar.stream_word(np.full(n, 0), stream)).astype(F)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def view_at(N, degrees):
    """a unit vector `degrees` from N, towards the frame's tangent"""
    t, _, n = em.frame64(N)
    a = np.radians(degrees)
    return np.cos(a) * n + np.sin(a) * t


# ---- 1. env_pdf ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("sun", "hostile", "one texel", "black"))
def test_env_pdf_sums_to_one(mods, kind):
    image = {"sun": lambda: ec.sun_sky(64, 32), "hostile": lambda: ec.hostile_sky(37, 19, 5), "one texel": lambda: np.full((1, 1, 4), 2.5, F),
             "black": lambda: np.zeros((8, 16, 4), F)}[kind]()
    H, W = image.shape[:2]
    p = table_of(image)
    centres = ec.texel_centres(p, W, H).astype(F)
    pe = em.env_pdf(p, W, H, centres).astype(np.float64).reshape(H, W)
    rc = p["rowCos"].astype(np.float64)
    omega = float(p["header"]["twoPiOverW"]) * (rc[:-1] - rc[1:])
    total = float((pe * omega[:, None]).sum())
    print("%s: sum of pdf x solid angle = %.9f" % (kind, total))
    if kind == "black":
        assert p["header"]["total"] == 0 and not pe.any()
        return
    if kind == "hostile":
        assert (pe[H // 2] == 0).all() and (pe > 0).any(1).sum() >= H - 2        # the row of zeros can not be drawn
    # every term q / total is rounded three times in float32: the sum of the positive terms is 1 within 4 x 2^-24 of itself
    assert abs(total - 1.0) <= 4 * 2.0 ** -24 + 1e-12
    # it is the density sampled_env draws with: the texel a drawn direction falls in has q / total of its row and column
    u, v, z = triples(4096, 3).T
    s = ec.sampled_env(image, p, u, v, np.clip(z, 0.05, 0.95))
    fy_ok = (s["fy"] > 0.05) & (s["fy"] < 0.95) & ~s["dark"]
    got = em.env_pdf(p, W, H, s["L"][fy_ok].astype(F))
    q = s["q"][fy_ok].astype(F)
    want = ((q / F(p["header"]["total"])).astype(F) / (F(p["header"]["twoPiOverW"]) * (p["rowCos"][s["y"][fy_ok]] - p["rowCos"][s["y"][fy_ok] + 1]).astype(F)).astype(F)).astype(F)
    assert fy_ok.sum() >= (1 if kind == "one texel" else 1024) and np.array_equal(got, want)
    # nothing is shown along a zero or non-finite direction, or by a table of another size
    assert not em.env_pdf(p, W, H, np.array([[0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 0]], F)).any()
    assert not em.env_pdf(p, W + 1, H, centres[:4]).any()


# ---- 2. scatter_pdf ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angle", (10.0, 70.0))
@pytest.mark.parametrize("transmission", (0.0, 0.5))
@pytest.mark.parametrize("metallic", (0.0, 1.0))
@pytest.mark.parametrize("r", (0.2, 0.5, 1.0))
def test_scatter_pdf_is_the_samplers_density(mods, r, metallic, transmission, angle):
    """the mean of [a reflective lobe and NoL > 0] / p_s(L) over the sampler's own directions is the area of the hemisphere, and of
    NoL / p_s(L) its projected area, within 4 standard errors of the sample"""
    N = unit((0.3, 0.8, 0.52))
    V = view_at(N, angle)
    rnd = triples(N_SAMPLES, 11 + int(angle))
    L, _, lobe = em.sample64(N, V, (0.8, 0.6, 0.4), metallic, r, transmission, rnd)
    n = rnd.shape[0]
    rows = lambda a: np.broadcast_to(np.asarray(a, F), (n,) + np.shape(a))
    NoL, ps = em.scatter_pdf(rows(N), rows(V), L.astype(F), rows(F(r)), rows(F(transmission)))
    counted = (lobe != em.LOBE_TRANSMISSION) & (NoL > 0)
    assert abs((lobe == em.LOBE_TRANSMISSION).mean() - 0.5 * transmission) < 0.01 and (ps[counted] > 0).all()
    with np.errstate(all="ignore"):
        inv = np.where(counted, 1.0 / ps.astype(np.float64), 0.0)
    for what, g, want in (("1", np.ones(n), 2.0 * np.pi), ("NoL", NoL.astype(np.float64), np.pi)):
        x = inv * g
        mean, se = x.mean(), x.std(ddof=1) / np.sqrt(n)
        print("r %.1f metallic %.0f transmission %.1f V at %.0f deg: mean of %s / p_s = %.5f, want %.5f, %.2f standard errors" % (r, metallic, transmission, angle, what,
                                                                                                                            mean, want, (mean - want) / se))
        assert abs(mean - want) <= 4.0 * se, what


# ---- 3. the rule ----------------------------------------------------------------------------------------------------------------------------
def test_the_weight_rule(mods):
    one = F(1.0)
    w = lambda lobe, r, NoL, ps, pe: em.mis_weight(np.array([lobe]), np.array([r], F), np.array([NoL], F), np.array([ps], F), np.array([pe], F))[0]
    assert w(em.LOBE_TRANSMISSION, 0.5, 0.5, 1.0, 1.0) == one
    assert w(em.LOBE_SPECULAR, 0.0, 0.5, 1.0, 1.0) == one and w(em.LOBE_SPECULAR, 1e-12, 0.5, 1.0, 1.0) == one       # (r r)(r r) underflows to 0
    assert w(em.LOBE_DIFFUSE, 0.0, 0.5, 1.0, 3.0) == F(0.25) and w(em.LOBE_NONE, 0.0, 0.5, 1.0, 3.0) == F(0.25)       # a mirror's diffuse lobe is no delta
    assert w(em.LOBE_SPECULAR, 0.5, 0.0, 1.0, 1.0) == one and w(em.LOBE_NONE, 0.5, -0.2, 1.0, 1.0) == one and w(em.LOBE_NONE, 0.5, np.nan, 1.0, 1.0) == one
    for bad in (np.nan, np.inf, -np.inf):
        assert w(em.LOBE_SPECULAR, 0.5, 0.5, bad, 1.0) == one and w(em.LOBE_NONE, 0.5, 0.5, 1.0, bad) == one
    assert w(em.LOBE_NONE, 0.5, 0.5, 0.0, 0.0) == one and w(em.LOBE_DIFFUSE, 0.5, 0.5, 0.0, 2.0) == F(0.0) and w(em.LOBE_DIFFUSE, 0.5, 0.5, 2.0, 0.0) == one
    assert w(em.LOBE_SPECULAR, 0.5, 0.5, 1.0, 3.0) == F(0.25)
    # the environment's weight is 1 - w_scatter by definition: the two sum to one, and it is the balance heuristic's other half
    rng = np.random.default_rng(3)
    ps, pe = (rng.uniform(0.0, 50.0, 4096).astype(F) ** 2 for _ in range(2))
    ws = em.mis_weight(np.full(4096, em.LOBE_NONE), np.full(4096, 0.5, F), np.full(4096, 0.5, F), ps, pe)
    sky = (F(1.0) - ws).astype(F)
    assert ((ws >= 0) & (ws <= 1)).all() and np.abs(sky.astype(np.float64) - pe.astype(np.float64) / (ps.astype(np.float64) + pe)).max() <= 2.0 ** -22
    # the lobes, at their borders: rnd.z == 0.5 is no longer the lower half, 2 rnd.z == transmission is no longer transmission
    below = lambda x: np.nextafter(F(x), F(-1))
    z = np.array([0.0, below(0.15), 0.15, below(0.5), 0.5, 1.0], F)
    rnd = np.stack([np.zeros(6, F), np.zeros(6, F), z], 1)
    T, D, S = em.LOBE_TRANSMISSION, em.LOBE_DIFFUSE, em.LOBE_SPECULAR
    assert em.lobe_of(rnd, np.full(6, 0.3, F)).tolist() == [T, T, D, D, S, S]
    assert em.lobe_of(rnd, np.zeros(6, F)).tolist() == [D, D, D, D, S, S]
    assert em.lobe_of(rnd, np.full(6, 1.0, F)).tolist() == [T, T, T, T, S, S] and em.lobe_of(rnd, np.full(6, 7.0, F)).tolist() == [T, T, T, T, S, S]
    assert em.lobe_of(rnd, np.full(6, np.nan, F)).tolist() == [D, D, D, D, S, S]
    text = open(os.path.join(ROOT, "radiance-ray-tracing_amd", "csrc", "stages.h")).read()
    assert "const bool lower = rnd.z < 0.5f;" in text and "if (lower && (2.0f * rnd.z) < transmission) {" in text
    mine = open(os.path.join(ROOT, "radiance-ray-tracing_amd", "csrc", "env_mis.h")).read()
    assert "const bool lower = rnd.z < 0.5f;" in mine and "if (lower && (2.0f * rnd.z) < transmission) return LOBE_TRANSMISSION;" in mine
    # scatter_pdf at a point worked by hand: N = V = L = +y, r = 1 (D = 1 / pi), transmission 0.25
    y = np.array([[0.0, 1.0, 0.0]], F)
    NoL, ps = em.scatter_pdf(y, y, y, np.array([1.0], F), np.array([0.25], F))
    assert NoL[0] == one and abs(float(ps[0]) - (0.5 / (4 * np.pi) + 0.375 / np.pi)) < 1e-6
    assert em.scatter_pdf(y, y, -y, np.array([1.0], F), np.array([0.0], F))[1][0] == 0


# ---- 4. unbiased, and less noise ------------------------------------------------------------------------------------------------------
def estimators(image, N, V, albedo, metallic, r):
    """per key: next-event estimation alone, and the MIS estimator -- the weighted sky sample plus the weighted sky texel along the
    scattered direction times nextFactor -- at one opaque point without an occluder, in float64"""
    H, W = image.shape[:2]
    p = table_of(image)
    n = N_SAMPLES
    rows = lambda a: np.broadcast_to(np.asarray(a, F), (n,) + np.shape(a))
    weight = lambda L, lobe: em.mis_weight(lobe, rows(F(r)), *em.scatter_pdf(rows(N), rows(V), L.astype(F), rows(F(r)), rows(F(0.0))), em.env_pdf(p, W, H, L.astype(F)))
    u, v, z = triples(n, 21, stream=0).T
    s = ec.sampled_env(image, p, u, v, z)
    nee = np.where(s["dark"][:, None], 0.0, em.brdf64(N, V, s["L"], albedo, metallic, r) * s["E"].astype(np.float64))
    w_sky = 1.0 - weight(s["L"], np.full(n, em.LOBE_NONE)).astype(np.float64)
    L, nf, lobe = em.sample64(N, V, albedo, metallic, r, 0.0, triples(n, 22))
    ty, tx = ec.lookup_texel(p, W, H, L)
    texel = image[ty, tx, :3].astype(np.float64)
    w_s = weight(L, lobe).astype(np.float64)
    return nee, nee * w_sky[:, None] + nf * texel * w_s[:, None]


@pytest.mark.parametrize("metallic", (0.0, 1.0))
def test_the_estimator_is_unbiased_at_a_point(mods, metallic):
    N = np.array([0.0, 1.0, 0.0])
    nee, mis = estimators(ec.sun_sky(64, 32), N, view_at(N, 40.0), (0.8, 0.6, 0.4), metallic, 0.3)
    d = mis - nee
    se = d.std(0, ddof=1) / np.sqrt(d.shape[0])
    print("metallic %.0f: next-event mean %s, MIS mean %s, difference in standard errors %s" % (metallic, nee.mean(0), mis.mean(0), d.mean(0) / se))
    assert (nee.mean(0) > 0).all() and (np.abs(d.mean(0)) <= 4.0 * se).all()


def test_less_noise_on_a_glossy_surface_under_a_broad_sky(mods):
    N = np.array([0.0, 1.0, 0.0])
    image = np.ones((32, 64, 4), F)
    nee, mis = estimators(image, N, view_at(N, 40.0), (0.8, 0.6, 0.4), 1.0, 0.1)
    d = mis - nee
    assert (np.abs(d.mean(0)) <= 4.0 * d.std(0, ddof=1) / np.sqrt(d.shape[0])).all()
    print("variance summed over rgb: next-event %.4g, MIS %.4g" % (nee.var(0).sum(), mis.var(0).sum()))
    assert mis.var(0).sum() < nee.var(0).sum()


# ---- 5. the ABI ---------------------------------------------------------------------------------------------------------------------------
def prototype(hdr, name):
    """the ctypes argument list of a prototype of include/rdx.h, from its text"""
    m = re.search(r"\b%s\((.*?)\);" % name, hdr, re.S)
    assert m, name
    text = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    kinds = []
    from radiance_ray_tracing_amd import _lib
    for arg in text.split(","):
        arg = " ".join(arg.split())
        kind = {"rdx_buffer": C.c_void_p, "size_t": C.c_size_t, "uint32_t": C.c_uint32, "const rdx_shading_buffers*": C.POINTER(_lib.rdx_shading_buffers),
                "uint32_t*": C.POINTER(C.c_uint32)}[arg.rsplit(" ", 1)[0]]
        kinds.append(kind)
    return kinds


def test_the_library_exports_the_calls(mods):
    _lib, rd, env = mods
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "rdx.h")).read()
    P, Z, U = C.c_void_p, C.c_size_t, C.c_uint32
    want = {"rdx_env_mis_weights": [P, Z, P, Z, P, Z, U, P, Z, U, P, Z, P, Z, P, Z, P, Z, U, U, P, Z],
            "rdx_trace_paths_env_mis": _lib.SIGNATURES["rdx_trace_paths_env"][1]}
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == (C.c_int, args) and getattr(L, name).argtypes == args and getattr(L, name).restype is C.c_int, name
        assert prototype(hdr, name) == args, name
    assert prototype(hdr, "rdx_trace_paths_env") == want["rdx_trace_paths_env_mis"]
    assert hdr.index("rdx_trace_paths_env_mis(rdx_buffer") > hdr.index("rdx_trace_paths_env(rdx_buffer")
    fields = [(n, em.MIS_WEIGHT_DTYPE.fields[n][1]) for n in em.MIS_WEIGHT_DTYPE.names]
    assert fields == [("w_scatter", 0), ("pdf_scatter", 4), ("pdf_env", 8), ("lobe", 12)] and em.MIS_WEIGHT_DTYPE.itemsize == 16
    record = re.search(r"typedef struct rdx_env_mis_weight \{(.*?)\}", hdr, re.S).group(1)
    assert " ".join(record.split()) == "float w_scatter, pdf_scatter, pdf_env; uint32_t lobe;"
    for k, lobe in enumerate(("DIFFUSE", "SPECULAR", "TRANSMISSION", "NONE")):
        assert "#define RDX_LOBE_%s %du" % (lobe, k) in hdr and getattr(env, "LOBE_" + lobe) == k
    for text in ("pSpec = D * NoH / (4.0f * VoH)", "pdf_scatter = 0.5f * pSpec + (0.5f * (1.0f - t)) * pDiff",
                 "pdf_env = ((float)q / (float)total) / (twoPiOverW * (rowCos[y] - rowCos[y + 1]))", "color += weight * (rdx_env_lookup(ray).rgb * w)",
                 "lit.rgb * (1.0f - w_scatter("):
        assert text in hdr, text
    from radiance_ray_tracing_amd import build
    assert "env_mis.hip" in build.SOURCES and "env_mis.h" in build.HEADERS
    for name in ("EnvMisWeights", "EnvMisWeightsTorch", "TraceEnvMisPaths", "TraceEnvMisPathsTorch"):
        assert callable(getattr(env, name)), name
    assert not hasattr(rd, "TraceEnvMisPaths") and not hasattr(rd, "EnvMisWeights")
    cxx = open(os.path.join(ROOT, "include", "radiance.h")).read()
    for name, sym in (("EnvMisWeights", "rdx_env_mis_weights"), ("TraceEnvMisPaths", "rdx_trace_paths_env_mis")):
        assert re.search(r"\b%s\(" % name, cxx) and sym + "(" in cxx, name
    # one text: the path kernel and the per-hit kernel call the same weight function, the header's
    unit = open(os.path.join(ROOT, "radiance-ray-tracing_amd", "csrc", "env_mis.hip")).read()
    head = open(os.path.join(ROOT, "radiance-ray-tracing_amd", "csrc", "env_mis.h")).read()
    assert unit.count("env_mis_weight(") == 3 and "MisWeight env_mis_weight(" in head and "float env_pdf(" in head and "float scatter_pdf(" in head
    assert "env_pdf(" not in unit and "scatter_pdf(" not in unit


def test_an_uninitialised_library_refuses_and_names_the_call(mods):
    """(a fresh process: the suite's other tests may have initialised the library in this one)"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import rrt_amd\n"
            "from radiance_ray_tracing_amd import _lib\n"
            "L = _lib.lib()\n"
            "print(L.rdx_env_mis_weights(None, 0, None, 0, None, 0, 0, None, 0, 0, None, 0, None, 0, None, 0, None, 0, 4, 4, None, 0), _lib.last_error())\n"
            "print(L.rdx_trace_paths_env_mis(None, None, 0, None, 0, 0, 4, None, 0, 0, None, 0, 0, None, 0, None, 0, 4, 4, None, None, 0, None), _lib.last_error())\n"
            ) % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == 2, out.stdout
    for line, name in zip(lines, ("rdx_env_mis_weights", "rdx_trace_paths_env_mis")):
        rcode, msg = line.split(None, 1)
        assert int(rcode) < 0 and name in msg and "rdx_init" in msg, out.stdout


def test_the_wrappers_refuse_wrong_arguments_before_the_library(mods, monkeypatch):
    _lib, rd, env = mods
    reached = []
    real = _lib.lib

    class Spy:
        def __getattr__(self, name):
            if name in ("rdx_env_mis_weights", "rdx_trace_paths_env_mis"):
                reached.append(name)
            return getattr(real(), name)
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    buf = rd.Buffer(1234, 1 << 20)
    sb = rd.ShadingBuffers(buf, buf, buf, None, buf, buf)
    e = env.Environment(buf, buf, 64, 32)
    good = dict(rays=buf, materials=buf, dirs=buf, n=4, environment=e)
    for kw, word in ((dict(rays=None), "Buffers"), (dict(dirs=7), "Buffers"), (dict(environment=buf), "Environment"), (dict(keys=buf, randoms=buf), "both"),
                     (dict(keys=3), "keys"), (dict(src=3), "src"), (dict(n=-1), "n must"), (dict(n=2.5), "n must"), (dict(nrecords=5), "nrecords"),
                     (dict(src=buf, nrecords=True), "nrecords"), (dict(out=True), "out")):
        a = dict(good, **kw)
        with pytest.raises(rd.RadianceError, match="EnvMisWeights") as err:
            env.EnvMisWeights(a.pop("rays"), a.pop("materials"), a.pop("dirs"), a.pop("n"), a.pop("environment"), **a)
        assert word in str(err.value), (kw, str(err.value))
    path = dict(tlas=buf, rays=buf, keys=buf, n=4, max_depth=2, lights=None, light_count=0, area=None, area_count=0, environment=e, scene_buffers=sb)
    for kw, word in ((dict(light_count=15, lights=buf, area_count=1, area=buf), "MAX_PATH_LIGHTS"), (dict(environment=None), "Environment"), (dict(lights=None, light_count=2), "lights"),
                     (dict(tlas=None), "Buffer"), (dict(max_depth=-1), "max_depth")):
        a = dict(path, **kw)
        with pytest.raises(rd.RadianceError, match="TraceEnvMisPaths") as err:
            env.TraceEnvMisPaths(*[a[k] for k in path])
        assert word in str(err.value), (kw, str(err.value))
    assert reached == []

"""CPU suite: the ABI of rdx_denoise (the settings record, the symbols, the header's text, the work size and its limits), the
argument checks of the wrappers of radiance_ray_tracing_amd.denoise, and the properties of denoise_cases.denoise_reference -- the
numpy restatement of the filter, one IEEE float32 operation at a time -- before test_gpu_denoise.py holds the kernels to its bits."""
import ctypes as C
import fractions
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import denoise_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
S = dc.Settings


@pytest.fixture(scope="module")
def mods(built):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import _lib, denoise, rd
    return _lib, rd, denoise


# ---- the record, the symbols, the header -------------------------------------------------------------------------------------------------
def test_the_settings_record(mods):
    _lib, rd, dn = mods
    T = _lib.rdx_denoise_settings
    assert C.sizeof(T) == 32 == dc.SETTINGS_DTYPE.itemsize
    for name in ("passes", "normal_squarings", "sigma_position", "sigma_colour", "flags", "_0"):
        assert getattr(T, name).offset == dc.SETTINGS_DTYPE.fields[name][1], name
    assert (T.passes.offset, T.sigma_position.offset, T.flags.offset, T._0.offset, T._0.size) == (0, 8, 16, 20, 12)
    s = dn.DenoiseSettings()
    assert (s.passes, s.normal_squarings, s.sigma_position, s.sigma_colour, s.demodulate, s.debug, s.flags) == (5, 5, 0.0, 0.0, True, False, 1)
    raw = np.frombuffer(bytes(dn.DenoiseSettings(3, 2, 0.1, 0.25, False, True)._struct()), dc.SETTINGS_DTYPE)[0]
    assert (raw["passes"], raw["normal_squarings"], raw["sigma_position"], raw["sigma_colour"], raw["flags"]) == (3, 2, F(0.1), F(0.25), 2) and not raw["_0"].any()
    assert (dn.DEMODULATE, dn.DEBUG, dn.MAX_PASSES, dn.MAX_SQUARINGS, dn.MAX_DIM, dn.MAX_PIXELS) == (1, 2, 8, 7, 16384, 1 << 26)


def test_the_library_exports_the_call(mods):
    _lib, rd, dn = mods
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "rdx.h")).read()
    P, Z, U = C.c_void_p, C.c_size_t, C.c_uint32
    want = {"rdx_denoise_work_size": (Z, [U, U]),
            "rdx_denoise": (C.c_int, [P, Z, P, Z, P, Z, U, U, C.POINTER(_lib.rdx_denoise_settings), P, Z, P, Z, P, Z])}
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig and getattr(L, name).argtypes == sig[1] and getattr(L, name).restype is sig[0], name
        assert re.search(r"\b%s\(" % name, hdr), name
    for text in ("typedef struct rdx_denoise_settings {      /* 32 B */", "#define RDX_DENOISE_DEMODULATE 1u", "#define RDX_DENOISE_DEBUG      2u",
                 "den_k = DEMODULATE ? fmaxf(a_k, 0.015625f) : 1", "w  = ((k * wn) * wz) * wc", "l(c) = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b",
                 "wz = sigma_position == 0 ? 1 : fmaxf(1 - fabsf(dot(n(p), P(q) - P(p))) / (sigma_position * (float)s), 0)",
                 "wc = sigma_colour == 0 ? 1 : 1 / (1 + x * x)", "width == 0 or height == 0 succeeds and touches nothing"):
        assert text in hdr, text
    from radiance_ray_tracing_amd import build
    assert "denoise.hip" in build.SOURCES and "denoise.h" in build.HEADERS
    for name in ("DenoiseSettings", "WorkSize", "Denoise", "DenoiseTorch"):
        assert callable(getattr(dn, name)), name
    assert not any("enoise" in name for name in dir(rd)), "rd.py gets no new public name"
    cxx = open(os.path.join(ROOT, "include", "radiance.h")).read()
    assert re.search(r"\bDenoise\(", cxx) and "rdx_denoise(" in cxx and "rdx_denoise_work_size(" in cxx
    unit = open(os.path.join(ROOT, "radiance-ray-tracing_amd", "csrc", "denoise.hip")).read()
    for kernel in ("k_denoise_prepare", "k_denoise_pass"):
        assert "\n%s(" % kernel in unit, kernel
    assert "store_rgba8(" in unit and '#include "raygen_device.h"' in unit


def test_work_size_and_its_limits(mods):
    _lib, rd, dn = mods
    L = _lib.lib()
    for W, H in ((1, 1), (5, 3), (64, 4), (1920, 1080), (16384, 1), (1, 16384), (16384, 4096), (8192, 8192)):
        size = dn.WorkSize(W, H)
        assert size == L.rdx_denoise_work_size(W, H) == dn.WORK_BYTES_PER_PIXEL * W * H and 0 < size <= 64 * W * H and size % 16 == 0, (W, H)
    for W, H in ((0, 1), (1, 0), (0, 0), (16385, 1), (1, 16385), (16384, 4097), (8193, 8192), (0xffffffff, 0xffffffff), (0x10000, 0x10000)):
        assert dn.WorkSize(W, H) == 0 == L.rdx_denoise_work_size(W, H), (W, H)
    for bad in ((-1, 4), (4, 2.5), (True, 4), ("4", 4), (1 << 32, 1)):
        with pytest.raises(rd.RadianceError, match="WorkSize"):
            dn.WorkSize(*bad)


def test_an_uninitialised_library_refuses_and_names_the_call(mods):
    """(a fresh process: the suite's other tests may have initialised the library in this one)"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import rrt_amd\n"
            "from radiance_ray_tracing_amd import _lib\n"
            "L = _lib.lib()\n"
            "print(L.rdx_denoise(None, 0, None, 0, None, 0, 4, 4, None, None, 0, None, 0, None, 0), _lib.last_error())\n"
            "print(L.rdx_denoise_work_size(64, 32))\n") % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == 2, out.stdout
    rcode, msg = lines[0].split(None, 1)
    assert int(rcode) < 0 and "rdx_denoise" in msg and "rdx_init" in msg, out.stdout
    assert int(lines[1]) == 48 * 64 * 32


def test_the_wrappers_refuse_wrong_arguments_before_the_library(mods, monkeypatch):
    """one refusal of each kind the wrappers can decide: handles that are no Buffers, settings that are none or outside their ranges,
    a size outside the limits, offsets off their alignment, short ranges, outputs that overlap, tensors of the wrong kind"""
    _lib, rd, dn = mods
    reached = []
    real = _lib.lib

    class Spy:
        def __getattr__(self, name):
            if name == "rdx_denoise":
                reached.append(name)
            return getattr(real(), name)
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    for kw in (dict(passes=9), dict(passes=-1), dict(passes=2.0), dict(passes=True), dict(normal_squarings=8), dict(normal_squarings=None), dict(sigma_position=-1.0),
               dict(sigma_position=float("inf")), dict(sigma_position=float("nan")), dict(sigma_colour=-0.5), dict(sigma_colour="1"), dict(sigma_colour=1e39),
               dict(sigma_position=1e-60), dict(sigma_colour=True), dict(demodulate=1), dict(debug=None)):
        with pytest.raises(rd.RadianceError, match="DenoiseSettings"):
            dn.DenoiseSettings(**kw)
    W, H = 8, 4
    n = W * H
    col, rec, out, img, work = rd.Buffer(11, 16 * n), rd.Buffer(12, 64 * n), rd.Buffer(13, 16 * n + 32), rd.Buffer(14, 4 * n + 8), rd.Buffer(15, dn.WORK_BYTES_PER_PIXEL * n + 16)
    rec2 = rd.Buffer(16, 64 * n)
    ok = dn.DenoiseSettings()
    bad = [dict(color=None), dict(materials=7), dict(surfaces=np.zeros(4)), dict(out=7), dict(image=7), dict(work=7),                    # handles
           dict(settings=None), dict(settings=dict(passes=5)), dict(settings=dc.Settings()),                                           # settings
           dict(width=16385, height=1), dict(width=1, height=16385), dict(width=16384, height=4097), dict(width=-1), dict(height=2.5), dict(width=True),    # sizes
           dict(color_offset=8), dict(materials_offset=4), dict(surfaces_offset=-16), dict(out_offset=24), dict(work_offset=1), dict(image_offset=2),        # offsets
           dict(width=9), dict(out_offset=48), dict(work_offset=32), dict(image_offset=12), dict(color_offset=16), dict(surfaces_offset=64),                  # short ranges
           dict(out=col), dict(work=rec), dict(image=rec2, surfaces=rec2), dict(work=out)]                                             # overlaps
    for kw in bad:
        a = dict(color=col, materials=rec, surfaces=rec2, width=W, height=H, settings=ok, out=out, image=img, work=work)
        a.update(kw)
        with pytest.raises(rd.RadianceError, match="Denoise"):
            dn.Denoise(a.pop("color"), a.pop("materials"), a.pop("surfaces"), a.pop("width"), a.pop("height"), a.pop("settings"), **a)
    import torch
    c, m, s = torch.zeros((n, 4)), torch.zeros((n, 16)), torch.zeros((n, 16))
    for colors in (c, c.numpy(), None):        # CPU tensors, arrays, nothing: refused before any CUDA call
        with pytest.raises(rd.RadianceError, match="DenoiseTorch"):
            dn.DenoiseTorch(colors, m, s, W, H, ok)
    assert reached == [], reached


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def _round_f32(x):
    """the float32 nearest to the Fraction x (ties to even), for x in the normal range"""
    if x == 0:
        return F(0)
    sign, x = (-1, -x) if x < 0 else (1, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if fractions.Fraction(2) ** e > x:
        e -= 1
    m = round(x / fractions.Fraction(2) ** (e - 23))           # 2^23 <= m <= 2^24, half to even
    return F(sign * float(m) * 2.0 ** (e - 23))


def test_the_restated_fma_is_the_exactly_rounded_one():
    """on random operands, on sums that cancel, and on sums that land on a float32 tie after the float64 addition rounded -- the case
    in which rounding twice differs from rounding once"""
    rng = np.random.default_rng(11)
    a = rng.normal(size=3000).astype(F)
    b = rng.normal(size=3000).astype(F)
    c = rng.normal(size=3000).astype(F)
    c[1000:2000] = (-(a[1000:2000].astype(np.float64) * b[1000:2000])).astype(F)            # cancellation
    # a * b = 1 + 2^-24 (a float32 tie) + 2^-47.., c tiny: the float64 sum rounds onto the tie unless it is kept odd
    a[2000:] = F(1.0) + F(2.0 ** -23) * rng.integers(1, 1 << 10, 1000).astype(F)
    b[2000:] = F(1.0) + F(2.0 ** -23) * rng.integers(1, 1 << 10, 1000).astype(F)
    c[2000:] = (rng.choice([-1.0, 1.0], 1000) * 2.0 ** -24 * (1.0 + rng.integers(0, 4, 1000) * 2.0 ** -30)).astype(F)
    got = dc.fma(a, b, c)
    want = np.array([_round_f32(fractions.Fraction(float(x)) * fractions.Fraction(float(y)) + fractions.Fraction(float(z))) for x, y, z in zip(a, b, c)], F)
    assert np.array_equal(dc.bits(got + F(0)), dc.bits(want + F(0)))       # (+ 0: the sign of a zero sum is not at stake)
    with np.errstate(all="ignore"):
        assert np.isnan(dc.fma(F(np.inf), F(0), F(1))) and dc.fma(F(3e38), F(3e38), F(1)) == np.inf and dc.fma(F(2), F(3), F(-np.inf)) == -np.inf


def test_a_flat_wall_of_constant_colour_comes_back():
    """within relative 2^-18 per channel: the worst case of 25 weighted additions and a division, per pass far below it"""
    for W, H in ((40, 24), (7, 5)):
        color, mat, surf = dc.wall(W, H)
        for st in (S(), S(5, 5, 0.05, 0.25, True), S(8, 0, 0.0, 0.0, False)):
            out = dc.denoise_reference(color, mat, surf, W, H, st)
            rel = np.abs(out[:, :3].astype(np.float64) / color[:, :3].astype(np.float64) - 1.0).max()
            assert rel <= 2.0 ** -18, (W, H, st, rel)
            assert np.array_equal(dc.bits(out[:, 3]), dc.bits(color[:, 3]))


def test_perpendicular_halves_never_mix():
    W, H = 48, 20
    color, mat, surf, right = dc.two_halves(W, H)
    for st in (S(demodulate=False), S(5, 1, 0.0, 0.0, False), S(4, 5, 0.0, 0.3, False)):
        out = dc.denoise_reference(color, mat, surf, W, H, st)
        for half in (right, ~right):
            lo, hi = color[half, :3].min(0), color[half, :3].max(0)
            assert (out[half, :3] >= lo).all() and (out[half, :3] <= hi).all(), st
        assert not dc.same(out, color)


def test_invalid_pixels_and_bad_colours_stay_where_they_are():
    W, H = 24, 16
    rng = np.random.default_rng(5)
    color, mat, surf = dc.noisy_wall(W, H, 5)
    invalid = rng.permutation(W * H)[:40]
    mat["hit"][invalid[:15]] = 0
    surf["hit"][invalid[15:30]] = 0
    mat["hit"][invalid[30:]] = 2
    for st in (S(), S(3, 5, 0.05, 0.4, True), S(3, 0, 0.0, 0.0, False)):
        base = dc.denoise_reference(color, mat, surf, W, H, st)
        assert np.array_equal(dc.bits(base[invalid]), dc.bits(color[invalid])), "an invalid pixel comes back bit for bit"
        assert np.isfinite(base[:, :3]).all()
        p = int(invalid[7])
        for value in (1e30, np.nan):
            c2 = color.copy()
            c2[p, :3] = value
            out = dc.denoise_reference(c2, mat, surf, W, H, st)
            others = np.arange(W * H) != p
            assert np.array_equal(dc.bits(out[others]), dc.bits(base[others])) and np.array_equal(dc.bits(out[p]), dc.bits(c2[p])), (st, value)
        v = int(np.setdiff1d(np.arange(W * H), invalid)[101])
        c3 = color.copy()
        c3[v, 1] = np.nan
        out = dc.denoise_reference(c3, mat, surf, W, H, st)
        others = np.arange(W * H) != v
        assert np.isfinite(out[others, :3]).all(), "a NaN colour at a valid pixel poisons no neighbour"


def test_no_pass_is_the_identity_up_to_the_albedo():
    W, H = 37, 19
    color, mat, surf = dc.hostile(W, H, 2)
    valid = dc.validity(mat, surf)
    assert valid.any() and (~valid).any()
    for demodulate in (False, True):
        out = dc.denoise_reference(color, mat, surf, W, H, S(0, 5, 0.1, 0.1, demodulate))
        assert np.array_equal(dc.bits(out[~valid]), dc.bits(color[~valid])) and np.array_equal(dc.bits(out[:, 3]), dc.bits(color[:, 3]))
        den = dc.den_of(mat, demodulate)
        with np.errstate(all="ignore"):
            want = (color[:, :3] / den) * den
        assert dc.same(out[valid, :3], want[valid])
        if not demodulate:
            assert dc.same(out, color)
    assert (dc.den_of(mat, True) >= dc.MIN_ALBEDO).all(), "a NaN, zero or negative albedo gives 1 / 64"


def test_white_noise_loses_the_stencils_share_of_its_variance():
    """one pass on a 64 x 64 wall of white noise leaves sum(h_i^2 h_j^2) = (70 / 256)^2 = 4900 / 65536 = 0.0748 of the variance in the
    interior; 0.06 .. 0.09 is the sampling error of 60 x 60 pixels.  Each further pass up to 4 lowers it again"""
    W = H = 64
    color, mat, surf = dc.noisy_wall(W, H, 7)
    inner = np.zeros((H, W), bool)
    inner[2:-2, 2:-2] = True
    inner = inner.reshape(-1)
    var = lambda a: float(a[inner, :3].astype(np.float64).var(0).mean())
    v0 = var(color)
    ratios = [var(dc.denoise_reference(color, mat, surf, W, H, S(k, 5, 0.0, 0.0, False))) / v0 for k in range(1, 5)]
    print("variance ratios after 1 .. 4 passes:", ratios)
    assert 0.06 <= ratios[0] <= 0.09, ratios
    assert all(b < a for a, b in zip(ratios, ratios[1:])), ratios

"""CPU suite: the ABI of rdx_shade_hits (the stock closest-hit shader on ray-query hits), its bounds rule through the host seam
rdx_debug_shade_in_bounds, and the COMPARAND of its GPU tests: the numpy restatement of the raygen loop in tests/shade_cases.py
(compose_frames) is itself held to the CPU oracle's own progressive frames, bit for bit, before test_gpu_shade.py drives it with
the public GPU calls; and the recordings that test relies on (tests/golden/refgpu_c{0,1,2}.npz) are shown to hold both branches
of the shadow test often enough."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import golden_cases as gc
import oracle_bind as ob
import shade_cases as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def mods(built):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import _lib, rd, scenes
    return _lib, rd, scenes


def test_struct_sizes_and_offsets(mods):
    _lib, rd, _ = mods
    assert C.sizeof(_lib.rdx_shade) == 48 == rd.SHADE_DTYPE.itemsize and sh.SHADE_DTYPE == rd.SHADE_DTYPE
    assert C.sizeof(_lib.rdx_shade_key) == 16 == rd.SHADE_KEY_DTYPE.itemsize and sh.SHADE_KEY_DTYPE == rd.SHADE_KEY_DTYPE
    assert C.sizeof(_lib.rdx_shading_buffers) == 8 * C.sizeof(C.c_void_p)
    names = ["scene", "meshInfo", "index", "uv", "normal", "material", "textureArray", "sampler"]
    assert [n for n, _ in _lib.rdx_shading_buffers._fields_] == names
    want = [("color", 0), ("hit", 12), ("colorOccluded", 16), ("materialIndex", 28), ("nextFactor", 32), ("slot", 44)]
    assert [(n, getattr(_lib.rdx_shade, n).offset) for n, _ in want] == want
    assert [(n, rd.SHADE_DTYPE.fields[n][1]) for n, _ in want] == want
    kwant = [("frameID", 0), ("pixel", 4), ("depth", 8), ("_0", 12)]
    assert [(n, getattr(_lib.rdx_shade_key, n).offset) for n, _ in kwant] == kwant
    assert [(n, rd.SHADE_KEY_DTYPE.fields[n][1]) for n, _ in kwant] == kwant
    hdr = open(os.path.join(ROOT, "include", "rdx.h")).read()
    body = re.search(r"typedef struct rdx_shade\s*\{(.*?)\}\s*rdx_shade;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [m.group(1) for m in re.finditer(r"(\w+)(?:\[\d+\])?\s*;", body)] == [n for n, _ in want]
    assert re.search(r"typedef struct rdx_shade_key\s*\{\s*uint32_t frameID, pixel, depth, _0;\s*\}", hdr)
    assert re.search(r"typedef struct rdx_shading_buffers\s*\{\s*rdx_buffer scene, meshInfo, index, uv, normal, material, textureArray;\s*rdx_sampler sampler;\s*\}", hdr)
    assert rd.NO_SLOT == sh.NO_SLOT == 0xffffffff


def test_every_symbol_is_present(mods):
    _lib, rd, scenes = mods
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "rdx.h")).read()
    for name in ("rdx_shade_hits", "rdx_debug_shade_in_bounds"):
        assert name in _lib.SIGNATURES and getattr(L, name)
        assert re.search(r"\b%s\(" % name, hdr)
    P, Z, U = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)
    assert _lib.SIGNATURES["rdx_shade_hits"] == (C.c_int, [P, P, Z, P, Z, P, Z, C.c_uint32, C.POINTER(_lib.rdx_shading_buffers), P, Z, P, Z, P, Z, P, Z, U, U])
    for name in ("ShadeHits", "ShadeHitsTorch", "ShadingBuffers", "SHADE_DTYPE", "SHADE_KEY_DTYPE", "DebugShadeInBounds"):
        assert hasattr(rd, name), name
    assert hasattr(scenes.DeviceScene, "shading_buffers")
    assert "ShadeHits" in open(os.path.join(ROOT, "include", "radiance.h")).read()
    build = open(os.path.join(ROOT, "radiance-ray-tracing_amd", "build.py")).read()
    assert '"shade.hip"' in build and '"shade.h"' in build


def test_shade_on_an_uninitialised_library_names_rdx_init(mods):
    """(a fresh process: the suite's other tests may have initialised the library in this one)"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import rrt_amd\n"
            "from radiance_ray_tracing_amd import _lib\n"
            "L = _lib.lib()\n"
            "rc = L.rdx_shade_hits(None, None, 0, None, 0, None, 0, 0, None, None, 0, None, 0, None, 0, None, 0, None, None)\n"
            "print(rc, _lib.last_error())\n") % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rc, msg = out.stdout.strip().split(None, 1)
    assert int(rc) < 0 and "rdx_init" in msg, out.stdout


@pytest.mark.parametrize("case", sh.bounds_table(), ids=lambda c: c[0])
def test_bounds_rule(mods, case):
    """rdx_debug_shade_in_bounds needs no device: the rule the kernel applies to every record, on the host"""
    rd = mods[1]
    what, kw, want = case
    assert sh.bounds_answer(rd, kw) is want, what


def test_bounds_rule_is_the_surface_rule_on_everything_that_rule_covers(mods):
    """with textures on (the uv stream counts) and a material table every instance points into, the extended rule answers what
    rdx_debug_surface_in_bounds answers -- except where 3 * item + 2 leaves 32 bits, which only the shader's arithmetic forbids"""
    import surface_cases as sc
    rd = mods[1]
    mi, mt, nidx, nn, nuv = sh.bounds_scene()
    for what, kw, want in sc.bounds_table():
        items = [kw["prim"]] + list(kw["idx3"] or ())
        if want and max(items) > 0x55555554:
            continue
        m = np.zeros(2, sh.MESH_INFO_DTYPE)
        src = kw.get("mi", mi)
        for f in ("vertexOffset", "indexOffset", "uvOffset", "normalOffset"):
            m[f] = src[f]
        nuv_ = kw.get("nuv", nuv)
        got = rd.DebugShadeInBounds(m, kw.get("ninst", 2), kw["inst"], kw["prim"], kw["idx3"], kw.get("nindex", nidx), kw.get("nnormal", nn),
                                    nuv_, mt, textures=nuv_ != 0, layers=sh.LAYERS, nmeshinfo=kw.get("nmeshinfo"))
        assert got is want, what


def test_bounds_rule_accepts_every_triangle_of_a_real_scene(mods):
    rd, scenes = mods[1], mods[2]
    s = gc.small_scene(scenes, "c1")
    b = s.buffers()
    mi, idx, mt = b["meshInfo"], b["index"], b["material"]
    ni, nn, nu = idx.shape[0], b["normal"].shape[0], b["uv"].shape[0]
    for inst, (mesh, _, _) in enumerate(s.instances):
        ntri = s.meshes[mesh][1].shape[0]
        for prim in (0, ntri // 2, ntri - 1):
            at = int(mi[inst]["indexOffset"]) + 3 * prim
            for tex in (False, True):
                assert rd.DebugShadeInBounds(mi, len(mi), inst, prim, idx[at:at + 3], ni, nn, nu, mt, textures=tex, layers=1), (inst, prim, tex)
            assert not rd.DebugShadeInBounds(mi, len(mi), inst, prim, idx[at:at + 3], ni, nn, nu, mt, nmaterials=int(mi[inst]["materialIndex"]))


def test_compose_frames_reproduces_the_oracles_own_frames(mods):
    """the restated raygen loop, driven by the oracle's seams (trace_batch, material_batch, generate_rays), gives the imageScratch of
    the oracle's own raygen (orc_render) for both progressive frames of c0, bit for bit"""
    _, rd, scenes = mods
    s = gc.small_scene(scenes, "c0")
    blob = gc.scene_blob(rd, s)
    osc = ob.OracleScene(s, blob)
    p = osc.rtprop[0]
    generate, bounce = sh.oracle_callables(ob.OracleScene(s, blob), blob)
    got = sh.compose_frames(s.width * s.height, int(p["totalSamples"]), int(p["batchSize"]), int(p["depth"]), 2, generate, bounce)
    assert int(p["batchSize"]) == 2 and int(p["depth"]) == 3
    for f in range(2):
        osc.frame()
        want = osc.scratch.reshape(-1, 4)
        same = (sh.bits(got[f]) == sh.bits(want)).all(1)
        assert same.all(), "frame %d: %d of %d pixels differ" % (f, int((~same).sum()), same.shape[0])
    assert not np.array_equal(got[0], got[1]) and got[1][:, :3].any()


def test_compose_frames_branches():
    """a hand-made scene of three pixels: pixel 0 misses at once (miss colour), pixel 1 hits twice then misses (the later miss
    adds nothing), pixel 2 hits to the depth limit; two samples per frame, two frames: the running mean"""
    F = np.float32
    col = {0: F(0.25), 1: F(0.5), 2: F(0.125)}

    def generate(px, rnd):
        assert rnd[:, 2].tolist() == px.tolist() and len(set(rnd[:, 1])) == 1 and (rnd[:, 0] >= rnd[:, 1]).all()
        o = np.zeros((px.shape[0], 3), F)
        o[:, 0] = px
        return o, np.zeros((px.shape[0], 3), F)

    def bounce(o, d, frame, pixels, depth):
        assert np.array_equal(o[:, 0].astype(np.uint32), pixels)
        hit = np.array([(p == 1 and depth < 2) or p == 2 for p in pixels])
        pc = np.where(hit[:, None], col[depth], sh.ENVIRONMENT[None]).astype(F) * F(frame + 1)
        return hit, pc, np.full((len(pixels), 3), 0.5, F), o, d
    got = sh.compose_frames(3, 0, 2, 3, 2, generate, bounce)

    def sample(p, frame):
        k = F(frame + 1)
        if p == 0:
            return sh.ENVIRONMENT * k
        terms = [col[0] * k, F(0.5) * (col[1] * k)] + ([F(0.25) * (col[2] * k)] if p == 2 else [])
        return np.full(3, sum(terms[1:], terms[0]), F)
    for p in range(3):
        acc = sample(p, 0)
        for frame in (1, 2, 3):
            acc = ((F(frame) * acc + sample(p, frame)) / F(frame + 1)).astype(F)
            if frame == 1:
                assert np.array_equal(sh.bits(got[0][p, :3]), sh.bits(acc)), p
        assert np.array_equal(sh.bits(got[1][p, :3]), sh.bits(acc)), p
    assert not got[1][:, 3].any()


def test_the_recordings_hold_both_branches_of_the_shadow_test(mods):
    """what test 1 of test_gpu_shade.py relies on: over the three scenes at least 100 recorded payloads are lit and at least 100
    are the ambient term alone (the shadow ray was occluded)"""
    scenes = mods[2]
    lit = occ = 0
    for name in gc.SCENES:
        G = np.load(os.path.join(GOLD, "refgpu_%s.npz" % name))
        h = np.ascontiguousarray(G["mat_hits"]).view(ob.HIT_DTYPE).reshape(-1)
        pay = np.ascontiguousarray(G["mat_payload"]).view(ob.PAYLOAD_DTYPE).reshape(-1)
        a, b = sh.recorded_branches(gc.small_scene(scenes, name), h, pay)
        print("%s: %d hits, lit %d, occluded %d" % (name, int((h["hit"] == 1).sum()), a, b))
        lit, occ = lit + a, occ + b
    assert lit >= 100 and occ >= 100, (lit, occ)

"""GPU suite (-m gpu): rd.ResolveMaterials / rd.LightHits and their torch variants (rdx_resolve_materials, rdx_light_hits) -- the
evaluated material of a ray query's hits and one directional light's direct term on it, on the device.

The comparand is rd.ShadeHits (rdx_shade_hits), which tests/test_gpu_shade.py holds to the reference's recorded payloads: its
two colours follow from a material record and the lit colour of light 0 by the two float32 operations of
tests/material_cases.py, its shadow rays are those of rdx_light_hits(light = 0), and rd.ResolveHits gives `above` and the face
normal.  The inputs are the 2048 recorded rays of c0 / c1 / c2 (shade_cases.Golden).  Every bar is equality of bits.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import accel_layout_cases as alc
import golden_cases as gc
import material_cases as mc
import ray_edge_cases as rec
import shade_cases as sh
import tlas_update_cases as tu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
same, bits = mc.same, mc.bits


@pytest.fixture(scope="module")
def mods(gpu):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd, scenes
    return rd, scenes


@pytest.fixture(scope="module")
def golden(mods):
    rd, scenes = mods
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = sh.Golden(rd, scenes, name)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def shaded(mods, golden):
    """query + shade + shadow query of a golden scene's 2048 recorded rays, not compacting (parent code); computed once"""
    rd, _ = mods
    cache = {}

    def get(name):
        if name not in cache:
            c = golden(name)
            cache[name] = sh.shade_batch(rd, c.dev.plt, c.dev.topAccelStruct, c.dev.shading_buffers(), c.mat_rays, c.keys)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def resolved(mods, golden):
    """query + ResolveMaterials + LightHits(0) + shadow query of the same rays; computed once"""
    rd, _ = mods
    cache = {}

    def get(name):
        if name not in cache:
            c = golden(name)
            cache[name] = mc.material_batch(rd, c.dev.plt, c.dev.topAccelStruct, c.dev.shading_buffers(), c.mat_rays)
        return cache[name]
    return get


# ---- 1. against rdx_shade_hits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.SCENES)
def test_against_shade_hits(mods, golden, shaded, resolved, name):
    """hit, materialIndex, both colours and the shadow rays of rd.ShadeHits follow from the material records and light 0; `above`
    and -- without a normal map -- `normal` are rd.ResolveHits'; the parameters are the Material table's, clamped"""
    rd, _ = mods
    c, r, m = golden(name), shaded(name), resolved(name)
    assert m["invalid"] == 0 and r["invalid"] == 0 and same(m["q"], r["q"])
    mc.check_against_shade(m, r, name)
    mat = m["mat"]
    k = mat["hit"] == 1
    assert 0 < int(k.sum()) and int(k.sum()) == r["live"]
    bS, invalid = rd.ResolveHits(c.dev.topAccelStruct, m["bR"], m["bH"], k.shape[0], c.dev.surface_buffers())
    surf = sh.read(rd, c.dev.plt, bS, k.shape[0], rd.SURFACE_DTYPE)
    assert invalid == 0 and np.array_equal(surf["hit"], mat["hit"]) and np.array_equal(surf["materialIndex"], mat["materialIndex"])
    assert mc.all_finite(surf["above"], surf["normal"])
    assert np.array_equal(bits(mat["above"]), bits(surf["above"])), name
    w = mc.table_props(c.b["material"], mat["materialIndex"][k])
    plain = w["plain"]
    assert plain["normal"].any() and np.array_equal(bits(mat["normal"][k][plain["normal"]]), bits(surf["normal"][k][plain["normal"]])), name
    for f in ("albedo", "metallic", "roughness"):
        assert plain[f].any() and np.array_equal(bits(mat[f][k][plain[f]]), bits(w[f][plain[f]])), (name, f)
    for f in ("transmission", "ior"):
        assert np.array_equal(bits(mat[f][k]), bits(w[f])), (name, f)
    shows = (bits(r["shade"]["color"]) != bits(r["shade"]["colorOccluded"])).any(1) & k
    print("%s: %d hits of %d, direct term non-zero on %d, occluded %d" % (name, int(k.sum()), k.shape[0], int(shows.sum()), int(m["occluded"].sum())))
    assert shows.sum() >= 100


# ---- 2. every light ------------------------------------------------------------------------------------------------------------------
def test_every_light(mods, golden):
    """c1 under a SceneProperties of three lights: light j through rd.LightHits equals rd.ShadeHits on a scene buffer whose
    lights[0] is light j -- colour and shadow rays -- and the lights differ"""
    rd, _ = mods
    c = golden("c1")
    dev, plt, tlas = c.dev, c.dev.plt, c.dev.topAccelStruct
    sp = mc.three_lights(rd)
    scene3 = sh.upload(rd, plt, np.array(sp).reshape(1))
    base = mc.material_batch(rd, plt, tlas, dev.shading_buffers(), c.mat_rays, want_shadow=False)
    mat, n = base["mat"], c.mat_rays.shape[0]
    k = mat["hit"] == 1
    lits, below = [], []
    for j in range(3):
        m = mc.light_batch(rd, plt, tlas, base["bR"], base["bM"], n, scene3, j)
        sb = dev.shading_buffers()
        sb.scene = sh.upload(rd, plt, mc.with_first_light(rd, sp, j).reshape(1))
        r = sh.shade_batch(rd, plt, tlas, sb, c.mat_rays, c.keys)
        assert r["invalid"] == 0 and np.array_equal(r["shade"]["hit"], mat["hit"])
        assert mc.all_finite(m["lit"]["rgb"], r["shade"]["color"])
        eq = (bits(mc.color_lit(m["lit"]["rgb"][k], mat["albedo"][k])) == bits(r["shade"]["color"][k])).all(1)
        assert eq.all(), "light %d: colour differs on %d of %d hits" % (j, int((~eq).sum()), eq.shape[0])
        assert (bits(mc.color_occluded(mat["albedo"][k])) == bits(r["shade"]["colorOccluded"][k])).all()
        assert same(m["shadow"], r["shadow"]), j
        assert np.array_equal(m["occluded"], r["occluded"]), j
        assert not m["lit"][~k].view(np.uint8).any() and not bits(m["lit"]["w"]).any()
        lits.append(m["lit"]["rgb"][k])
        below.append(int((~bits(m["lit"]["rgb"][k]).any(1)).sum()))
    print("every light: %d hits, direct term zero on %s of them per light" % (int(k.sum()), below))
    assert not same(lits[1], lits[0]) and not same(lits[2], lits[0]) and not same(lits[2], lits[1])
    assert below[1] > below[0]          # light 1 shines upwards: the direct term is exactly zero on every surface that faces up


# ---- 3. frames ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.SCENES)
def test_frames_with_the_colour_from_material_records(mods, golden, name):
    """the raygen loop with each bounce's colour from ResolveMaterials + LightHits(0) + the any-hit query + the ambient term (next
    ray and factor from ShadeHits): imageScratch of both progressive frames equals the reference's recorded frames"""
    rd, _ = mods
    c = golden(name)
    dev, p = c.dev, c.s.rtprop
    dev.bind()
    generate, bounce = mc.gpu_callables(rd, dev)
    got = sh.compose_frames(dev.width * dev.height, 0, int(p["batchSize"]), int(p["depth"]), 2, generate, bounce)
    for f in range(2):
        want = np.ascontiguousarray(c.G["scratch%d" % f]).reshape(-1, 4)
        assert mc.all_finite(got[f], want)
        eq = (bits(got[f]) == bits(want)).all(1)
        assert eq.all(), "%s frame %d: %d of %d pixels differ from the recording" % (name, f, int((~eq).sum()), eq.shape[0])


# ---- 4. textures ----------------------------------------------------------------------------------------------------------------------
def test_textures(mods):
    """a scene in which each of the four texture indices is set on some material: option "textures" 0, then 1 with a repeat /
    linear and a clamp / nearest sampler -- identity 1 holds against rd.ShadeHits under the same settings, and the records differ"""
    rd, scenes = mods
    s = mc.textured_scene(scenes)
    dev = scenes.DeviceScene(s)
    plt, tlas = dev.plt, dev.topAccelStruct
    tex = mc.textures()
    img = rd.CreateImageArray(plt, 16, 16, 3)
    for l in range(3):
        rd.WriteImage(plt, img, 16, 16, l, tex[l])
    px = np.arange(s.width * s.height, dtype=np.uint32)
    o, d = rd.GenerateBatch(px, np.stack([np.zeros_like(px), np.zeros_like(px), px], 1))
    rays, keys = sh.rays_of(rd, o, d), sh.keys_of((px % 5).astype(np.uint32), px, (px % 3).astype(np.uint32))
    outs = []
    try:
        for textures, addr, filt in ((0, rd.RD_ADDRESS_REPEAT, rd.RD_FILTER_LINEAR), (1, rd.RD_ADDRESS_REPEAT, rd.RD_FILTER_LINEAR),
                                     (1, rd.RD_ADDRESS_CLAMP, rd.RD_FILTER_NEAREST)):
            rd.SetOption("textures", textures)
            sb = dev.shading_buffers(img, rd.CreateSampler(plt, addr, filt))
            m = mc.material_batch(rd, plt, tlas, sb, rays)
            r = sh.shade_batch(rd, plt, tlas, sb, rays, keys)
            assert m["invalid"] == 0 and r["invalid"] == 0
            mc.check_against_shade(m, r, "textures %d sampler %s/%s" % (textures, addr, filt))
            outs.append(m["mat"].copy())
        k = outs[0]["hit"] == 1
        assert set(np.unique(outs[0]["materialIndex"][k])) == {0, 1, 2}
        # texel 0 with textures off: albedo 0, metallic 0, roughness at its floor, and a normal that is NOT the face normal
        surf = sh.read(rd, plt, rd.ResolveHits(tlas, m["bR"], m["bH"], px.shape[0], dev.surface_buffers())[0], px.shape[0], rd.SURFACE_DTYPE)
        off = outs[0]
        assert not bits(off["albedo"][k]).any()
        m1, m2 = k & (off["materialIndex"] == 1), k & (off["materialIndex"] == 2)
        assert m1.sum() > 20 and m2.sum() > 20
        assert not bits(off["metallic"][m1]).any() and (bits(off["roughness"][m1]) == bits(F(0.05))).all()
        assert (bits(off["normal"][m2]) != bits(surf["normal"][m2])).any(1).all()
        assert (bits(off["normal"][k & ~m2]) == bits(surf["normal"][k & ~m2])).all()
        for a, b in ((0, 1), (1, 2), (0, 2)):
            for f in ("albedo", "normal", "roughness", "metallic"):
                assert not same(outs[a][f], outs[b][f]), (a, b, f)
            for f in ("hit", "materialIndex", "above", "transmission", "ior"):
                assert same(outs[a][f], outs[b][f]), (a, b, f)
        # textures on without an image array: texel 0, as with textures off
        assert same(mc.material_batch(rd, plt, tlas, dev.shading_buffers(), rays, want_shadow=False)["mat"], outs[0])
        with pytest.raises(rd.RadianceError, match="uv"):
            rd.ResolveMaterials(tlas, m["bR"], m["bH"], px.shape[0],
                                rd.ShadingBuffers(dev.rdSceneData, dev.meshInfoData, dev.indexData, None, dev.normalData, dev.materialData, img))
    finally:
        rd.SetOption("textures", 0)


# ---- 5. bounds ------------------------------------------------------------------------------------------------------------------------
def test_records_that_point_outside_a_buffer_are_zeroed_and_counted(mods, golden, shaded):
    """the construction of test_gpu_shade.py: 4 KiB of slack behind every stream, views of the content alone, 64 of c1's 2048
    records each breaking one rule by less than the slack -- 64 counted, 64 zero records, the other 1984 bit for bit as before"""
    rd, _ = mods
    c = golden("c1")
    plt, tlas = c.dev.plt, c.dev.topAccelStruct
    sb, ok, bad, poisoned, check = mc.bounds_case(rd, c, shaded("c1")["q"])
    rd.SetOption("textures", 1)
    try:
        check(bad, poisoned)
        base = mc.material_batch(rd, plt, tlas, sb, c.mat_rays, hits=ok)
        assert base["invalid"] == 0 and (base["mat"]["hit"] == 1).all()
        # (none of c1's materials has a texture: with valid records the views and the image change nothing)
        own = mc.material_batch(rd, plt, tlas, c.dev.shading_buffers(), c.mat_rays, hits=ok, want_shadow=False)
        assert same(own["mat"], base["mat"])
        got = mc.material_batch(rd, plt, tlas, sb, c.mat_rays, hits=bad)
        assert got["invalid"] == 64 and int(poisoned.sum()) == 64
        assert not got["mat"][poisoned].view(np.uint8).any(), "poisoned records came back non-zero"
        assert (got["mat"]["hit"][~poisoned] == 1).all()
        assert not got["lit"][poisoned].view(np.uint8).any() and not got["shadow"][poisoned].view(np.uint8).any()
        for f in ("mat", "lit", "shadow"):
            assert same(got[f][~poisoned], base[f][~poisoned]), f
    finally:
        rd.SetOption("textures", 0)


# ---- 6. shapes, offsets, refusals -----------------------------------------------------------------------------------------------------
def test_shapes(mods, golden, resolved):
    """n in {0, 1, 63, 64, 65, 255, 256, 257}: the corresponding rows of the 2048-record run (rows 700.. of c0 hold hits and misses)"""
    rd, _ = mods
    c, full = golden("c0"), resolved("c0")
    plt, tlas, sb = c.dev.plt, c.dev.topAccelStruct, c.dev.shading_buffers()
    first = 700
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        rows = slice(first, first + n)
        up = lambda a: sh.upload(rd, plt, a) if n else rd.CreateBuffer(plt, 16)
        bR, bH = up(c.mat_rays[rows]), up(full["q"][rows])
        bM, invalid = rd.ResolveMaterials(tlas, bR, bH, n, sb)
        assert invalid == 0 and same(sh.read(rd, plt, bM, n, mc.MATERIAL_RECORD_DTYPE), full["mat"][rows]), n
        bL, bSh = rd.LightHits(bR, bM, n, sb.scene, 0)
        assert same(sh.read(rd, plt, bL, n, mc.LIT_DTYPE), full["lit"][rows]) and same(sh.read(rd, plt, bSh, n, rd.RAY_DTYPE), full["shadow"][rows]), n
        bL2, none = rd.LightHits(bR, bM, n, sb.scene, 0, shadow=None)
        assert none is None and same(sh.read(rd, plt, bL2, n, mc.LIT_DTYPE), full["lit"][rows]), n
    hit = full["mat"]["hit"][first:first + 257] == 1
    assert 0 < int(hit.sum()) < 257


def _refusals(rd, run, cases, snapshot, good, symbol):
    for what, kw, word in cases:
        with pytest.raises(rd.RadianceError) as e:
            run(**kw)
        assert word in str(e.value) and symbol in str(e.value), (what, str(e.value))
        now = snapshot()
        for k in now:
            assert np.array_equal(now[k], good[k]), (what, k)


def test_offsets_and_refusals(mods, golden, resolved):
    """n = 200 of c1's records at distinct non-zero offsets in buffers filled with 0xA5: the records equal the plain call's and no
    byte outside the written ranges is touched; one refusal of each kind, after each of which every buffer is unchanged; material
    records of the caller's own with hit = 2 or garbage normals write only their own ranges"""
    rd, _ = mods
    c, plain = golden("c1"), resolved("c1")
    dev, plt, tl = c.dev, c.dev.plt, c.dev.topAccelStruct
    sb = dev.shading_buffers()
    n, tail = 200, 128
    off = dict(rays=96, hits=160, mat=192, lit=48, shadow=32)
    rec_size = dict(rays=32, hits=32, mat=64, lit=16, shadow=32)
    B = {k: rd.CreateBuffer(plt, off[k] + rec_size[k] * n + tail) for k in off}
    fill = lambda buf: rd.WriteBuffer(plt, buf, buf.size, np.full(buf.size, 0xA5, np.uint8))
    for buf in B.values():
        fill(buf)
    rd.WriteBuffer(plt, B["rays"], 32 * n, c.mat_rays[:n], offset=off["rays"])
    rd.WriteBuffer(plt, B["hits"], 32 * n, plain["q"][:n], offset=off["hits"])
    snapshot = lambda: {k: rd.ReadBuffer(plt, B[k], B[k].size).copy() for k in B}

    def resolve(**kw):
        a = dict(tlas=tl, rays=B["rays"], hits=B["hits"], n=n, scene_buffers=sb, out=B["mat"], rays_offset=off["rays"], hits_offset=off["hits"],
                 out_offset=off["mat"])
        a.update(kw)
        return rd.ResolveMaterials(a.pop("tlas"), a.pop("rays"), a.pop("hits"), a.pop("n"), a.pop("scene_buffers"), **a)

    def light(**kw):
        a = dict(rays=B["rays"], materials=B["mat"], n=n, scene=sb.scene, light=0, lit=B["lit"], shadow=B["shadow"], rays_offset=off["rays"],
                 materials_offset=off["mat"], lit_offset=off["lit"], shadow_offset=off["shadow"])
        a.update(kw)
        return rd.LightHits(a.pop("rays"), a.pop("materials"), a.pop("n"), a.pop("scene"), a.pop("light"), **a)

    before = snapshot()
    assert resolve() == (B["mat"], 0)
    assert light() == (B["lit"], B["shadow"])
    after = snapshot()
    for k in ("rays", "hits"):
        assert np.array_equal(after[k], before[k]), k
    for k, want in (("mat", plain["mat"]), ("lit", plain["lit"]), ("shadow", plain["shadow"])):
        lo, hi = off[k], off[k] + rec_size[k] * n
        assert same(after[k][lo:hi], want[:n]), k
        assert (after[k][:lo] == 0xA5).all() and (after[k][hi:] == 0xA5).all(), k
    # n == 0 touches nothing
    for k in ("lit", "shadow"):
        fill(B[k])
    fill(B["mat"])
    assert resolve(n=0) == (B["mat"], 0) and light(n=0) == (B["lit"], B["shadow"])
    assert all((rd.ReadBuffer(plt, B[k], B[k].size) == 0xA5).all() for k in ("mat", "lit", "shadow"))
    resolve(); light()
    good = snapshot()

    one = rd.CreateBuffer(plt, 32 * n * 8)          # rays | hits | room for outputs, for the overlap cases
    rd.WriteBuffer(plt, one, 32 * n, c.mat_rays[:n])
    rd.WriteBuffer(plt, one, 32 * n, plain["q"][:n], offset=32 * n)
    rd.WriteBuffer(plt, one, 64 * n, plain["mat"][:n], offset=64 * n)
    null, unknown = rd.Buffer(None, 1 << 20), rd.Buffer(12345678, 1 << 20)
    S = lambda **kw: rd.ShadingBuffers(**{**dict(scene=dev.rdSceneData, meshInfo=dev.meshInfoData, index=dev.indexData, uv=dev.uvData, normal=dev.normalData,
                                                material=dev.materialData), **kw})
    in_one = dict(rays=one, hits=one, rays_offset=0, hits_offset=32 * n)
    _refusals(rd, resolve, [
        ("rays_offset 8", dict(rays_offset=8), "16"), ("hits_offset 8", dict(hits_offset=8), "16"), ("out_offset 24", dict(out_offset=24), "16"),
        ("rays past the end", dict(rays_offset=off["rays"] + tail + 16), "ray buffer"),
        ("records past the end", dict(hits_offset=off["hits"] + tail + 16), "hit buffer"),
        ("out past the end", dict(out_offset=off["mat"] + tail + 16), "output buffer"),
        ("out one record short", dict(out=rd.CreateBuffer(plt, 64 * n - 16), out_offset=0), "output buffer"),
        ("out over the rays", dict(in_one, out=one, out_offset=32 * n - 64), "overlap"),
        ("out over the records", dict(in_one, out=one, out_offset=64 * n - 64), "overlap"),
        ("null tlas", dict(tlas=null), "TLAS"), ("null rays", dict(rays=null), "ray buffer handle"), ("unknown hits", dict(hits=unknown), "hit buffer handle"),
        ("null out", dict(out=null), "output buffer handle"),
        ("null scene", dict(scene_buffers=S(scene=null)), "SceneProperties"), ("null meshInfo", dict(scene_buffers=S(meshInfo=null)), "meshInfo"),
        ("null index", dict(scene_buffers=S(index=null)), "index"), ("null normal", dict(scene_buffers=S(normal=null)), "normal"),
        ("null material", dict(scene_buffers=S(material=null)), "material"), ("unknown uv", dict(scene_buffers=S(uv=rd.Buffer(12345678, 64))), "uv"),
        ("unknown textureArray", dict(scene_buffers=S(textureArray=rd.Buffer(12345678, 64))), "textureArray"),
        ("a scene buffer smaller than SceneProperties", dict(scene_buffers=S(scene=rd.CreateBuffer(plt, 160))), "SceneProperties"),
        ("misaligned wrapped rays", dict(rays=rd.WrapDeviceMemory(plt, B["rays"].device_ptr + 8, 32 * n + 64, keepalive=B["rays"]), rays_offset=16), "aligned"),
        ("misaligned wrapped out", dict(out=rd.WrapDeviceMemory(plt, B["mat"].device_ptr + 4, 64 * n + 64, keepalive=B["mat"]), out_offset=0), "aligned"),
        ("misaligned wrapped index stream", dict(scene_buffers=S(index=rd.WrapDeviceMemory(plt, dev.indexData.device_ptr + 2, dev.indexData.size - 2, keepalive=dev.indexData))), "aligned"),
    ], snapshot, good, "rdx_resolve_materials")
    in_one = dict(rays=one, materials=one, rays_offset=0, materials_offset=64 * n)
    small = rd.CreateBuffer(plt, 160)
    _refusals(rd, light, [
        ("rays_offset 8", dict(rays_offset=8), "16"), ("materials_offset 8", dict(materials_offset=8), "16"), ("lit_offset 4", dict(lit_offset=4), "16"),
        ("shadow_offset 24", dict(shadow_offset=24), "16"),
        ("rays past the end", dict(rays_offset=off["rays"] + tail + 16), "ray buffer"),
        ("records past the end", dict(materials_offset=off["mat"] + tail + 16), "material-record buffer"),
        ("lit past the end", dict(lit_offset=off["lit"] + tail + 16), "lit buffer"),
        ("shadow past the end", dict(shadow_offset=off["shadow"] + tail + 16), "shadow-ray buffer"),
        ("shadow one record short", dict(shadow=rd.CreateBuffer(plt, 32 * n - 16), shadow_offset=0), "shadow-ray buffer"),
        ("lit over the rays", dict(in_one, lit=one, lit_offset=32 * n - 16), "overlap"),
        ("lit over the records", dict(in_one, lit=one, lit_offset=128 * n - 16), "overlap"),
        ("shadow over the records", dict(in_one, shadow=one, shadow_offset=64 * n), "overlap"),
        ("shadow over lit", dict(lit=one, lit_offset=128 * n, shadow=one, shadow_offset=144 * n - 32), "overlap"),
        ("lit over the SceneProperties", dict(lit=rd.WrapDeviceMemory(plt, dev.rdSceneData.device_ptr, 16, keepalive=dev.rdSceneData), lit_offset=0, n=1), "overlap"),
        ("null rays", dict(rays=null), "ray buffer handle"), ("unknown materials", dict(materials=unknown), "material-record buffer handle"),
        ("null scene", dict(scene=null), "SceneProperties"), ("null lit", dict(lit=null), "lit buffer handle"),
        ("unknown shadow", dict(shadow=unknown), "shadow-ray buffer handle"),
        ("a scene buffer smaller than SceneProperties", dict(scene=small), "SceneProperties"),
        ("misaligned wrapped records", dict(materials=rd.WrapDeviceMemory(plt, B["mat"].device_ptr + 8, 64 * n + 64, keepalive=B["mat"]), materials_offset=0), "aligned"),
        ("misaligned wrapped lit", dict(lit=rd.WrapDeviceMemory(plt, B["lit"].device_ptr + 4, 16 * n + 32, keepalive=B["lit"]), lit_offset=0), "aligned"),
    ], snapshot, good, "rdx_light_hits")
    # light > 4 at the C ABI (rd.LightHits refuses it before the library sees it), and a NULL scene struct
    from radiance_ray_tracing_amd import _lib
    L = _lib.lib()
    for bad_light in (5, 0xffffffff):
        assert L.rdx_light_hits(B["rays"].handle, off["rays"], B["mat"].handle, off["mat"], n, sb.scene.handle, bad_light, B["lit"].handle, off["lit"], None, 0) != 0
        assert "light" in _lib.last_error() and "rdx_light_hits" in _lib.last_error()
    assert L.rdx_resolve_materials(tl.handle, B["rays"].handle, 0, B["hits"].handle, 0, n, None, B["mat"].handle, 0, None) != 0
    assert "scene" in _lib.last_error()
    unknown_sampler = _lib.rdx_shading_buffers(dev.rdSceneData.handle, dev.meshInfoData.handle, dev.indexData.handle, None, dev.normalData.handle,
                                              dev.materialData.handle, None, 12345678)
    assert L.rdx_resolve_materials(tl.handle, B["rays"].handle, 0, B["hits"].handle, 0, n, C.byref(unknown_sampler), B["mat"].handle, 0, None) != 0
    assert "sampler" in _lib.last_error()
    assert all(np.array_equal(v, good[k]) for k, v in snapshot().items())
    # adjacent ranges of one buffer are fine, and the calls still work after the refusals: rays | records | material records | lit | shadow
    assert rd.ResolveMaterials(tl, one, one, n, sb, one, 0, 32 * n, 64 * n)[1] == 0
    rd.LightHits(one, one, n, sb.scene, 0, one, one, 0, 64 * n, 128 * n, 144 * n)
    assert same(rd.ReadBuffer(plt, one, 64 * n, offset=64 * n), plain["mat"][:n]) and same(rd.ReadBuffer(plt, one, 16 * n, offset=128 * n), plain["lit"][:n])
    assert same(rd.ReadBuffer(plt, one, 32 * n, offset=144 * n), plain["shadow"][:n])
    for fn in (lambda: resolve(scene_buffers=[dev.meshInfoData]), lambda: resolve(out=7), lambda: light(lit=7), lambda: light(shadow=7), lambda: light(scene=None)):
        with pytest.raises(rd.RadianceError):
            fn()

    # material records of the caller's own: hit = 2 -> zeros; hit = 1 with garbage normals -> whatever the arithmetic gives, inside
    # the output ranges (the kernel gathers nothing, so there is nothing a record could make it read)
    own = plain["mat"][:n].copy()
    own["hit"][0::4] = 2
    garbage = np.arange(n) % 4 == 1
    own["hit"][garbage] = 1
    own["normal"][garbage] = np.resize(np.array([[np.nan, 0, 0], [np.inf, -np.inf, 0], [0, 0, 0], [3e38, 3e38, 3e38], [1e-42, 0, 0]], F), (int(garbage.sum()), 3))
    rd.WriteBuffer(plt, B["mat"], 64 * n, own, offset=off["mat"])
    for k in ("lit", "shadow"):
        fill(B[k])
    light()
    now = snapshot()
    for k in ("lit", "shadow"):
        lo, hi = off[k], off[k] + rec_size[k] * n
        assert (now[k][:lo] == 0xA5).all() and (now[k][hi:] == 0xA5).all(), k
    lit = now["lit"][off["lit"]:off["lit"] + 16 * n].view(mc.LIT_DTYPE)
    shadow = now["shadow"][off["shadow"]:off["shadow"] + 32 * n].view(rd.RAY_DTYPE)
    assert not np.ascontiguousarray(lit[0::4]).view(np.uint8).any() and not np.ascontiguousarray(shadow[0::4]).view(np.uint8).any()
    untouched = (np.arange(n) % 4 >= 2) & (plain["mat"]["hit"][:n] == 1)
    assert untouched.any() and same(lit[untouched], plain["lit"][:n][untouched]) and same(shadow[untouched], plain["shadow"][:n][untouched])
    assert not bits(lit["w"]).any()
    assert (bits(shadow["tmax"][garbage]) == bits(F(1000.0))).all() and same(shadow["origin"][garbage], own["above"][garbage])


# ---- 7. after UpdateAccelStruct -----------------------------------------------------------------------------------------------------
def _decorated(scenes, name):
    """accel_layout_cases.scene(name) with a camera, a light and one material per custom id (as tests/test_gpu_shade.py)"""
    s = alc.scene(name)
    nmat = 1 + max(mat for _, _, mat in s.instances)
    s.materials = [scenes.material((0.25 + 0.07 * (k % 9), 0.8 - 0.06 * (k % 7), 0.3 + 0.05 * (k % 5)), 0.1 * (k % 3), 0.4 + 0.05 * (k % 4)) for k in range(nmat)]
    s.camera = scenes.blender_camera(64, 36, 0.05, 0.036, 12.0, 0.0, (1.0, 12.0, 2.5), (-100.0, 180.0, 0.0))
    s.sceneProps = scenes.blender_dir_light(-45.0, 20.0, 5.0)
    s.rtprop = scenes._rtprop(0, 2, 3)
    return s


def test_after_update_accel_struct(mods):
    """the 9-instance grid sharing two BLAS: the last instance is carried far away, then the first nudged.  Each time the material
    records, lit colours and shadow rays are bitwise what a freshly built TLAS gives, and differ from those before the move"""
    rd, scenes = mods
    s = _decorated(scenes, "shared_blas")
    dev = scenes.DeviceScene(s)
    o, d = rec.own_primary_rays(s, 2048)
    rays = sh.rays_of(rd, o, d)
    prev = mc.material_batch(rd, dev.plt, dev.topAccelStruct, dev.shading_buffers(), rays)
    assert prev["invalid"] == 0 and 100 <= int((prev["mat"]["hit"] == 1).sum()) < rays.shape[0]
    insts = tu.instances(s)
    for move in ("B", "A"):
        insts = tu.apply(insts, move)
        rd.UpdateAccelStruct(dev.plt, dev.topAccelStruct, tu.rd_instances(rd, insts, dev.blas))
        got = mc.material_batch(rd, dev.plt, dev.topAccelStruct, dev.shading_buffers(), rays)
        t = scenes.Scene(s.name)
        t.meshes, t.materials, t.camera, t.sceneProps, t.rtprop = s.meshes, s.materials, s.camera, s.sceneProps, s.rtprop
        for mi, tf, sbt, mat in insts:
            t.add_instance(mi, tf, mat, sbt)
        fresh = scenes.DeviceScene(t)
        want = mc.material_batch(rd, fresh.plt, fresh.topAccelStruct, fresh.shading_buffers(), rays)
        assert got["invalid"] == 0 and want["invalid"] == 0
        for k in ("q", "mat", "lit", "shadow", "occluded"):
            assert same(got[k], want[k]), (move, k)
        assert not same(got["mat"], prev["mat"]), move
        prev = got


# ---- 8. torch variants ---------------------------------------------------------------------------------------------------------------
_TORCH_CHILD = r"""
import os, sys
ROOT = sys.argv[1]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
assert torch.cuda.is_available()
torch.zeros(1, device="cuda").cpu()                      # torch initialises the GPU first (tests/test_cpu_oracle._gpu_present)
import numpy as np
import rrt_amd
from radiance_ray_tracing_amd import rd, scenes
import material_cases as mc
import shade_cases as sh
c = sh.Golden(rd, scenes, "c1")
dev, n = c.dev, c.mat_rays.shape[0]
tlas, sb = dev.topAccelStruct, dev.shading_buffers()
scene3 = sh.upload(rd, dev.plt, np.array(mc.three_lights(rd)).reshape(1))
want = mc.material_batch(rd, dev.plt, tlas, sb, c.mat_rays, scene=scene3, light=2)
hit = want["mat"]["hit"] == 1
assert 0 < int(hit.sum())
# the tensor route, on tensors a torch op produced
t = (torch.from_numpy(c.mat_rays.view(np.float32).reshape(n, 8).copy()).cuda() * torch.ones(8, device="cuda")).contiguous()
h = rd.QueryRaysTorch(tlas, t, rd.QUERY_CLOSEST)
mat, invalid = rd.ResolveMaterialsTorch(tlas, t, h, sb)
assert invalid == 0 and mat.dtype == torch.float32 and tuple(mat.shape) == (n, 16)
assert np.array_equal(mat.cpu().numpy().view(np.uint32), want["mat"].view(np.uint32).reshape(n, 16))
lit, shadow = rd.LightHitsTorch(t, mat, scene3, 2)
assert lit.dtype == torch.float32 and tuple(lit.shape) == (n, 4) and tuple(shadow.shape) == (n, 8)
assert np.array_equal(lit.cpu().numpy().view(np.uint32), want["lit"].view(np.uint32).reshape(n, 4))
assert np.array_equal(shadow.cpu().numpy().view(np.uint32), want["shadow"].view(np.uint32).reshape(n, 8))
lit2, none = rd.LightHitsTorch(t, mat, scene3, 2, want_shadow=False)
assert none is None and torch.equal(lit2.view(torch.int32), lit.view(torch.int32))
# the light loop of the README over the three lights, against the same loop on buffers
direct = torch.zeros((n, 3), device="cuda")
ref = np.zeros((n, 3), np.float32)
for j in range(3):
    lit, shadow = rd.LightHitsTorch(t, mat, scene3, j)
    occluded = rd.QueryRaysTorch(tlas, shadow, rd.QUERY_ANY)[:, 3:4] == 1
    direct += torch.where(occluded, torch.zeros_like(lit[:, :3]), lit[:, :3])
    w = mc.light_batch(rd, dev.plt, tlas, want["bR"], want["bM"], n, scene3, j)
    ref = (ref + np.where(w["occluded"][:, None], np.float32(0), w["lit"]["rgb"])).astype(np.float32)
color = direct + mat[:, 4:7] * 0.1
assert np.isfinite(ref).all() and np.array_equal(direct.cpu().numpy().view(np.uint32), ref.view(np.uint32))
assert np.array_equal(color.cpu().numpy().view(np.uint32), (ref + mc.ambient(want["mat"]["albedo"])).astype(np.float32).view(np.uint32))
# an `out` tensor of the caller's, an int32 hit tensor viewed as float32, n = 0
out = torch.empty((n, 16), dtype=torch.float32, device="cuda")
got, _ = rd.ResolveMaterialsTorch(tlas, t, h.view(torch.float32), sb, out=out)
assert got is out and torch.equal(out.view(torch.int32), mat.view(torch.int32))
e, inv = rd.ResolveMaterialsTorch(tlas, t[:0], h[:0], sb)
assert tuple(e.shape) == (0, 16) and inv == 0
e = rd.LightHitsTorch(t[:0], mat[:0], scene3, 0)
assert tuple(e[0].shape) == (0, 4) and tuple(e[1].shape) == (0, 8)
bad = [lambda: rd.ResolveMaterialsTorch(tlas, t[:, :7], h, sb), lambda: rd.ResolveMaterialsTorch(tlas, t.double(), h, sb),
       lambda: rd.ResolveMaterialsTorch(tlas, t.cpu(), h, sb), lambda: rd.ResolveMaterialsTorch(tlas, t, h[:-1], sb),
       lambda: rd.ResolveMaterialsTorch(tlas, t, h.long(), sb), lambda: rd.ResolveMaterialsTorch(tlas, t, h, sb, out=out[:, :8]),
       lambda: rd.ResolveMaterialsTorch(tlas, c.mat_rays, h, sb),
       lambda: rd.LightHitsTorch(t, mat[:, :8], scene3, 0), lambda: rd.LightHitsTorch(t, mat.double(), scene3, 0),
       lambda: rd.LightHitsTorch(t, mat.cpu(), scene3, 0), lambda: rd.LightHitsTorch(t[:-1], mat, scene3, 0),
       lambda: rd.LightHitsTorch(t, mat, scene3, 5), lambda: rd.LightHitsTorch(t, mat, mat, 0)]
for j, fn in enumerate(bad):
    try:
        fn()
    except rd.RadianceError:
        continue
    raise AssertionError("bad argument set %d was accepted" % j)
print("TORCH-MATERIALS-OK", n, int(hit.sum()))
"""


def test_torch_tensors_in_a_fresh_process(gpu):
    """rd.ResolveMaterialsTorch / rd.LightHitsTorch equal the buffer route bit for bit, the README's light loop included; wrong
    dtype, shape or device is refused in Python.  torch is initialised first, in a process of its own (as tests/test_gpu_shade.py)"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _TORCH_CHILD, ROOT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "TORCH-MATERIALS-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])

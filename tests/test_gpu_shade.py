"""GPU suite (-m gpu): rd.ShadeHits / rd.ShadeHitsTorch (rdx_shade_hits) -- the stock closest-hit shader on the hits of a ray
query, on the device.

Comparands, in this order of authority:
  1. the reference's own device code, recorded (tests/golden/refgpu_c{0,1,2}.npz): its `material` payloads `mat_payload` on the
     primary rays gen_o / gen_d at golden_cases.spread(npix, N_MATERIAL), and its two progressive frames scratch0 / scratch1 --
     reproduced from the public calls alone (GenerateBatch, QueryRays, ShadeHits) by shade_cases.compose_frames, which
     tests/test_shade_cpu.py holds to the CPU oracle's own frames;
  2. where oracle/_ref is built, the same code run live on a scene of instances;
  3. the library's own seam rd.MaterialBatch, for what no recording covers (textures, another shader binding table).
Every bar is equality of bits.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import accel_layout_cases as alc
import golden_cases as gc
import oracle_bind as ob
import ray_edge_cases as rec
import refgpu_bind as rg
import shade_cases as sh
import surface_cases as sc
import tlas_update_cases as tu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U4 = np.dtype("<u4")


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
    """query + shade + shadow query of a golden scene's 2048 recorded rays, not compacting; computed once"""
    rd, _ = mods
    cache = {}

    def get(name):
        if name not in cache:
            c = golden(name)
            cache[name] = sh.shade_batch(rd, c.dev.plt, c.dev.topAccelStruct, c.dev.shading_buffers(), c.mat_rays, c.keys)
        return cache[name]
    return get


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- 1. recorded payloads ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.SCENES)
def test_recorded_payloads(golden, shaded, name):
    """on every hit the reference recorded: hit, the colour its shadow test chose, nextFactor and the next ray, bit for bit"""
    c, r = golden(name), shaded(name)
    assert r["invalid"] == 0 and r["live"] == int((c.mat_hits["hit"] == 1).sum())
    lit, occ = sh.check_against_payloads(r, c.mat_hits, c.mat_pay, name)
    print("%s: %d hits of %d, lit %d, occluded %d" % (name, r["live"], c.mat_hits.shape[0], lit, occ))
    # (the recordings show the same split wherever the surface faces the light by more than rounding: tests/test_shade_cpu.py)
    assert lit >= sh.recorded_branches(c.s, c.mat_hits, c.mat_pay)[0] and occ <= int(r["occluded"].sum())
    k = r["shade"]["hit"] == 1
    assert np.array_equal(r["shade"]["materialIndex"][k], c.mat_hits["instanceCustomIndex"][k])
    # not compacting: slot = the ray's own number, and the record of a ray that does not survive is zeros
    assert np.array_equal(r["shade"]["slot"][k], np.flatnonzero(k).astype(np.uint32))
    assert not r["next"][~k].view(np.uint8).any() and not r["shadow"][~k].view(np.uint8).any()


def test_both_branches_of_the_shadow_test_occur(golden, shaded):
    """over the three scenes at least 100 hits took the lit colour and at least 100 the occluded one, counted where the two differ"""
    lit = occ = 0
    for name in gc.SCENES:
        r, s = shaded(name), shaded(name)["shade"]
        shows = (sh.bits(s["color"]) != sh.bits(s["colorOccluded"])).any(1) & (s["hit"] == 1)
        lit, occ = lit + int((shows & ~r["occluded"]).sum()), occ + int((shows & r["occluded"]).sum())
    assert lit >= 100 and occ >= 100, (lit, occ)


# ---- 2. whole frames from public calls ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.SCENES)
def test_frames_from_public_calls(mods, golden, name):
    """GenerateBatch -> (QueryRays -> ShadeHits, compacting -> QueryRays on the shadow rays -> select -> accumulate) per bounce:
    imageScratch of both progressive frames equals the reference's recorded frames and this library's own TraceRays"""
    rd, _ = mods
    c = golden(name)
    dev, p = c.dev, c.s.rtprop
    dev.bind()
    generate, bounce = sh.gpu_callables(rd, dev)
    got = sh.compose_frames(dev.width * dev.height, 0, int(p["batchSize"]), int(p["depth"]), 2, generate, bounce)
    dev.set_rtprop(totalSamples=0); dev.clear_scratch()
    for f in range(2):
        want = np.ascontiguousarray(c.G["scratch%d" % f]).reshape(-1, 4)
        eq = (sh.bits(got[f]) == sh.bits(want)).all(1)
        assert eq.all(), "%s frame %d: %d of %d pixels differ from the recording" % (name, f, int((~eq).sum()), eq.shape[0])
        dev.render()
        assert same(got[f], dev.read_scratch().reshape(-1, 4)), (name, f)


# ---- 3. compaction ------------------------------------------------------------------------------------------------------------------
def _compaction_batches(golden):
    c = golden("c0")
    hit = c.mat_hits["hit"] == 1
    mixed = np.arange(2048)
    out = [("n=%d" % n, mixed[:n] + (0 if n == 2048 else 700)) for n in (63, 64, 65, 2048)]      # (rows 700.. of c0 hold hits and misses)
    out += [("n=1 hit", np.flatnonzero(hit)[:1]), ("n=1 miss", np.flatnonzero(~hit)[:1]),
            ("all miss", np.flatnonzero(~hit)[:200]), ("all hit", np.flatnonzero(hit)[:200])]
    return c, out


def test_compaction(mods, golden):
    rd, _ = mods
    c, batches = _compaction_batches(golden)
    plt, tlas, sb = c.dev.plt, c.dev.topAccelStruct, c.dev.shading_buffers()
    seen_mixed_wave = False
    for tag, rows in batches:
        rays, keys = c.mat_rays[rows], c.keys[rows]
        n = rays.shape[0]
        plain = sh.shade_batch(rd, plt, tlas, sb, rays, keys)
        hits = np.flatnonzero(plain["shade"]["hit"] == 1)
        assert plain["live"] == hits.shape[0], tag
        if tag == "all miss":
            assert hits.shape[0] == 0
        if tag == "all hit":
            assert hits.shape[0] == n
        # sentinel-filled outputs, one record longer than needed
        bR, bK = sh.upload(rd, plt, rays), sh.upload(rd, plt, keys)
        bH = rd.QueryRays(tlas, bR, n, rd.QUERY_CLOSEST)
        fill = lambda size: sh.upload(rd, plt, np.full(size, 0xA5, np.uint8))
        bN, bSh, bSrc = fill(32 * n + 32), fill(32 * n + 32), fill(4 * n + 16)
        bS, _, _, _, live, invalid = rd.ShadeHits(tlas, bR, bH, bK, n, sb, next=bN, shadow=bSh, src=bSrc)
        assert (live, invalid) == (hits.shape[0], 0), tag
        shade = sh.read(rd, plt, bS, n, rd.SHADE_DTYPE)
        raw = {k: rd.ReadBuffer(plt, b, b.size).copy() for k, b in (("next", bN), ("shadow", bSh), ("src", bSrc))}
        src = raw["src"][:4 * live].view(U4)
        assert sorted(src.tolist()) == hits.tolist(), tag
        assert np.array_equal(shade["slot"][src], np.arange(live, dtype=np.uint32)), tag
        dead = np.setdiff1d(np.arange(n), hits)
        assert (shade["slot"][dead] == sh.NO_SLOT).all(), tag
        for f in ("color", "hit", "colorOccluded", "materialIndex", "nextFactor"):
            assert same(shade[f], plain["shade"][f]), (tag, f)
        for k in ("next", "shadow"):
            got = raw[k][:32 * live].view(rd.RAY_DTYPE)
            assert same(got, plain[k][src]), (tag, k)
            assert (raw[k][32 * live:] == 0xA5).all(), (tag, k, "records from `live` on were touched")
        assert (raw["src"][4 * live:] == 0xA5).all(), tag
        # the survivors of each aligned group of 64 inputs are contiguous and ascending
        group = src // 64
        for g in np.unique(group):
            at = np.flatnonzero(group == g)
            assert np.array_equal(at, np.arange(at[0], at[0] + at.shape[0])), (tag, int(g))
            assert (np.diff(src[at].astype(np.int64)) > 0).all(), (tag, int(g))
            seen_mixed_wave |= 0 < at.shape[0] < min(64, n - 64 * int(g))
        # without `next`: the next direction is not sampled, everything else is what it was
        bS2, bN2, bSh2, bSrc2, live2, _ = rd.ShadeHits(tlas, bR, bH, bK, n, sb, next=None, compact=True)
        assert bN2 is None and live2 == live
        s2, src2 = sh.read(rd, plt, bS2, n, rd.SHADE_DTYPE), sh.read(rd, plt, bSrc2, live, U4)
        for f in ("color", "hit", "colorOccluded", "materialIndex"):
            assert same(s2[f], shade[f]), (tag, f)
        assert sorted(src2.tolist()) == hits.tolist() and np.array_equal(s2["slot"][src2], np.arange(live, dtype=np.uint32))
        assert (sh.bits(s2["nextFactor"][hits]) == sh.bits(np.float32(1.0))).all() and not sh.bits(s2["nextFactor"][dead]).any(), tag
        assert same(sh.read(rd, plt, bSh2, live, rd.RAY_DTYPE), plain["shadow"][src2]), tag
    assert seen_mixed_wave, "no group of 64 inputs held both survivors and others"


# ---- 4. bounds ----------------------------------------------------------------------------------------------------------------------
SLACK = 4096


def test_records_that_point_outside_a_buffer_are_zeroed_and_counted(mods, golden):
    """Every scene stream lives in an allocation 4 KiB larger than its content (the slack holds plausible values), the library
    gets a view of the content alone; option "textures" is 1 and a two-layer image array is given, so the uv stream and the
    texture indices count.  64 of c1's 2048 records are rewritten so that each breaks one rule by less than the slack -- a kernel
    that did not check would read memory this test owns: the 64 come back as zero records (slot 0xffffffff) and counted, the
    other 1984 bit for bit as before.

    The streams are c1's with: one trap triangle (0, 1, the vertex one past the last mesh) appended to the indices; a Material
    with albedoTexIdx == layers appended, which instance T's MeshInfo points at; instance M's MeshInfo pointing past the Material
    table.  Records that hit M or T are re-pointed at instance 0 first, so that no unpoisoned record breaks a rule."""
    rd, _ = mods
    c = golden("c1")
    plt, b, tlas = c.dev.plt, c.b, c.dev.topAccelStruct
    M, T, LAYERS = 5, 6, 2
    mi, mt = b["meshInfo"].copy(), b["material"]
    ninst, nidx0, nfl, nmat = mi.shape[0], b["index"].shape[0], b["normal"].shape[0], b["material"].shape[0]
    A = int(np.flatnonzero(mi["normalOffset"] == mi["normalOffset"].max())[-1])
    assert A not in (M, T) and b["uv"].shape[0] == nfl
    nvA = (nfl - int(mi[A]["normalOffset"])) // 3
    index = np.concatenate([b["index"], np.array([0, 1, nvA], np.uint32)])
    bad_mat = mt[:1].copy()
    bad_mat["albedoTexIdx"] = LAYERS
    materials = np.concatenate([mt, bad_mat])
    mi[T]["materialIndex"] = nmat
    mi[M]["materialIndex"] = nmat + 1 + 20                     # 21 records past the table: 1008 bytes into the slack
    nidx = index.shape[0]
    trap = lambda inst, k: (nidx0 - int(mi[inst]["indexOffset"])) // 3 + k

    def view(content, slack_fill):
        content = np.ascontiguousarray(content)
        whole = np.concatenate([content.view(np.uint8).reshape(-1), np.resize(np.ascontiguousarray(slack_fill).view(np.uint8).reshape(-1), SLACK)])
        buf = sh.upload(rd, plt, whole)
        assert buf.size == content.nbytes + SLACK
        return rd.WrapDeviceMemory(plt, buf.device_ptr, content.nbytes, keepalive=buf)
    img = rd.CreateImageArray(plt, 4, 4, LAYERS)
    for l in range(LAYERS):
        rd.WriteImage(plt, img, 4, 4, l, np.full((4, 4, 4), 60 + 100 * l, np.uint8))
    sb = rd.ShadingBuffers(c.dev.rdSceneData, view(mi, mi[:1]), view(index, np.arange(3, dtype=np.uint32)), view(b["uv"], np.float32([0.25, 0.75, 0.0])),
                           view(b["normal"], np.float32([0.6, 0.0, 0.8])), view(materials, mt[:1]), img,
                           rd.CreateSampler(plt, rd.RD_ADDRESS_REPEAT, rd.RD_FILTER_NEAREST))
    rd.SetOption("textures", 1)
    try:
        q = sh.shade_batch(rd, plt, tlas, sb, c.mat_rays, c.keys)["q"]
        assert (q["hit"] == 1).all()
        ok = q.copy()
        moved = np.isin(ok["instanceIndex"], (M, T))
        ok["instanceIndex"][moved], ok["primitiveIndex"][moved] = 0, 0
        base = sh.shade_batch(rd, plt, tlas, sb, c.mat_rays, c.keys, hits=ok)
        assert base["invalid"] == 0 and base["live"] == 2048 and (base["shade"]["hit"] == 1).all()
        # (none of c1's materials has a texture: with valid records the views and the image change nothing)
        own = sh.shade_batch(rd, plt, tlas, c.dev.shading_buffers(), c.mat_rays, c.keys, hits=ok)
        assert same(own["shade"], base["shade"]) and same(own["next"], base["next"])

        rng = np.random.default_rng(9)
        rows = np.sort(rng.choice(q.shape[0], 64, replace=False))
        bad, kinds = ok.copy(), []
        for j, r in enumerate(rows):
            inst, k = int(bad["instanceIndex"][r]), j % 8
            if k == 0:      # instanceIndex: the first past the instance count (= the MeshInfo count), and further
                bad["instanceIndex"][r] = ninst + j // 8
            elif k == 1:    # ... and further ones whose MeshInfo would still be read from the slack (4096 / 32 = 128 records)
                bad["instanceIndex"][r] = ninst + 8 + 15 * (j // 8)
            elif k == 2:    # triangles past the index stream, by less than the slack
                bad["primitiveIndex"][r] = trap(inst, 1 + 37 * (j // 8))
            elif k == 3:    # 3 * primitiveIndex wraps in 32 bits to the triangle before the mesh / into the stream
                bad["primitiveIndex"][r] = (0xffffffff, 0x55555556, 0x7fffffff, 0xaaaaaaab)[(j // 8) % 4]
            elif k == 4:    # the trap triangle: a vertex whose normal and uv lie one vertex past their streams
                bad["instanceIndex"][r], bad["primitiveIndex"][r] = A, trap(A, 0)
            elif k == 5:    # materialIndex past the Material table
                bad["instanceIndex"][r], bad["primitiveIndex"][r] = M, (j // 8) % 2
            elif k == 6:    # a texture layer past the image array
                bad["instanceIndex"][r], bad["primitiveIndex"][r] = T, (j // 8) % 2
            else:           # a triangle far into the slack, its three indices still inside it
                bad["primitiveIndex"][r] = trap(inst, 300)
            kinds.append(k)
        assert 3 * 300 + 2 < SLACK // 4 and 8 + 15 * 7 < SLACK // 32 and (21 + 1) * 48 < SLACK
        poisoned = np.zeros(q.shape[0], bool)
        poisoned[rows] = True
        # first through the host seam -- the same function the kernel compiles: every poisoned record invalid, every other valid
        for r in range(q.shape[0]):
            inst, prim = int(bad["instanceIndex"][r]), int(bad["primitiveIndex"][r])
            first = int(mi[inst]["indexOffset"]) + 3 * prim if inst < ninst else -1
            idx3 = index[first:first + 3] if 0 <= first and first + 3 <= nidx else None
            got = rd.DebugShadeInBounds(mi, ninst, inst, prim, idx3, nidx, nfl, nfl, materials, textures=True, layers=LAYERS)
            assert got is (not poisoned[r]), (r, inst, prim)
        # M and T are invalid by their material alone: with the table they point into, and without textures, they shade
        assert rd.DebugShadeInBounds(mi, ninst, T, 0, index[int(mi[T]["indexOffset"]):][:3], nidx, nfl, nfl, materials, textures=False, layers=LAYERS)
        got = sh.shade_batch(rd, plt, tlas, sb, c.mat_rays, c.keys, hits=bad)
        z = got["shade"][poisoned]
        nz = z.view(np.uint32).reshape(64, 12)[:, :11].any(1) | (z["slot"] != sh.NO_SLOT)
        assert not nz.any(), "poisoned records came back non-zero: kinds %s" % sorted({kinds[i] for i in np.flatnonzero(nz)})
        assert got["invalid"] == 64 and got["live"] == 1984
        assert not got["next"][poisoned].view(np.uint8).any() and not got["shadow"][poisoned].view(np.uint8).any()
        for k in ("shade", "next", "shadow"):
            assert same(got[k][~poisoned], base[k][~poisoned]), k
        # compacting: the invalid records do not survive
        comp = sh.shade_batch(rd, plt, tlas, sb, c.mat_rays, c.keys, hits=bad, compact=True)
        assert comp["invalid"] == 64 and comp["live"] == 1984 and sorted(comp["src"].tolist()) == np.flatnonzero(~poisoned).tolist()
    finally:
        rd.SetOption("textures", 0)


# ---- 5. offsets and refusals ----------------------------------------------------------------------------------------------------------
def test_offsets_and_refusals(mods, golden, shaded):
    """n = 200 of c1's records at distinct offsets in buffers filled with 0xA5: the records equal the plain call's and no byte
    outside the output ranges is touched; then every refusal, after each of which the outputs are unchanged"""
    rd, _ = mods
    c, plain = golden("c1"), shaded("c1")
    dev, plt, tl = c.dev, c.dev.plt, c.dev.topAccelStruct
    sb = dev.shading_buffers()
    n, tail = 200, 128
    off = dict(rays=96, hits=160, keys=48, shade=192, next=64, shadow=32, src=16)
    rec_size = dict(rays=32, hits=32, keys=16, shade=48, next=32, shadow=32, src=4)
    B = {k: rd.CreateBuffer(plt, off[k] + rec_size[k] * n + tail) for k in off}
    fill = lambda buf: rd.WriteBuffer(plt, buf, buf.size, np.full(buf.size, 0xA5, np.uint8))
    for buf in B.values():
        fill(buf)
    rd.WriteBuffer(plt, B["rays"], 32 * n, c.mat_rays[:n], offset=off["rays"])
    rd.WriteBuffer(plt, B["hits"], 32 * n, plain["q"][:n], offset=off["hits"])
    rd.WriteBuffer(plt, B["keys"], 16 * n, c.keys[:n], offset=off["keys"])
    outs = ("shade", "next", "shadow", "src")
    snapshot = lambda: {k: rd.ReadBuffer(plt, B[k], B[k].size).copy() for k in B}

    def run(**kw):
        a = dict(tlas=tl, rays=B["rays"], hits=B["hits"], keys=B["keys"], n=n, scene_buffers=sb, shade=B["shade"], next=B["next"], shadow=B["shadow"],
                 src=None, rays_offset=off["rays"], hits_offset=off["hits"], keys_offset=off["keys"], shade_offset=off["shade"],
                 next_offset=off["next"], shadow_offset=off["shadow"], src_offset=off["src"])
        a.update(kw)
        return rd.ShadeHits(a.pop("tlas"), a.pop("rays"), a.pop("hits"), a.pop("keys"), a.pop("n"), a.pop("scene_buffers"), **a)

    before = snapshot()
    ret = run()
    assert ret[0] is B["shade"] and ret[1] is B["next"] and ret[2] is B["shadow"] and ret[3] is None and ret[4:] == (n, 0)
    after = snapshot()
    for k in ("rays", "hits", "keys", "src"):
        assert np.array_equal(after[k], before[k]), k
    for k in ("shade", "next", "shadow"):
        lo, hi = off[k], off[k] + rec_size[k] * n
        assert same(after[k][lo:hi], plain[k][:n]), k
        assert (after[k][:lo] == 0xA5).all() and (after[k][hi:] == 0xA5).all(), k
    good = snapshot()
    # n == 0 touches nothing
    for k in outs:
        fill(B[k])
    assert run(n=0, src=B["src"])[4:] == (0, 0) and all((rd.ReadBuffer(plt, B[k], B[k].size) == 0xA5).all() for k in outs)

    one = rd.CreateBuffer(plt, 32 * n * 6)          # rays | hits | room for outputs, for the overlap cases
    rd.WriteBuffer(plt, one, 32 * n, c.mat_rays[:n])
    rd.WriteBuffer(plt, one, 32 * n, plain["q"][:n], offset=32 * n)
    null = rd.Buffer(None, 1 << 20)
    S = lambda **kw: rd.ShadingBuffers(**{**dict(scene=dev.rdSceneData, meshInfo=dev.meshInfoData, index=dev.indexData, uv=dev.uvData, normal=dev.normalData,
                                                material=dev.materialData), **kw})
    in_one = dict(rays=one, hits=one, rays_offset=0, hits_offset=32 * n)
    cases = [
        ("rays_offset 8", dict(rays_offset=8), "16"), ("hits_offset 8", dict(hits_offset=8), "16"), ("keys_offset 8", dict(keys_offset=8), "16"),
        ("shade_offset 8", dict(shade_offset=8), "16"), ("next_offset 24", dict(next_offset=24), "16"), ("shadow_offset 4", dict(shadow_offset=4), "16"),
        ("src_offset 4", dict(src=B["src"], src_offset=4), "16"),
        ("rays past the end", dict(rays_offset=off["rays"] + tail + 16), "ray buffer"),
        ("records past the end", dict(hits_offset=off["hits"] + tail + 16), "hit buffer"),
        ("keys past the end", dict(keys_offset=off["keys"] + tail + 16), "key buffer"),
        ("shade past the end", dict(shade_offset=off["shade"] + tail + 16), "shade buffer"),
        ("next past the end", dict(next_offset=off["next"] + tail + 16), "next-ray buffer"),
        ("shadow past the end", dict(shadow_offset=off["shadow"] + tail + 16), "shadow-ray buffer"),
        ("src past the end", dict(src=B["src"], src_offset=off["src"] + tail + 16), "src buffer"),
        ("src holds live records, not n", dict(src=rd.CreateBuffer(plt, 4 * n - 16), src_offset=0), "src buffer"),
        ("next one record short", dict(next=rd.CreateBuffer(plt, 32 * n - 16), next_offset=0), "next-ray buffer"),
        ("shade over the rays", dict(in_one, shade=one, shade_offset=32 * n - 48), "overlap"),
        ("shade over the records", dict(in_one, shade=one, shade_offset=64 * n - 48), "overlap"),
        ("next = the records", dict(in_one, next=one, next_offset=32 * n), "overlap"),
        ("shadow over the keys", dict(keys=one, keys_offset=64 * n, shadow=one, shadow_offset=64 * n + 16 * n - 32), "overlap"),
        ("src over the first ray's tail", dict(in_one, n=1, src=one, src_offset=16), "overlap"),
        ("next over shade", dict(shade=one, shade_offset=64 * n, next=one, next_offset=64 * n + 48 * n - 32), "overlap"),
        ("shadow = next", dict(next=one, next_offset=64 * n, shadow=one, shadow_offset=64 * n), "overlap"),
        ("src over shadow", dict(shadow=one, shadow_offset=64 * n, src=one, src_offset=64 * n + 32 * n - 16), "overlap"),
        ("null tlas", dict(tlas=null), "TLAS"), ("null rays", dict(rays=null), "ray buffer handle"), ("null hits", dict(hits=null), "hit buffer handle"),
        ("null keys", dict(keys=null), "key buffer handle"), ("null shade", dict(shade=null), "shade buffer handle"),
        ("unknown next", dict(next=rd.Buffer(12345678, 1 << 20)), "next-ray buffer handle"),
        ("unknown shadow", dict(shadow=rd.Buffer(12345678, 1 << 20)), "shadow-ray buffer handle"),
        ("unknown src", dict(src=rd.Buffer(12345678, 1 << 20)), "src buffer handle"),
        ("null scene", dict(scene_buffers=S(scene=null)), "SceneProperties"), ("null meshInfo", dict(scene_buffers=S(meshInfo=null)), "meshInfo"),
        ("null index", dict(scene_buffers=S(index=null)), "index"), ("null normal", dict(scene_buffers=S(normal=null)), "normal"),
        ("null material", dict(scene_buffers=S(material=null)), "material"),
        ("unknown uv", dict(scene_buffers=S(uv=rd.Buffer(12345678, 64))), "uv"),
        ("unknown textureArray", dict(scene_buffers=S(textureArray=rd.Buffer(12345678, 64))), "textureArray"),
        ("a scene buffer smaller than SceneProperties", dict(scene_buffers=S(scene=rd.CreateBuffer(plt, 160))), "SceneProperties"),
        ("misaligned wrapped rays", dict(rays=rd.WrapDeviceMemory(plt, B["rays"].device_ptr + 8, 32 * n + 64, keepalive=B["rays"]), rays_offset=16), "aligned"),
        ("misaligned wrapped shade", dict(shade=rd.WrapDeviceMemory(plt, B["shade"].device_ptr + 4, 48 * n + 64, keepalive=B["shade"]), shade_offset=0), "aligned"),
        ("misaligned wrapped index stream", dict(scene_buffers=S(index=rd.WrapDeviceMemory(plt, dev.indexData.device_ptr + 2, dev.indexData.size - 2, keepalive=dev.indexData))), "aligned"),
    ]
    run()
    good = snapshot()
    for what, kw, word in cases:
        with pytest.raises(rd.RadianceError) as e:
            run(**kw)
        assert word in str(e.value) and "rdx_shade_hits" in str(e.value), (what, str(e.value))
        now = snapshot()
        for k in B:
            assert np.array_equal(now[k], good[k]), (what, k)
    from radiance_ray_tracing_amd import _lib
    L = _lib.lib()
    assert L.rdx_shade_hits(tl.handle, B["rays"].handle, 0, B["hits"].handle, 0, B["keys"].handle, 0, n, None, B["shade"].handle, 0, None, 0, None, 0, None, 0, None, None) != 0
    assert "scene" in _lib.last_error()
    unknown_sampler = _lib.rdx_shading_buffers(dev.rdSceneData.handle, dev.meshInfoData.handle, dev.indexData.handle, None, dev.normalData.handle,
                                              dev.materialData.handle, None, 12345678)
    import ctypes as C
    assert L.rdx_shade_hits(tl.handle, B["rays"].handle, 0, B["hits"].handle, 0, B["keys"].handle, 0, n, C.byref(unknown_sampler), B["shade"].handle, 0,
                            None, 0, None, 0, None, 0, None, None) != 0
    assert "sampler" in _lib.last_error()
    assert all(np.array_equal(v, good[k]) for k, v in snapshot().items())
    # adjacent ranges of one buffer are fine: rays, records, then shade | next | shadow; the call still works after the refusals
    ret = run(**in_one, shade=one, shade_offset=64 * n, next=one, next_offset=112 * n, shadow=one, shadow_offset=144 * n)
    assert ret[4:] == (n, 0)
    assert same(rd.ReadBuffer(plt, one, 48 * n, offset=64 * n), plain["shade"][:n]) and same(rd.ReadBuffer(plt, one, 32 * n, offset=112 * n), plain["next"][:n])
    for what, fn in (("a list", lambda: run(scene_buffers=[dev.meshInfoData])), ("not a Buffer", lambda: run(scene_buffers=(1, 2, 3, 4, 5, 6))),
                     ("shade not a Buffer", lambda: run(shade=7)), ("sampler not a Sampler", lambda: run(scene_buffers=S(sampler=dev.uvData)))):
        with pytest.raises(rd.RadianceError):
            fn()


# ---- 6. after UpdateAccelStruct -----------------------------------------------------------------------------------------------------
def _decorated(scenes, name):
    """accel_layout_cases.scene(name) with a camera, a light and one material per custom id (as tests/test_gpu_tlas_update.py)"""
    s = alc.scene(name)
    nmat = 1 + max(mat for _, _, mat in s.instances)
    s.materials = [scenes.material((0.25 + 0.07 * (k % 9), 0.8 - 0.06 * (k % 7), 0.3 + 0.05 * (k % 5)), 0.1 * (k % 3), 0.4 + 0.05 * (k % 4)) for k in range(nmat)]
    s.camera = scenes.blender_camera(64, 36, 0.05, 0.036, 12.0, 0.0, (1.0, 12.0, 2.5), (-100.0, 180.0, 0.0))
    s.sceneProps = scenes.blender_dir_light(-45.0, 20.0, 5.0)
    s.rtprop = scenes._rtprop(0, 2, 3)
    return s


def test_after_update_accel_struct(mods):
    """the 9-instance grid sharing two BLAS: the last instance is carried far away, then the first nudged.  Each time the shade
    records, next rays and shadow rays are bitwise what a freshly built TLAS gives, and differ from those before the move"""
    rd, scenes = mods
    s = _decorated(scenes, "shared_blas")
    dev = scenes.DeviceScene(s)
    o, d = rec.own_primary_rays(s, 4096)
    rays = sh.rays_of(rd, o, d)
    n = rays.shape[0]
    keys = sh.keys_of(np.arange(n) % 7, np.arange(n), np.arange(n) % 5)
    prev = sh.shade_batch(rd, dev.plt, dev.topAccelStruct, dev.shading_buffers(), rays, keys, compact=False)
    assert prev["invalid"] == 0 and 100 <= prev["live"] < n
    insts = tu.instances(s)
    for move in ("B", "A"):
        insts = tu.apply(insts, move)
        rd.UpdateAccelStruct(dev.plt, dev.topAccelStruct, tu.rd_instances(rd, insts, dev.blas))
        got = sh.shade_batch(rd, dev.plt, dev.topAccelStruct, dev.shading_buffers(), rays, keys)
        t = scenes.Scene(s.name)
        t.meshes, t.materials, t.camera, t.sceneProps, t.rtprop = s.meshes, s.materials, s.camera, s.sceneProps, s.rtprop
        for mi, tf, sbt, mat in insts:
            t.add_instance(mi, tf, mat, sbt)
        fresh = scenes.DeviceScene(t)
        want = sh.shade_batch(rd, fresh.plt, fresh.topAccelStruct, fresh.shading_buffers(), rays, keys)
        assert got["invalid"] == 0 and want["invalid"] == 0 and got["live"] == want["live"]
        for k in ("q", "shade", "next", "shadow", "occluded"):
            assert same(got[k], want[k]), (move, k)
        assert not same(got["shade"], prev["shade"]), move
        prev = got


# ---- 7. a scene of instances against the live reference --------------------------------------------------------------------------
def test_instanced_scene_against_the_live_reference(mods):
    """five instances of one icosphere BLAS and a heightfield, rotated, scaled non-uniformly and translated: 4096 rays against the
    reference's own device code run here (RefScene.trace -> HitData, RefScene.material_batch -> payloads), bit for bit"""
    rd, scenes = mods
    if not rg.available("p"):
        pytest.skip("oracle/_ref/ref_shader_gfx950_p.co is not built (needs the reference's sources: `make -C oracle`)")
    s = sc.instanced_scene(scenes)
    dev = scenes.DeviceScene(s)
    o, d = sc.instanced_rays()
    blob = rd.ReadBuffer(dev.plt, dev.topAccelStruct, dev.topAccelStruct.size).tobytes()
    rs = rg.RefScene(rg.RefGpu("p"), s, blob)
    h = rs.trace(o, d)
    n = o.shape[0]
    frames, depths = gc.material_inputs(n)
    pay = rs.material_batch(h, d, frames, depths)
    r = sh.shade_batch(rd, dev.plt, dev.topAccelStruct, dev.shading_buffers(), sh.rays_of(rd, o, d), sh.keys_of(frames, np.arange(n), depths))
    assert r["invalid"] == 0
    hit = h["hit"] == 1
    assert (np.bincount(h["instanceIndex"][hit], minlength=6) >= 50).all()
    lit, occ = sh.check_against_payloads(r, h, pay, "instanced")
    print("instanced: %d hits, lit %d, occluded %d" % (int(hit.sum()), lit, occ))
    assert lit >= 100 and occ >= 100 and lit + occ <= int(hit.sum())


# ---- 8. textures, another shader binding table, torch ----------------------------------------------------------------------------------
def _textured_scene(scenes, w, h):
    """two textured quads + a textured box (the scene of tests/test_gpu_parity.py::test_image_array_and_texture_path)"""
    s = scenes.Scene("textured")
    floor = s.add_mesh(scenes.quad([-3, 0, -3], [3, 0, -3], [3, 0, 3], [-3, 0, 3], [0, 1, 0]))
    wall = s.add_mesh(scenes.quad([-3, 0, 3], [3, 0, 3], [3, 4, 3], [-3, 4, 3], [0, 0, -1]))
    cube = s.add_mesh(scenes.box([-0.8, 0.0, -0.8], [0.8, 1.6, 0.8]))
    m0 = scenes.material((0.7, 0.7, 0.7), 0.0, 0.6); m0["albedoTexIdx"] = 0
    m1 = scenes.material((0.7, 0.7, 0.7), 0.0, 0.6); m1["albedoTexIdx"] = 1; m1["roughnessTexIdx"] = 2; m1["metallicTexIdx"] = 2
    m2 = scenes.material((0.9, 0.8, 0.5), 0.2, 0.4); m2["albedoTexIdx"] = 0; m2["normalTexIdx"] = 1
    s.materials = [m0, m1, m2]
    s.add_instance(floor, None, 0); s.add_instance(wall, None, 1); s.add_instance(cube, scenes.translate(0.3, 0.0, 0.2) @ scenes.rotate_y(25.0), 2)
    s.camera = scenes.blender_camera(w, h, 0.05, 0.036, 8.0, 0.0, (0.5, 9.0, 2.5), (-100.0, 180.0, 0.0))
    s.sceneProps = scenes.blender_dir_light(-45.0, 20.0, 6.0)
    s.rtprop = scenes._rtprop(0, 2, 3)
    return s


def _test_textures(size=64):
    yy, xx = np.mgrid[0:size, 0:size]
    t = np.zeros((3, size, size, 4), np.uint8)
    t[0, ..., 0] = np.where(((xx // 8) + (yy // 8)) % 2, 230, 40); t[0, ..., 1] = 120; t[0, ..., 2] = (xx * 4) % 256; t[0, ..., 3] = 255
    t[1, ..., 0] = (xx * 3 + yy) % 256; t[1, ..., 1] = (yy * 5) % 256; t[1, ..., 2] = 200; t[1, ..., 3] = 255
    t[2, ..., 0] = 17; t[2, ..., 1] = 60 + (xx % 16) * 8; t[2, ..., 2] = np.where(yy % 32 < 16, 0, 255); t[2, ..., 3] = 255
    return t


def _check_against_seam(rd, r, seam, tag):
    """the lit colour, nextFactor and the next ray of every hit equal rd.MaterialBatch on the same hits, bit for bit"""
    s, k = r["shade"], seam["hit"] == 1
    assert np.array_equal(s["hit"] == 1, k), tag
    slot = s["slot"][k]
    for name, got, want in (("color", s["color"][k], seam["color"][k]), ("nextFactor", s["nextFactor"][k], seam["nextFactor"][k]),
                            ("nextRayOrigin", r["next"]["origin"][slot], seam["nextRayOrigin"][k]),
                            ("nextRayDirection", r["next"]["direction"][slot], seam["nextRayDirection"][k])):
        eq = (sh.bits(got) == sh.bits(want)).all(1)
        assert eq.all(), "%s: %s differs on %d of %d hits" % (tag, name, int((~eq).sum()), eq.shape[0])


def test_textures_equal_the_material_seam(mods):
    """option "textures": 0 -> texel 0 whatever is given; 1 -> the image array is read through the sampler, for a linear / repeat
    and a nearest / clamp sampler: bit-equal to rd.MaterialBatch, which reads the bound descriptors"""
    rd, scenes = mods
    W, H = 96, 54
    s = _textured_scene(scenes, W, H)
    dev = scenes.DeviceScene(s)
    plt = dev.plt
    tex = _test_textures()
    img = rd.CreateImageArray(plt, 64, 64, 3)
    for l in range(3):
        rd.WriteImage(plt, img, 64, 64, l, tex[l])
    px = np.arange(W * H, dtype=np.uint32)[::2]
    o, d = rd.GenerateBatch(px, np.stack([np.zeros_like(px), np.zeros_like(px), px], 1))
    hits = rd.TraceBatch(dev.topAccelStruct, o, d)
    hit = hits["hit"] == 1
    assert set(np.unique(hits["instanceCustomIndex"][hit])) == {0, 1, 2}
    frames, depths = (px % 5).astype(np.uint32), (px % 3).astype(np.int32)
    rays, keys = sh.rays_of(rd, o, d), sh.keys_of(frames, px, depths)
    outs = []
    try:
        for textures, addr, filt in ((0, rd.RD_ADDRESS_REPEAT, rd.RD_FILTER_LINEAR), (1, rd.RD_ADDRESS_REPEAT, rd.RD_FILTER_LINEAR),
                                     (1, rd.RD_ADDRESS_CLAMP, rd.RD_FILTER_NEAREST), (1, None, None)):
            rd.SetOption("textures", textures)
            sampler = rd.CreateSampler(plt, addr, filt) if addr is not None else None
            ds = list(dev.descSet); ds[11] = img; ds[12] = sampler
            rd.BindDescriptorSet(plt, ds)
            seam = rd.MaterialBatch(hits[hit], d[hit], px[hit], frames[hit], depths[hit])
            r = sh.shade_batch(rd, plt, dev.topAccelStruct, dev.shading_buffers(img, sampler), rays, keys)
            assert r["invalid"] == 0
            full = np.zeros(hits.shape[0], rd.PAYLOAD_DTYPE)
            full[hit] = seam
            _check_against_seam(rd, r, full, "textures %d sampler %s/%s" % (textures, addr, filt))
            outs.append(r["shade"].copy())
        # textures on without an image array: texel 0, as with textures off
        r = sh.shade_batch(rd, plt, dev.topAccelStruct, dev.shading_buffers(), rays, keys)
        assert same(r["shade"], outs[0])
        assert not same(outs[0], outs[1]) and not same(outs[1], outs[2])          # the textures are really read
        with pytest.raises(rd.RadianceError, match="uv"):
            rd.ShadeHits(dev.topAccelStruct, sh.upload(rd, plt, rays), sh.upload(rd, plt, r["q"]), sh.upload(rd, plt, keys), rays.shape[0],
                         rd.ShadingBuffers(dev.rdSceneData, dev.meshInfoData, dev.indexData, None, dev.normalData, dev.materialData, img))
    finally:
        rd.SetOption("textures", 0)
        dev.bind()


def test_stock_table_with_instance_sbt_offsets(mods):
    """the scene of test_instance_sbt_offsets (a): two instances with SBTOffset 1 dispatch row 2, closest-hit `shadow` -- the
    payload is hit, black, and keeps what it held on entry: factor 1, the next ray = the ray itself, no shadow query (a shadow
    record with tmax 0); every other hit equals rd.MaterialBatch"""
    rd, scenes = mods
    s = scenes.c1_cornell(96, 54, spp=2, depth=4, sphere_subdiv=3)
    s.sbt_offsets = {5: 1, 7: 1}
    dev = scenes.DeviceScene(s)
    px = np.arange(96 * 54, dtype=np.uint32)[::2]
    o, d = rd.GenerateBatch(px, np.stack([np.zeros_like(px), np.zeros_like(px), px], 1))
    hits = rd.TraceBatch(dev.topAccelStruct, o, d, reference_order=True)
    frames, depths = (px % 5).astype(np.uint32), (px % 3).astype(np.int32)
    rays = sh.rays_of(rd, o, d)
    r = sh.shade_batch(rd, dev.plt, dev.topAccelStruct, dev.shading_buffers(), rays, sh.keys_of(frames, px, depths))
    assert r["invalid"] == 0 and np.array_equal(r["q"]["hit"], hits["hit"]) and np.array_equal(r["q"]["instanceSBTOffset"], hits["instanceSBTOffset"])
    row2 = (hits["hit"] == 1) & (hits["instanceSBTOffset"] == 1)
    row1 = (hits["hit"] == 1) & ~row2
    assert int(row2.sum()) > 100 and int(row1.sum()) > 1000
    seam = np.zeros(hits.shape[0], rd.PAYLOAD_DTYPE)
    seam[row1] = rd.MaterialBatch(hits[row1], d[row1], px[row1], frames[row1], depths[row1])
    sub = dict(shade=r["shade"][~row2], next=r["next"])
    _check_against_seam(rd, sub, seam[~row2], "rows 1")
    z, slot = r["shade"][row2], r["shade"]["slot"][row2]
    assert (z["hit"] == 1).all() and not sh.bits(z["color"]).any() and not sh.bits(z["colorOccluded"]).any()
    assert (sh.bits(z["nextFactor"]) == sh.bits(np.float32(1.0))).all()
    assert same(r["next"]["origin"][slot], rays["origin"][row2]) and same(r["next"]["direction"][slot], rays["direction"][row2])
    assert not r["shadow"][slot].view(np.uint8).any() and not r["occluded"][row2].any()


_SBT2_CHILD = r"""
import os, sys
ROOT = sys.argv[1]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import rrt_amd
from radiance_ray_tracing_amd import rd, scenes
import shade_cases as sh
out = []
for offsets in ({}, {0: 4, 3: 4, 5: 4, 7: 4}):
    s = scenes.c1_cornell(96, 54, spp=2, depth=4, sphere_subdiv=3)
    s.sbt_offsets = dict(offsets)
    dev = scenes.DeviceScene(s)
    px = np.arange(96 * 54, dtype=np.uint32)[::2]
    o, d = rd.GenerateBatch(px, np.stack([np.zeros_like(px), np.zeros_like(px), px], 1))
    hits = rd.TraceBatch(dev.topAccelStruct, o, d, reference_order=True)
    frames, depths = (px % 5).astype(np.uint32), (px % 3).astype(np.int32)
    r = sh.shade_batch(rd, dev.plt, dev.topAccelStruct, dev.shading_buffers(), sh.rays_of(rd, o, d), sh.keys_of(frames, px, depths))
    k = hits["hit"] == 1
    assert r["invalid"] == 0 and np.array_equal(r["shade"]["hit"] == 1, k)
    if offsets:
        assert int((r["q"]["instanceSBTOffset"][k] == 4).sum()) > 500
    seam = rd.MaterialBatch(hits[k], d[k], px[k], frames[k], depths[k])
    slot = r["shade"]["slot"][k]
    for got, want in ((r["shade"]["color"][k], seam["color"]), (r["shade"]["nextFactor"][k], seam["nextFactor"]),
                      (r["next"]["origin"][slot], seam["nextRayOrigin"]), (r["next"]["direction"][slot], seam["nextRayDirection"])):
        assert np.array_equal(sh.bits(got), sh.bits(want))
    out.append((r["shade"].copy(), r["next"].copy(), r["occluded"].copy()))
for a, b in zip(*out):
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
print("SBT2-SHADE-OK")
"""


def test_two_table_library_dispatches_through_the_offset_rows(gpu):
    """a library built for tests/golden/sbt_two_tables.json (RDX_SBT_HEADER): instances with SBTOffset 4 reach `material` through
    row 5 -- ShadeHits equals rd.MaterialBatch there, and equals itself on the same scene with every offset 0"""
    lib = os.path.join(ROOT, "radiance-ray-tracing_amd", "librdx_sbt2.so")
    assert os.path.exists(lib), "librdx_sbt2.so is not built (__graft_entry__.build() builds it)"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _SBT2_CHILD, ROOT]
    out = subprocess.run(cmd, env=dict(os.environ, RDX_LIB=lib), capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "SBT2-SHADE-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


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
import shade_cases as sh
c = sh.Golden(rd, scenes, "c0")
dev, n = c.dev, c.mat_rays.shape[0]
sb = dev.shading_buffers()
want = sh.shade_batch(rd, dev.plt, dev.topAccelStruct, sb, c.mat_rays, c.keys)
hits = np.flatnonzero(want["shade"]["hit"] == 1)
assert 0 < hits.shape[0] < n
# the tensor route, on tensors a torch op produced
t = (torch.from_numpy(c.mat_rays.view(np.float32).reshape(n, 8).copy()).cuda() * torch.ones(8, device="cuda")).contiguous()
k = torch.from_numpy(c.keys.view(np.int32).reshape(n, 4).copy()).cuda()
h = rd.QueryRaysTorch(dev.topAccelStruct, t, 1)
shade, nxt, shadow, src, live, invalid = rd.ShadeHitsTorch(dev.topAccelStruct, t, h, k, sb)
assert (live, invalid) == (hits.shape[0], 0)
assert shade.dtype == torch.float32 and tuple(shade.shape) == (n, 12) and tuple(nxt.shape) == (live, 8) and tuple(shadow.shape) == (live, 8)
assert src.dtype == torch.int32 and tuple(src.shape) == (live,)
s = shade.cpu().numpy().view(rd.SHADE_DTYPE).reshape(-1)
srcn = src.cpu().numpy().astype(np.int64)
assert sorted(srcn.tolist()) == hits.tolist() and np.array_equal(s["slot"][srcn], np.arange(live, dtype=np.uint32))
for f in ("color", "hit", "colorOccluded", "materialIndex", "nextFactor"):
    assert np.array_equal(np.ascontiguousarray(s[f]).view(np.uint32), np.ascontiguousarray(want["shade"][f]).view(np.uint32)), f
assert np.array_equal(nxt.cpu().numpy().view(np.uint32), want["next"][srcn].view(np.uint32).reshape(live, 8))
assert np.array_equal(shadow.cpu().numpy().view(np.uint32), want["shadow"][srcn].view(np.uint32).reshape(live, 8))
# the twenty-line loop of the README: the next bounce straight from the compacted tensors
h2 = rd.QueryRaysTorch(dev.topAccelStruct, nxt, 1)
occ = rd.QueryRaysTorch(dev.topAccelStruct, shadow, 2)[:, 3] == 1
assert np.array_equal(occ.cpu().numpy(), want["occluded"][srcn])
assert tuple(h2.shape) == (live, 8)
# not compacting, no next ray
shade2, nxt2, shadow2, src2, live2, _ = rd.ShadeHitsTorch(dev.topAccelStruct, t, h.view(torch.float32), k, sb, compact=False, sample_next=False)
assert nxt2 is None and src2 is None and live2 == live and tuple(shadow2.shape) == (n, 8)
assert np.array_equal(shadow2.cpu().numpy().view(np.uint32), want["shadow"].view(np.uint32).reshape(n, 8))
e = rd.ShadeHitsTorch(dev.topAccelStruct, t[:0], h[:0], k[:0], sb)
assert tuple(e[0].shape) == (0, 12) and tuple(e[1].shape) == (0, 8) and e[4:] == (0, 0)
bad = [(t[:, :7], h, k), (t.double(), h, k), (t.cpu(), h, k), (t, h[:, :7], k), (t, h.long(), k), (t, h.cpu(), k), (t, h[:-1], k),
       (t, h, k[:, :3]), (t, h, k.float()), (t, h, k.cpu()), (t, h, k[:-1]), (c.mat_rays, h, k)]
for j, (r_, h_, k_) in enumerate(bad):
    try:
        rd.ShadeHitsTorch(dev.topAccelStruct, r_, h_, k_, sb)
    except rd.RadianceError:
        continue
    raise AssertionError("bad argument set %d was accepted" % j)
print("TORCH-SHADE-OK", n, live)
"""


def test_torch_tensors_in_a_fresh_process(gpu):
    """rd.ShadeHitsTorch equals the buffer route bit for bit; wrong dtype, shape or device is refused in Python.  torch is
    initialised first, in a process of its own (as tests/test_gpu_ray_query.py does)"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _TORCH_CHILD, ROOT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "TORCH-SHADE-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])

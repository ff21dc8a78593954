"""GPU suite (-m gpu): rd.TracePaths and its torch route (rdx_trace_paths) -- radiance along the caller's own rays on the frame
path's stages.

Comparands, in this order of authority:
  1. the reference's own device code, recorded (tests/golden/refgpu_c{0,1,2}.npz): its two progressive frames scratch0 / image0,
     scratch1 / image1, which GenerateRays -> TracePaths -> Accumulate must write;
  2. the loop over the public calls rd.QueryRays / rd.ShadeHits (paths_cases.public_loop), which tests/test_gpu_raygen.py holds to
     those recordings and tests/test_paths_cpu.py checks by hand, for rays no camera makes;
  3. the library's own frame path, TraceRays, which the existing suite holds to the recordings.
Every bar is equality of bits.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_cases as gc
import paths_cases as pc
import raygen_cases as rc
import shade_cases as sh
import tlas_update_cases as tu
from test_gpu_shade import _decorated, _test_textures, _textured_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U4 = np.float32, np.dtype("<u4")
S = rc.SENTINEL
DEPTH = 4
SEED = {"c1": 20261019, "c2": 20261020}        # chosen so that the loop over the public calls keeps >= 25 % of the rays for two bounces
# the options rdx_trace_paths reads, as rdx_init leaves them (rdx_runtime.cpp Context::Options)
DEFAULTS = dict(kernel=3, sort=-1, fuse=-1, quad=1, cull=-1, group_entry_items=1, chunk_paths=16 << 20)


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


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def scene_box(rd, dev):
    blob = rd.ReadBuffer(dev.plt, dev.topAccelStruct, dev.topAccelStruct.size).tobytes()
    s = rd.DebugAccelLayout(blob)[0]
    return np.array(s["sceneLo"], np.float64), np.array(s["sceneHi"], np.float64)


def batch_for(rd, dev, seed):
    """paths_cases.arbitrary_batch against the scene of `dev`, the first hits of the stock interval from rd.QueryRays"""
    plt, tlas = dev.plt, dev.topAccelStruct

    def first_t(rays):
        h = sh.read(rd, plt, rd.QueryRays(tlas, sh.upload(rd, plt, rays), rays.shape[0], rd.QUERY_CLOSEST), rays.shape[0], rd.RAY_HIT_DTYPE)
        return h["hit"] == 1, h["t"]
    lo, hi = scene_box(rd, dev)
    return pc.arbitrary_batch(rd, lo, hi, first_t, seed)


@pytest.fixture(scope="module")
def batches(mods, golden):
    """per golden scene: the arbitrary batch and the answer of the loop over the public calls at DEPTH, computed once"""
    rd, _ = mods
    cache = {}

    def get(name):
        if name not in cache:
            dev = golden(name).dev
            rays, keys, kind = batch_for(rd, dev, SEED[name])
            rad, counts, first = pc.public_loop(rd, dev.plt, dev.topAccelStruct, dev.shading_buffers(), rays, keys, DEPTH)
            cache[name] = dict(rays=rays, keys=keys, kind=kind, rad=rad, counts=counts, first=first)
        return cache[name]
    return get


def check_radiance(got, want, tag):
    eq = (sh.bits(got) == sh.bits(want)).all(1)
    assert eq.all(), "%s: radiance differs from the loop over the public calls on %d of %d rays (first: %s)" % (
        tag, int((~eq).sum()), eq.shape[0], np.flatnonzero(~eq)[:8].tolist())
    assert not sh.bits(got[:, 3]).any(), "%s: radiance.w is not 0" % tag


def frames_through_trace_paths(rd, dev, nframes=2):
    """`nframes` progressive frames of the scene's own camera, batchSize and depth into buffers of their own: per sample
    GenerateRays -> TracePaths -> Accumulate -> [(imageScratch (npix, 4) float32, image (npix, 4) uint8) after each frame]"""
    plt, npix, p = dev.plt, dev.width * dev.height, dev.scene.rtprop
    cam, sb = dev.frame_buffers()[0], dev.shading_buffers()
    scratch, image = rd.CreateBuffer(plt, 16 * npix), rd.CreateImage(plt, dev.width, dev.height)
    rd.WriteBuffer(plt, scratch, 16 * npix, np.zeros(4 * npix, F))
    batch, depth, total, out = int(p["batchSize"]), int(p["depth"]), 0, []
    for _ in range(nframes):
        for it in range(batch):
            rays, keys = rd.GenerateRays(cam, npix, total + it, total)
            radiance = rd.TracePaths(dev.topAccelStruct, rays, keys, npix, depth, sb)
            assert rd.Accumulate(radiance, npix, total + it, scratch, image) == 0
        total += batch
        out.append((rd.ReadBuffer(plt, scratch, 16 * npix).view(F).reshape(npix, 4).copy(), rd.ReadBuffer(plt, image, 4 * npix).reshape(npix, 4).copy()))
    return out


# ---- 1. recorded frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.SCENES)
def test_recorded_frames(mods, golden, name):
    """per sample GenerateRays -> TracePaths -> Accumulate with the image, batchSize samples a frame, two frames: imageScratch and
    the RGBA8 image equal the reference's recorded frames and what this library's own TraceRays leaves in the scene's buffers"""
    rd, _ = mods
    c = golden(name)
    dev = c.dev
    npix = dev.width * dev.height
    dev.bind()
    got = frames_through_trace_paths(rd, dev)
    dev.set_rtprop(totalSamples=0); dev.clear_scratch()
    try:
        for f in range(2):
            eq = (sh.bits(got[f][0]) == sh.bits(np.ascontiguousarray(c.G["scratch%d" % f]).reshape(-1, 4))).all(1)
            assert eq.all(), "%s frame %d: imageScratch differs from the recording on %d of %d pixels" % (name, f, int((~eq).sum()), npix)
            eq = (got[f][1] == c.G["image%d" % f].reshape(-1, 4)).all(1)
            assert eq.all(), "%s frame %d: the image differs from the recording on %d of %d pixels" % (name, f, int((~eq).sum()), npix)
            img = dev.render()
            assert same(got[f][0], dev.read_scratch().reshape(-1, 4)) and same(got[f][1], img.reshape(-1, 4)), (name, f)
    finally:
        dev.set_rtprop(totalSamples=0); dev.clear_scratch()


# ---- 2. arbitrary rays against the loop over the public calls ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c1", "c2"))
def test_arbitrary_rays(mods, golden, batches, name):
    """1037 rays no camera makes -- origins inside and outside the scene box, directions of any length and axis-aligned ones, every
    interval kind, a frameID per ray, repeated pixels, junk in the key's unused words -- at depth 4: radiance equals the loop over
    rd.QueryRays / rd.ShadeHits for every ray, w is 0, and `hits` holds what rd.QueryRays writes for the first segment"""
    rd, _ = mods
    dev, b = golden(name).dev, batches(name)
    n = b["rays"].shape[0]
    print("%s: counts per depth %s, kinds %s" % (name, b["counts"], np.bincount(b["kind"], minlength=len(pc.KINDS)).tolist()))
    # the stated cases are present, by the loop's own counts
    assert n == 1037 and all(int((b["kind"] == k).sum()) >= 1 for k in range(len(pc.KINDS)))
    assert len(b["counts"]) >= 3 and b["counts"][2] >= 0.25 * n, "fewer than 25 %% of the rays survive two bounces: %s" % b["counts"]
    hit = b["first"]["hit"] == 1
    assert not hit[b["kind"] == 1].any() and not hit[b["kind"] == 3].any() and not hit[b["kind"] == 4].any()     # tmax before the first hit, NaN, tmax 0
    rad, hits = pc.trace_paths(rd, dev.plt, dev.topAccelStruct, dev.shading_buffers(), b["rays"], b["keys"], DEPTH)
    check_radiance(rad, b["rad"], name)
    assert same(hits, b["first"]), "%s: `hits` differs from rd.QueryRays" % name
    want = sh.read(rd, dev.plt, rd.QueryRays(dev.topAccelStruct, sh.upload(rd, dev.plt, b["rays"]), n, rd.QUERY_CLOSEST), n, rd.RAY_HIT_DTYPE)
    assert same(hits, want)
    # without `hits` the internal scratch serves: the same radiance
    assert same(pc.trace_paths(rd, dev.plt, dev.topAccelStruct, dev.shading_buffers(), b["rays"], b["keys"], DEPTH, want_hits=False)[0], rad)
    assert rad[:, :3].any() and np.unique(sh.bits(rad[:, :3]), axis=0).shape[0] > n // 8


# ---- 3. outputs stay inside their ranges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 64))
def test_outputs_stay_inside_their_ranges(mods, golden, batches, n):
    """radiance and hits in the middle of sentinel-filled allocations, through wrapped views of the middle (the Frame pattern of
    tests/test_gpu_raygen.py) AND at non-zero offsets into them: the n records are the batch's first n, every byte outside the
    two ranges -- records from n on included -- keeps the sentinel"""
    rd, _ = mods
    dev, b = golden("c1").dev, batches("c1")
    plt = dev.plt
    lead, off_r, off_h, room, tail = 256, 48, 96, 3, 512
    allR, allH = rc.filled(rd, plt, lead + off_r + 16 * (n + room) + tail), rc.filled(rd, plt, lead + off_h + 32 * (n + room) + tail)
    wR = rd.WrapDeviceMemory(plt, allR.device_ptr + lead, off_r + 16 * (n + room), keepalive=allR)
    wH = rd.WrapDeviceMemory(plt, allH.device_ptr + lead, off_h + 32 * (n + room), keepalive=allH)
    ret = rd.TracePaths(dev.topAccelStruct, sh.upload(rd, plt, b["rays"][:n], 64), sh.upload(rd, plt, b["keys"][:n], 64), n, DEPTH, dev.shading_buffers(),
                        radiance=wR, hits=wH, radiance_offset=off_r, hits_offset=off_h)
    assert ret is wR
    r, h = rc.whole(rd, plt, allR), rc.whole(rd, plt, allH)
    r0, h0 = lead + off_r, lead + off_h
    check_radiance(r[r0:r0 + 16 * n].view(F).reshape(n, 4), b["rad"][:n], "n = %d" % n)
    assert same(h[h0:h0 + 32 * n], b["first"][:n])
    assert (r[:r0] == S).all() and (r[r0 + 16 * n:] == S).all(), "a byte outside the radiance range was written"
    assert (h[:h0] == S).all() and (h[h0 + 32 * n:] == S).all(), "a byte outside the hit range was written"


# ---- 4. options do not matter -------------------------------------------------------------------------------------------------------
def test_options_do_not_matter(mods, golden, batches):
    rd, _ = mods
    dev, b = golden("c2").dev, batches("c2")
    run = lambda: pc.trace_paths(rd, dev.plt, dev.topAccelStruct, dev.shading_buffers(), b["rays"], b["keys"], DEPTH)
    rad, hits = run()
    check_radiance(rad, b["rad"], "defaults")
    settings = [("kernel", v) for v in (0, 1, 2, 3)] + [(o, v) for o in ("sort", "fuse", "quad", "cull", "group_entry_items") for v in (0, 1)] + [("chunk_paths", 100)]
    try:
        for opt, value in settings:
            rd.SetOption(opt, value)
            got_r, got_h = run()
            st = rd.GetTraceStats()
            rd.SetOption(opt, DEFAULTS[opt])
            assert same(got_r, rad) and same(got_h, hits), "option %s = %d changes the result" % (opt, value)
            if opt == "chunk_paths":      # eleven chunks, the last partial: one first-segment launch each
                assert st.rays_primary == rad.shape[0] and st.launches_extend >= 11
    finally:
        for opt, value in DEFAULTS.items():
            rd.SetOption(opt, value)
    assert same(run()[0], rad)


# ---- 5. depths ----------------------------------------------------------------------------------------------------------------------
def test_depths(mods, golden, batches):
    """max_depth 0: zeros (and `hits` is still the query's); 1: the loop with `next` NULL -- no next direction is sampled; 8; 62 is
    the last accepted depth and 63 is refused"""
    rd, _ = mods
    dev, b = golden("c1").dev, batches("c1")
    plt, tlas, sb = dev.plt, dev.topAccelStruct, dev.shading_buffers()
    rad, hits = pc.trace_paths(rd, plt, tlas, sb, b["rays"], b["keys"], 0)
    assert not rad.view(np.uint8).any() and same(hits, b["first"])
    assert not pc.trace_paths(rd, plt, tlas, sb, b["rays"], b["keys"], 0, want_hits=False)[0].view(np.uint8).any()
    for depth in (1, 8):
        want, counts, _ = pc.public_loop(rd, plt, tlas, sb, b["rays"], b["keys"], depth)
        rad, hits = pc.trace_paths(rd, plt, tlas, sb, b["rays"], b["keys"], depth)
        check_radiance(rad, want, "depth %d" % depth)
        assert same(hits, b["first"]) and len(counts) <= depth + 1
        assert not same(rad, b["rad"]), "depth %d gives the radiance of depth %d" % (depth, DEPTH)
    bR, bK = sh.upload(rd, plt, b["rays"]), sh.upload(rd, plt, b["keys"])
    out = rc.filled(rd, plt, 16 * b["rays"].shape[0])
    with pytest.raises(rd.RadianceError, match="rdx_trace_paths.*63"):
        rd.TracePaths(tlas, bR, bK, b["rays"].shape[0], 63, sb, radiance=out)
    assert (rc.whole(rd, plt, out) == S).all()
    rd.TracePaths(tlas, bR, bK, 64, 62, sb, radiance=out)


# ---- 6. other scene kinds -----------------------------------------------------------------------------------------------------------
def test_instance_sbt_offsets(mods):
    """the scene tests/test_gpu_shade.py and tests/test_gpu_parity.py::test_instance_sbt_offsets use: two instances with SBTOffset 1
    dispatch row 2 -- the reference-order kernel route.  The comparand here is the frame path (which test_gpu_parity.py and
    test_gpu_reference.py hold to the oracle and to the reference's device code), not the loop over the public calls: a SHADOW
    ray that meets an instance with an offset dispatches row offset + 2, which has no hit shader, so it does not occlude -- the
    frame path's shadow stage knows the instance it met, rd.QueryRays(..., QUERY_ANY) reports `hit` alone.  Two progressive
    frames through GenerateRays -> TracePaths -> Accumulate equal what TraceRays leaves; `hits` equals rd.QueryRays"""
    rd, scenes = mods
    s = scenes.c1_cornell(96, 54, spp=2, depth=4, sphere_subdiv=3)
    s.sbt_offsets = {5: 1, 7: 1}
    dev = scenes.DeviceScene(s)
    plt, npix = dev.plt, dev.width * dev.height
    got = frames_through_trace_paths(rd, dev)
    dev.set_rtprop(totalSamples=0); dev.clear_scratch()
    for f in range(2):
        img = dev.render()
        eq = (sh.bits(got[f][0]) == sh.bits(dev.read_scratch().reshape(-1, 4))).all(1)
        assert eq.all(), "frame %d: imageScratch differs from TraceRays' on %d of %d pixels" % (f, int((~eq).sum()), npix)
        assert same(got[f][1], img.reshape(-1, 4)), f
    rays, keys = rd.GenerateRays(dev.frame_buffers()[0], npix, 0, 0)
    _, bH = rd.TracePaths(dev.topAccelStruct, rays, keys, npix, DEPTH, dev.shading_buffers(), hits=True)
    first = sh.read(rd, plt, bH, npix, rd.RAY_HIT_DTYPE)
    assert same(first, sh.read(rd, plt, rd.QueryRays(dev.topAccelStruct, rays, npix, rd.QUERY_CLOSEST), npix, rd.RAY_HIT_DTYPE))
    assert int(((first["hit"] == 1) & (first["instanceSBTOffset"] == 1)).sum()) > 200


def test_textures(mods):
    """option "textures" 1 with an image array and a sampler: the loop over the public calls under the same option, and not the
    radiance of textures 0"""
    rd, scenes = mods
    dev = scenes.DeviceScene(_textured_scene(scenes, 96, 54))
    plt = dev.plt
    tex = _test_textures()
    img = rd.CreateImageArray(plt, 64, 64, 3)
    for l in range(3):
        rd.WriteImage(plt, img, 64, 64, l, tex[l])
    rays, keys, _ = batch_for(rd, dev, 11)
    sb = dev.shading_buffers(img, rd.CreateSampler(plt, rd.RD_ADDRESS_REPEAT, rd.RD_FILTER_LINEAR))
    off = pc.trace_paths(rd, plt, dev.topAccelStruct, sb, rays, keys, DEPTH)[0]
    check_radiance(off, pc.public_loop(rd, plt, dev.topAccelStruct, sb, rays, keys, DEPTH)[0], "textures 0")
    try:
        rd.SetOption("textures", 1)
        want, counts, first = pc.public_loop(rd, plt, dev.topAccelStruct, sb, rays, keys, DEPTH)
        rad, hits = pc.trace_paths(rd, plt, dev.topAccelStruct, sb, rays, keys, DEPTH)
        check_radiance(rad, want, "textures 1")
        print("textures: counts %s" % counts)
        assert same(hits, first) and counts[1] >= 50 and not same(rad, off)
        with pytest.raises(rd.RadianceError, match="rdx_trace_paths.*uv"):
            rd.TracePaths(dev.topAccelStruct, sh.upload(rd, plt, rays), sh.upload(rd, plt, keys), rays.shape[0], DEPTH,
                          rd.ShadingBuffers(dev.rdSceneData, dev.meshInfoData, dev.indexData, None, dev.normalData, dev.materialData, img))
    finally:
        rd.SetOption("textures", 0)
        dev.bind()


def test_after_update_accel_struct(mods):
    """the 9-instance grid sharing two BLAS: the last instance is carried far away, then the first nudged.  Each time the radiance
    is bitwise what a freshly built TLAS gives -- by TracePaths and by the loop over the public calls -- and differs from before"""
    rd, scenes = mods
    s = _decorated(scenes, "shared_blas")
    dev = scenes.DeviceScene(s)
    rays, keys, _ = batch_for(rd, dev, 3)
    prev = pc.trace_paths(rd, dev.plt, dev.topAccelStruct, dev.shading_buffers(), rays, keys, DEPTH)[0]
    insts = tu.instances(s)
    for move in ("B", "A"):
        insts = tu.apply(insts, move)
        rd.UpdateAccelStruct(dev.plt, dev.topAccelStruct, tu.rd_instances(rd, insts, dev.blas))
        got, got_h = pc.trace_paths(rd, dev.plt, dev.topAccelStruct, dev.shading_buffers(), rays, keys, DEPTH)
        t = scenes.Scene(s.name)
        t.meshes, t.materials, t.camera, t.sceneProps, t.rtprop = s.meshes, s.materials, s.camera, s.sceneProps, s.rtprop
        for mi, tf, sbt, mat in insts:
            t.add_instance(mi, tf, mat, sbt)
        fresh = scenes.DeviceScene(t)
        want, want_h = pc.trace_paths(rd, fresh.plt, fresh.topAccelStruct, fresh.shading_buffers(), rays, keys, DEPTH)
        assert same(got, want) and same(got_h, want_h), move
        check_radiance(got, pc.public_loop(rd, fresh.plt, fresh.topAccelStruct, fresh.shading_buffers(), rays, keys, DEPTH)[0], "after move %s" % move)
        assert not same(got, prev), move
        prev = got


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(mods, golden, batches):
    """every refusal of include/rdx.h returns an error that names the call, and leaves the sentinel-filled outputs as they were;
    n == 0 succeeds and writes nothing"""
    rd, _ = mods
    dev, b = golden("c1").dev, batches("c1")
    plt, tl = dev.plt, dev.topAccelStruct
    n, tail = 200, 128
    bR, bK = sh.upload(rd, plt, b["rays"][:n], tail), sh.upload(rd, plt, b["keys"][:n], tail)
    oR, oH = rc.filled(rd, plt, 16 * n + tail), rc.filled(rd, plt, 32 * n + tail)
    one = rc.filled(rd, plt, 32 * n * 4)            # rays | keys | room for outputs, for the overlap cases
    rd.WriteBuffer(plt, one, 32 * n, b["rays"][:n])
    rd.WriteBuffer(plt, one, 16 * n, b["keys"][:n], offset=32 * n)
    null, unknown = rd.Buffer(None, 1 << 20), rd.Buffer(12345678, 1 << 20)
    outs = dict(radiance=oR, hits=oH, one=one)
    snapshot = lambda: {k: rc.whole(rd, plt, v) for k, v in outs.items()}
    good = snapshot()
    SB = lambda **kw: rd.ShadingBuffers(**{**dict(scene=dev.rdSceneData, meshInfo=dev.meshInfoData, index=dev.indexData, uv=dev.uvData, normal=dev.normalData,
                                                 material=dev.materialData), **kw})

    def run(**kw):
        a = dict(tlas=tl, rays=bR, keys=bK, n=n, max_depth=DEPTH, scene_buffers=dev.shading_buffers(), radiance=oR, hits=oH)
        a.update(kw)
        return rd.TracePaths(a.pop("tlas"), a.pop("rays"), a.pop("keys"), a.pop("n"), a.pop("max_depth"), a.pop("scene_buffers"), **a)

    wrapped = lambda buf, shift, size: rd.WrapDeviceMemory(plt, buf.device_ptr + shift, size, keepalive=buf)
    in_one = dict(rays=one, rays_offset=0, keys=one, keys_offset=32 * n)
    cases = [
        ("null tlas", dict(tlas=null), "TLAS"), ("unknown tlas", dict(tlas=unknown), "TLAS"),
        ("null rays", dict(rays=null), "ray buffer handle"), ("unknown rays", dict(rays=unknown), "ray buffer handle"),
        ("null keys", dict(keys=null), "key buffer handle"), ("unknown keys", dict(keys=unknown), "key buffer handle"),
        ("null radiance", dict(radiance=null), "radiance buffer handle"), ("unknown radiance", dict(radiance=unknown), "radiance buffer handle"),
        ("unknown hits", dict(hits=unknown), "hit buffer handle"),
        ("null scene", dict(scene_buffers=SB(scene=null)), "SceneProperties"), ("null meshInfo", dict(scene_buffers=SB(meshInfo=null)), "meshInfo"),
        ("null index", dict(scene_buffers=SB(index=null)), "index"), ("null normal", dict(scene_buffers=SB(normal=null)), "normal"),
        ("null material", dict(scene_buffers=SB(material=null)), "material"),
        ("unknown uv", dict(scene_buffers=SB(uv=rd.Buffer(12345678, 64))), "uv"),
        ("unknown textureArray", dict(scene_buffers=SB(textureArray=rd.Buffer(12345678, 64))), "textureArray"),
        ("a scene buffer smaller than SceneProperties", dict(scene_buffers=SB(scene=rd.CreateBuffer(plt, 160))), "SceneProperties"),
        ("max_depth 63", dict(max_depth=63), "63"), ("max_depth 2^31", dict(max_depth=1 << 31), "62"),
        ("rays_offset 8", dict(rays_offset=8), "16"), ("keys_offset 4", dict(keys_offset=4), "16"), ("radiance_offset 8", dict(radiance_offset=8), "16"),
        ("hits_offset 24", dict(hits_offset=24), "16"),
        ("rays past the end", dict(rays_offset=tail + 16), "ray buffer"), ("keys past the end", dict(keys_offset=tail + 16), "key buffer"),
        ("radiance past the end", dict(radiance_offset=tail + 16), "radiance buffer"), ("hits past the end", dict(hits_offset=tail + 16), "hit buffer"),
        ("radiance one record short", dict(radiance=rd.CreateBuffer(plt, 16 * n - 16)), "radiance buffer"),
        ("hits one record short", dict(hits=rd.CreateBuffer(plt, 32 * n - 16)), "hit buffer"),
        ("an offset beyond the buffer", dict(keys_offset=1 << 30), "key buffer"),
        ("radiance over the rays' tail", dict(in_one, radiance=one, radiance_offset=32 * n - 16), "overlap"),
        ("radiance over the keys", dict(in_one, radiance=one, radiance_offset=32 * n), "overlap"),
        ("hits = the rays", dict(in_one, hits=one, hits_offset=0), "overlap"),
        ("hits over the keys' tail", dict(in_one, hits=one, hits_offset=48 * n - 16), "overlap"),
        ("hits over the radiance", dict(radiance=one, radiance_offset=64 * n, hits=one, hits_offset=80 * n - 16), "overlap"),
        ("hits = the radiance", dict(radiance=one, radiance_offset=64 * n, hits=one, hits_offset=64 * n), "overlap"),
        ("radiance wraps the rays' memory", dict(radiance=wrapped(bR, 0, 16 * n)), "overlap"),
        ("misaligned wrapped rays", dict(rays=wrapped(bR, 8, 32 * n + 64)), "aligned"),
        ("misaligned wrapped keys", dict(keys=wrapped(bK, 4, 16 * n + 64)), "aligned"),
        ("misaligned wrapped radiance", dict(radiance=wrapped(oR, 8, 16 * n + 64)), "aligned"),
        ("misaligned wrapped hits", dict(hits=wrapped(oH, 8, 32 * n + 64)), "aligned"),
        ("misaligned wrapped index stream", dict(scene_buffers=SB(index=wrapped(dev.indexData, 2, dev.indexData.size - 2))), "aligned"),
    ]
    for what, kw, word in cases:
        with pytest.raises(rd.RadianceError) as e:
            run(**kw)
        assert word in str(e.value) and "rdx_trace_paths" in str(e.value), (what, str(e.value))
        now = snapshot()
        for k in outs:
            assert np.array_equal(now[k], good[k]), (what, k)
    from radiance_ray_tracing_amd import _lib
    L = _lib.lib()
    assert L.rdx_trace_paths(tl.handle, bR.handle, 0, bK.handle, 0, n, DEPTH, None, oR.handle, 0, None, 0) != 0
    assert "scene" in _lib.last_error() and "rdx_trace_paths" in _lib.last_error()
    unknown_sampler = _lib.rdx_shading_buffers(dev.rdSceneData.handle, dev.meshInfoData.handle, dev.indexData.handle, None, dev.normalData.handle,
                                              dev.materialData.handle, None, 12345678)
    assert L.rdx_trace_paths(tl.handle, bR.handle, 0, bK.handle, 0, n, DEPTH, C.byref(unknown_sampler), oR.handle, 0, None, 0) != 0
    assert "sampler" in _lib.last_error() and "rdx_trace_paths" in _lib.last_error()
    # n == 0 returns 0 and writes nothing -- also at the very end of the buffers
    assert L.rdx_trace_paths(tl.handle, bR.handle, 0, bK.handle, 0, 0, DEPTH, C.byref(dev.shading_buffers()._struct()), oR.handle, 0, oH.handle, 0) == 0
    assert run(n=0) is oR and run(n=0, rays_offset=32 * n + tail, keys_offset=16 * n + tail, radiance_offset=16 * n + tail, hits_offset=32 * n + tail) is oR
    assert all(np.array_equal(v, good[k]) for k, v in snapshot().items())
    # adjacent ranges of one buffer are fine, and the call still works after the refusals
    run(**in_one, radiance=one, radiance_offset=48 * n, hits=one, hits_offset=64 * n)
    check_radiance(rd.ReadBuffer(plt, one, 16 * n, offset=48 * n).view(F).reshape(n, 4), b["rad"][:n], "adjacent ranges")
    assert same(rd.ReadBuffer(plt, one, 32 * n, offset=64 * n), b["first"][:n])
    assert (rd.ReadBuffer(plt, one, 32 * n, offset=96 * n) == S).all()


# ---- 8. torch tensors -----------------------------------------------------------------------------------------------------------------
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
import paths_cases as pc
import shade_cases as sh
F = np.float32
c = sh.Golden(rd, scenes, "c0")
dev, plt, tlas = c.dev, c.dev.plt, c.dev.topAccelStruct
sb = dev.shading_buffers()
cam, scratch, image = dev.frame_buffers()
npix = dev.width * dev.height
p = c.s.rtprop
depth, batch = int(p["depth"]), int(p["batchSize"])
# the buffer route and the tensor route on the same inputs
rays, keys = rd.GenerateRaysTorch(cam, npix, 5, 4)
rays = (rays * torch.tensor([1, 1, 1, 1, 2.5, 2.5, 2.5, 1], device="cuda")).contiguous()       # a tensor a torch op produced: non-unit directions
rn = rays.cpu().numpy().view(rd.RAY_DTYPE).reshape(-1)
kn = keys.cpu().numpy().view(rd.SHADE_KEY_DTYPE).reshape(-1)
want_r, want_h = pc.trace_paths(rd, plt, tlas, sb, rn, kn, depth)
got = rd.TracePathsTorch(tlas, rays, keys, depth, sb)
assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == (npix, 4) and got.is_cuda
assert np.array_equal(got.cpu().numpy().view(np.uint32), want_r.view(np.uint32))
got2, hits = rd.TracePathsTorch(tlas, rays, keys, depth, sb, want_hits=True)
assert hits.dtype == torch.int32 and tuple(hits.shape) == (npix, 8)
assert torch.equal(got2.view(torch.int32), got.view(torch.int32))
assert np.array_equal(hits.cpu().numpy().view(np.uint8).reshape(-1), want_h.view(np.uint8).reshape(-1))
assert torch.equal(hits, rd.QueryRaysTorch(tlas, rays, rd.QUERY_CLOSEST))
assert want_r[:, :3].any()
# frame c0 through the three torch calls: the recording
dev.clear_scratch()
for f in range(2):
    for it in range(batch):
        r, k = rd.GenerateRaysTorch(cam, npix, f * batch + it, f * batch)
        rd.AccumulateTorch(rd.TracePathsTorch(tlas, r, k, depth, sb), f * batch + it, scratch, image)
    assert np.array_equal(dev.read_scratch().reshape(-1).view(np.uint32), c.G["scratch%d" % f].view(np.uint32)), f
    assert np.array_equal(rd.ReadBuffer(plt, image, 4 * npix), c.G["image%d" % f]), f
dev.clear_scratch()
empty = rd.TracePathsTorch(tlas, rays[:0], keys[:0], depth, sb, want_hits=True)
assert tuple(empty[0].shape) == (0, 4) and tuple(empty[1].shape) == (0, 8)
wide = torch.zeros((npix, 16), dtype=torch.float32, device="cuda")
bad = [dict(rays=rays[:, :7]), dict(rays=rays.double()), dict(rays=rays.cpu()), dict(rays=wide[:, ::2]), dict(rays=rn), dict(keys=keys.long()),
       dict(keys=keys[:, :3]), dict(keys=keys[:-1]), dict(keys=keys.cpu()), dict(keys=keys.float()), dict(max_depth=-1), dict(max_depth=2.0), dict(sb=(1, 2))]
for j, kw in enumerate(bad):
    a = dict(rays=rays, keys=keys, max_depth=depth, sb=sb)
    a.update(kw)
    try:
        rd.TracePathsTorch(tlas, a["rays"], a["keys"], a["max_depth"], a["sb"])
    except rd.RadianceError:
        continue
    raise AssertionError("TracePathsTorch: bad argument set %d was accepted" % j)
print("TORCH-PATHS-OK", npix)
"""


def test_torch_tensors_in_a_fresh_process(gpu):
    """rd.TracePathsTorch equals rd.TracePaths on the same inputs bit for bit; GenerateRaysTorch -> TracePathsTorch -> AccumulateTorch
    writes the recorded frames of c0; a non-contiguous tensor, a wrong dtype, shape or device is refused in Python.  torch is
    initialised first, in a process of its own (as tests/test_gpu_raygen.py does)"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _TORCH_CHILD, ROOT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "TORCH-PATHS-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


# ---- 9. stats -------------------------------------------------------------------------------------------------------------------------
def test_stats_equal_the_frame_paths(mods, golden):
    """after the first sample of c1's first frame through GenerateRays -> TracePaths, the ray counts of rdx_get_trace_stats and
    rdx_get_bounce_counts equal those of TraceRays for the same frame at batchSize 1"""
    rd, _ = mods
    c = golden("c1")
    dev, plt = c.dev, c.dev.plt
    npix, depth = dev.width * dev.height, int(c.s.rtprop["depth"])
    dev.bind()
    rays, keys = rd.GenerateRays(dev.frame_buffers()[0], npix, 0, 0)
    rd.SetProfiling(True)
    try:
        rd.TracePaths(dev.topAccelStruct, rays, keys, npix, depth, dev.shading_buffers())
        st, counts = rd.GetTraceStats(), rd.GetBounceCounts(depth + 2).copy()
    finally:
        rd.SetProfiling(False)
    mine = {k: int(getattr(st, k)) for k in ("pixels", "rays_primary", "rays_bounce", "rays_shadow", "closest_hits", "launches_extend", "launches_shadow")}
    assert st.ms_total > 0 and st.ms_shade > 0 and st.ms_extend > 0 and st.ms_generate > 0 and st.ms_accumulate == 0
    dev.set_rtprop(totalSamples=0, batchSize=1); dev.clear_scratch()
    try:
        dev.render()
        ft, fcounts = rd.GetTraceStats(), rd.GetBounceCounts(depth + 2)
        theirs = {k: int(getattr(ft, k)) for k in mine}
    finally:
        dev.set_rtprop(totalSamples=0, batchSize=int(c.s.rtprop["batchSize"])); dev.clear_scratch()
    print("trace_paths", mine, counts.tolist(), "trace_rays", theirs, fcounts.tolist())
    assert mine == theirs and np.array_equal(counts, fcounts)
    assert mine["rays_primary"] == npix and mine["rays_bounce"] > 0 and mine["rays_shadow"] > 0 and counts[0] == npix

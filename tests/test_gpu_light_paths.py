"""GPU suite (-m gpu): rd.TraceLightPaths and its torch route (rdx_trace_paths_lights) -- radiance along the caller's own rays with
every light of the scene sampled at every hit, in one call.

Comparands, in this order of authority:
  1. the README's second Quick-start loop over the public calls, scatter_cases.path_tracer_numpy, which tests/test_gpu_scatter.py
     holds -- for one light -- to the reference's recorded frames;
  2. rd.TracePaths, for one light;
  3. the reference's own device code, recorded (tests/golden/refgpu_c0.npz), for one light through GenerateRays -> TraceLightPaths
     -> Accumulate.
Every bar is equality of bits.  The batch is paths_cases.arbitrary_batch (n = 1037: four blocks, the last one partial and ending in
a partial wave) on c1 and c2 with the seeds of test_gpu_paths.py, at depth 4, under light_paths_cases.five_lights.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import light_paths_cases as lp
import material_cases as mc
import paths_cases as pc
import raygen_cases as rc
import scatter_cases as sc
import shade_cases as sh
from test_gpu_paths import DEFAULTS, SEED, batch_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
S = rc.SENTINEL
DEPTH = 4
COUNTS = (0, 1, 2, 3, 5)


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


same = mc.same


class Case:
    """one golden scene under the five lights: the arbitrary batch, and per light count the answer of the README's loop, computed
    once and left unchanged"""

    def __init__(self, rd, dev, seed):
        self.rd, self.dev, self.plt, self.tlas = rd, dev, dev.plt, dev.topAccelStruct
        self.rays, self.keys, self.kind = batch_for(rd, dev, seed)
        self.n = self.rays.shape[0]
        self.sp = lp.five_lights(rd)
        self.scene = lp.scene_buffer(rd, self.plt, self.sp)
        self.sb = lp.buffers_with_scene(rd, dev, self.scene)
        self.occlusion = lp.occlusion_at_depth0(rd, dev, self.scene, self.rays)
        self._want = {}

    def want(self, light_count, depth=DEPTH):
        """(color (n, 3), live rays per bounce) of scatter_cases.path_tracer_numpy"""
        if (light_count, depth) not in self._want:
            color, _, lives = sc.path_tracer_numpy(self.rd, self.dev, self.scene, light_count, self.rays, self.keys["frameID"], self.keys["pixel"], depth)
            self._want[(light_count, depth)] = (color, lives)
        return self._want[(light_count, depth)]

    def run(self, light_count, depth=DEPTH, sb=None):
        return lp.trace(self.rd, self.plt, self.tlas, sb or self.sb, self.rays, self.keys, depth, light_count)


@pytest.fixture(scope="module")
def cases(mods, golden):
    rd, _ = mods
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Case(rd, golden(name).dev, SEED[name])
        return cache[name]
    return get


def check_radiance(got, want_color, tag):
    eq = (sh.bits(got[:, :3]) == sh.bits(want_color)).all(1)
    assert eq.all(), "%s: radiance differs from the README's loop on %d of %d rays (first: %s)" % (tag, int((~eq).sum()), eq.shape[0], np.flatnonzero(~eq)[:8].tolist())
    assert not sh.bits(got[:, 3]).any(), "%s: radiance.w is not 0" % tag


def expected_counts(n, lives, depth=DEPTH):
    out = np.zeros(depth + 2, np.uint64)
    out[0] = n
    out[1:1 + len(lives)] = lives
    return out


# ---- 1. the README loop ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c1", "c2"))
def test_the_comparand_is_not_vacuous(cases, name):
    """by the public calls alone: at least 25 % of the rays are alive for two bounces, and every one of the five lights has at least
    20 depth-0 hits whose shadow ray is occluded and at least 20 whose shadow ray is not"""
    c = cases(name)
    _, lives = c.want(5)
    print("%s: live rays per bounce %s, (occluded, visible) per light at depth 0 %s" % (name, lives, c.occlusion))
    assert c.n == 1037 and len(lives) >= 2 and lives[1] >= 0.25 * c.n, lives
    for j, (occ, vis) in enumerate(c.occlusion):
        assert occ >= 20 and vis >= 20, "%s light %d: %d occluded, %d visible" % (name, j, occ, vis)


@pytest.mark.parametrize("light_count", COUNTS)
@pytest.mark.parametrize("name", ("c1", "c2"))
def test_the_readme_loop(mods, cases, name, light_count):
    rd, _ = mods
    c = cases(name)
    color, lives = c.want(light_count)
    got, invalid = c.run(light_count)
    counts = rd.GetBounceCounts(DEPTH + 2).copy()
    check_radiance(got, color, "%s, %d lights" % (name, light_count))
    assert invalid == 0
    assert np.array_equal(counts, expected_counts(c.n, lives)), (counts.tolist(), lives)
    assert len(lives) >= 2 and lives[1] >= 0.25 * c.n
    if light_count:      # the lights matter: on 20 paths at the least the colour is not that of the ambient term alone
        assert (sh.bits(c.want(0)[0]) != sh.bits(color)).any(1).sum() >= 20


# ---- 2. one light -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c0", "c1", "c2"))
def test_one_light_is_trace_paths(mods, golden, name):
    """with the scene's own SceneProperties and light_count 1: the bits of rd.TracePaths"""
    rd, _ = mods
    dev = golden(name).dev
    rays, keys, _ = batch_for(rd, dev, SEED.get(name, 20261021))
    sb = dev.shading_buffers()
    want, _ = pc.trace_paths(rd, dev.plt, dev.topAccelStruct, sb, rays, keys, DEPTH, want_hits=False)
    got, invalid = lp.trace(rd, dev.plt, dev.topAccelStruct, sb, rays, keys, DEPTH, 1)
    eq = (sh.bits(got) == sh.bits(want)).all(1)
    assert eq.all() and invalid == 0, "%s: differs from rd.TracePaths on %d of %d rays" % (name, int((~eq).sum()), eq.shape[0])
    assert want[:, :3].any() and np.unique(sh.bits(want[:, :3]), axis=0).shape[0] > rays.shape[0] // 8


def test_one_light_writes_the_recorded_frames(mods, golden):
    """c0, the smallest golden scene: per sample GenerateRays -> TraceLightPaths(1) -> Accumulate, batchSize samples a frame, two
    frames: imageScratch and the RGBA8 image are the reference's recorded scratch0 / image0 and scratch1 / image1"""
    rd, _ = mods
    c = golden("c0")
    dev = c.dev
    plt, npix, p = dev.plt, dev.width * dev.height, dev.scene.rtprop
    cam, sb = dev.frame_buffers()[0], dev.shading_buffers()
    scratch, image = rd.CreateBuffer(plt, 16 * npix), rd.CreateImage(plt, dev.width, dev.height)
    rd.WriteBuffer(plt, scratch, 16 * npix, np.zeros(4 * npix, F))
    batch, depth, total = int(p["batchSize"]), int(p["depth"]), 0
    for f in range(2):
        for it in range(batch):
            rays, keys = rd.GenerateRays(cam, npix, total + it, total)
            radiance, invalid = rd.TraceLightPaths(dev.topAccelStruct, rays, keys, npix, depth, 1, sb)
            assert invalid == 0 and rd.Accumulate(radiance, npix, total + it, scratch, image) == 0
        total += batch
        got_s = rd.ReadBuffer(plt, scratch, 16 * npix).view(F).reshape(npix, 4)
        eq = (sh.bits(got_s) == sh.bits(np.ascontiguousarray(c.G["scratch%d" % f]).reshape(-1, 4))).all(1)
        assert eq.all(), "frame %d: imageScratch differs from the recording on %d of %d pixels" % (f, int((~eq).sum()), npix)
        assert np.array_equal(rd.ReadBuffer(plt, image, 4 * npix).reshape(-1), c.G["image%d" % f].reshape(-1)), f


# ---- 3. the lights are read per call ----------------------------------------------------------------------------------------------------
def test_lights_are_read_by_every_call(mods, cases, golden):
    """lights[1] of a scene buffer is rewritten between two calls: the second call has the bits of the loop for the new light"""
    rd, _ = mods
    c = cases("c1")
    dev = c.dev
    sp = c.sp.copy()
    scene = lp.scene_buffer(rd, c.plt, sp)
    sb = lp.buffers_with_scene(rd, dev, scene)
    first, _ = c.run(3, sb=sb)
    check_radiance(first, c.want(3)[0], "before the rewrite")
    sp["lights"][1]["direction"] = (0.5, -0.6, 0.2, 0.0)
    sp["lights"][1]["color"] = (4.0, 0.25, 1.0, 1.0)
    rd.WriteBuffer(c.plt, scene, sp.nbytes, np.array(sp).reshape(1))
    second, _ = c.run(3, sb=sb)
    want, _, _ = sc.path_tracer_numpy(rd, dev, scene, 3, c.rays, c.keys["frameID"], c.keys["pixel"], DEPTH)
    check_radiance(second, want, "after the rewrite")
    assert not same(first, second)


# ---- 4. chunks and options ---------------------------------------------------------------------------------------------------------------
def test_chunks_and_options_do_not_matter(mods, cases):
    rd, _ = mods
    c = cases("c2")
    rad, _ = c.run(3)
    check_radiance(rad, c.want(3)[0], "defaults")
    _, lives = c.want(3)
    settings = [("chunk_paths", 100)] + [("kernel", v) for v in (0, 1, 2, 3)] + [(o, v) for o in ("quad", "cull", "group_entry_items") for v in (0, 1)]
    try:
        for opt, value in settings:
            rd.SetOption(opt, value)
            got, invalid = c.run(3)
            st, counts = rd.GetTraceStats(), rd.GetBounceCounts(DEPTH + 2).copy()
            rd.SetOption(opt, DEFAULTS[opt])
            assert same(got, rad) and invalid == 0, "option %s = %d changes the result" % (opt, value)
            assert np.array_equal(counts, expected_counts(c.n, lives)), (opt, value)
            if opt == "chunk_paths":      # eleven chunks, the last partial: at least one closest-hit launch each
                assert st.rays_primary == c.n and st.launches_extend >= 11
    finally:
        for opt, value in DEFAULTS.items():
            rd.SetOption(opt, value)
    assert same(c.run(3)[0], rad)


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------------
def test_edges(mods, cases):
    """max_depth 0: zeros; max_depth 1: one bounce; n = 0 touches nothing; n = 65 inside a 1037-record output range at a non-zero
    offset leaves every other byte untouched"""
    rd, _ = mods
    c = cases("c1")
    plt = c.plt
    got, invalid = c.run(3, depth=0)
    assert got.shape == (c.n, 4) and not got.view(np.uint8).any() and invalid == 0
    assert not rd.GetBounceCounts(4).any()
    color, lives = c.want(3, depth=1)
    got, _ = c.run(3, depth=1)
    check_radiance(got, color, "depth 1")
    assert len(lives) == 1 and np.array_equal(rd.GetBounceCounts(3), [c.n, lives[0], 0])
    assert not same(got[:, :3], c.want(3)[0])
    bR, bK = sh.upload(rd, plt, c.rays), sh.upload(rd, plt, c.keys)
    out = rc.filled(rd, plt, 16 * c.n)
    ret, invalid = rd.TraceLightPaths(c.tlas, bR, bK, 0, DEPTH, 3, c.sb, radiance=out)
    assert ret is out and invalid == 0 and (rc.whole(rd, plt, out) == S).all()
    rd.TraceLightPaths(c.tlas, bR, bK, 0, DEPTH, 3, c.sb, radiance=out, rays_offset=32 * c.n, keys_offset=16 * c.n, radiance_offset=16 * c.n)
    assert (rc.whole(rd, plt, out) == S).all()
    n, first, at = 65, 200, 300
    rd.TraceLightPaths(c.tlas, bR, bK, n, DEPTH, 3, c.sb, radiance=out, rays_offset=32 * first, keys_offset=16 * first, radiance_offset=16 * at)
    w = rc.whole(rd, plt, out)
    check_radiance(w[16 * at:16 * (at + n)].view(F).reshape(n, 4), c.want(3)[0][first:first + n], "n = 65 at an offset")
    assert (w[:16 * at] == S).all() and (w[16 * (at + n):] == S).all(), "a byte outside the radiance range was written"


# ---- 6. fencing ------------------------------------------------------------------------------------------------------------------------
def test_scene_buffers_that_do_not_describe_the_scene_are_fenced(mods, cases):
    """a material buffer that holds fewer Materials than the scene uses: the hits whose Material lies past it are misses, counted as
    rd.ResolveMaterials counts them over the bounces of the loop on the same buffers; a path whose first hit is one of them shows
    the miss colour; the call succeeds"""
    rd, _ = mods
    c = cases("c1")
    dev = c.dev
    nmat = dev.materialData.size // 48
    keep = nmat // 2
    assert keep >= 1
    short = rd.WrapDeviceMemory(c.plt, dev.materialData.device_ptr, 48 * keep, keepalive=dev.materialData)
    sb = lp.buffers_with_scene(rd, dev, c.scene, material=short)
    # the loop variant of light_paths_cases is the README's loop: on the scene's own buffers it has path_tracer_numpy's bits
    color, lives, invalid, _ = lp.public_loop(rd, c.plt, c.tlas, c.sb, dev.surface_buffers(), 3, c.rays, c.keys["frameID"], c.keys["pixel"], DEPTH)
    assert invalid == 0 and same(color, c.want(3)[0]) and lives == c.want(3)[1]
    color, lives, invalid, first_invalid = lp.public_loop(rd, c.plt, c.tlas, sb, dev.surface_buffers(), 3, c.rays, c.keys["frameID"], c.keys["pixel"], DEPTH)
    print("fencing: %d of %d Materials kept, invalid %d, first hit invalid on %d paths, lives %s" % (keep, nmat, invalid, int(first_invalid.sum()), lives))
    assert invalid >= 20 and first_invalid.sum() >= 20 and lives[0] >= 100
    got, got_invalid = c.run(3, sb=sb)
    check_radiance(got, color, "short material buffer")
    assert got_invalid == invalid
    assert (sh.bits(got[first_invalid, :3]) == sh.bits(sh.ENVIRONMENT)).all()
    assert np.array_equal(rd.GetBounceCounts(DEPTH + 2), expected_counts(c.n, lives))
    assert not same(got[:, :3], c.want(3)[0])


# ---- 7. stats --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light_count", (0, 3))
def test_stats(mods, cases, light_count):
    rd, _ = mods
    c = cases("c2")
    _, lives = c.want(light_count)
    rd.SetProfiling(True)
    try:
        c.run(light_count)
        st = rd.GetTraceStats()
    finally:
        rd.SetProfiling(False)
    assert st.pixels == c.n and st.rays_primary == c.n
    assert st.rays_bounce == sum(lives[:DEPTH - 1]) and st.rays_bounce > 0
    assert st.closest_hits == sum(lives) and st.rays_shadow == light_count * st.closest_hits
    assert st.launches_extend == len(lives) and st.launches_shadow == (sum(1 for v in lives if v) if light_count else 0)
    assert st.ms_total > 0 and st.ms_extend > 0 and st.ms_shade > 0 and (st.ms_shadow > 0) == (light_count > 0)
    assert st.ms_generate == 0 and st.ms_accumulate == 0


# ---- 8. torch tensors ------------------------------------------------------------------------------------------------------------------
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
import light_paths_cases as lp
import shade_cases as sh
c = sh.Golden(rd, scenes, "c0")
dev, plt, tlas = c.dev, c.dev.plt, c.dev.topAccelStruct
sb = lp.buffers_with_scene(rd, dev, lp.scene_buffer(rd, plt, lp.five_lights(rd)))
cam = dev.frame_buffers()[0]
npix = dev.width * dev.height
depth = 3
rays, keys = rd.GenerateRaysTorch(cam, npix, 5, 4)
rays = (rays * torch.tensor([1, 1, 1, 1, 2.5, 2.5, 2.5, 1], device="cuda")).contiguous()       # a tensor a torch op produced: non-unit directions
rn = rays.cpu().numpy().view(rd.RAY_DTYPE).reshape(-1)
kn = keys.cpu().numpy().view(rd.SHADE_KEY_DTYPE).reshape(-1)
for L in (0, 3):
    want, invalid = lp.trace(rd, plt, tlas, sb, rn, kn, depth, L)
    got = rd.TraceLightPathsTorch(tlas, rays, keys, depth, L, sb)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == (npix, 4) and got.is_cuda
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)) and invalid == 0 and want[:, :3].any()
empty = rd.TraceLightPathsTorch(tlas, rays[:0], keys[:0], depth, 3, sb)
assert tuple(empty.shape) == (0, 4)
wide = torch.zeros((npix, 16), dtype=torch.float32, device="cuda")
bad = [dict(rays=rays[:, :7]), dict(rays=rays.double()), dict(rays=rays.cpu()), dict(rays=wide[:, ::2]), dict(rays=rn), dict(keys=keys.long()),
       dict(keys=keys[:, :3]), dict(keys=keys[:-1]), dict(keys=keys.cpu()), dict(keys=keys.float()), dict(max_depth=-1), dict(max_depth=2.0), dict(sb=(1, 2)),
       dict(L=-1), dict(L=6), dict(L=2.5), dict(L="3")]
for j, kw in enumerate(bad):
    a = dict(rays=rays, keys=keys, max_depth=depth, L=3, sb=sb)
    a.update(kw)
    for fn, name in ((rd.TraceLightPathsTorch, "TraceLightPathsTorch"), (rd.TracePathsTorch, "TracePathsTorch")):
        if name == "TracePathsTorch" and "L" in kw:
            continue
        args = (tlas, a["rays"], a["keys"], a["max_depth"]) + ((a["L"],) if name == "TraceLightPathsTorch" else ()) + (a["sb"],)
        try:
            fn(*args)
        except rd.RadianceError as e:
            assert name[:-5] in str(e), (name, str(e))
            continue
        raise AssertionError("%s: bad argument set %d was accepted" % (name, j))
print("TORCH-LIGHT-PATHS-OK", npix)
"""


def test_torch_tensors_in_a_fresh_process(gpu):
    """rd.TraceLightPathsTorch equals rd.TraceLightPaths on the same inputs bit for bit; a non-contiguous tensor, a wrong dtype, shape
    or device is refused in Python exactly where rd.TracePathsTorch refuses it.  torch is initialised first, in a process of its own
    (as tests/test_gpu_paths.py does)"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _TORCH_CHILD, ROOT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "TORCH-LIGHT-PATHS-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(mods, cases):
    """every refusal of include/rdx.h returns an error that names the call, and leaves the sentinel-filled output as it was"""
    rd, _ = mods
    c = cases("c1")
    dev, plt, tl = c.dev, c.plt, c.tlas
    n, tail = 200, 128
    bR, bK = sh.upload(rd, plt, c.rays[:n], tail), sh.upload(rd, plt, c.keys[:n], tail)
    oR = rc.filled(rd, plt, 16 * n + tail)
    one = rc.filled(rd, plt, 32 * n * 4)            # rays | keys | room for the output, for the overlap cases
    rd.WriteBuffer(plt, one, 32 * n, c.rays[:n])
    rd.WriteBuffer(plt, one, 16 * n, c.keys[:n], offset=32 * n)
    big_scene = rc.filled(rd, plt, 176 + 16 * n)    # a SceneProperties followed by room for the output
    rd.WriteBuffer(plt, big_scene, 176, np.array(c.sp).reshape(1))
    null, unknown = rd.Buffer(None, 1 << 20), rd.Buffer(12345678, 1 << 20)
    outs = dict(radiance=oR, one=one)
    snapshot = lambda: {k: rc.whole(rd, plt, v) for k, v in outs.items()}
    good = snapshot()
    SB = lambda **kw: rd.ShadingBuffers(**{**dict(scene=c.scene, meshInfo=dev.meshInfoData, index=dev.indexData, uv=dev.uvData, normal=dev.normalData,
                                                 material=dev.materialData), **kw})

    def run(**kw):
        a = dict(tlas=tl, rays=bR, keys=bK, n=n, max_depth=DEPTH, light_count=3, scene_buffers=c.sb, radiance=oR)
        a.update(kw)
        return rd.TraceLightPaths(a.pop("tlas"), a.pop("rays"), a.pop("keys"), a.pop("n"), a.pop("max_depth"), a.pop("light_count"), a.pop("scene_buffers"), **a)

    wrapped = lambda buf, shift, size: rd.WrapDeviceMemory(plt, buf.device_ptr + shift, size, keepalive=buf)
    in_one = dict(rays=one, rays_offset=0, keys=one, keys_offset=32 * n)
    cases_ = [
        ("null tlas", dict(tlas=null), "TLAS"), ("unknown tlas", dict(tlas=unknown), "TLAS"),
        ("null rays", dict(rays=null), "ray buffer handle"), ("unknown rays", dict(rays=unknown), "ray buffer handle"),
        ("null keys", dict(keys=null), "key buffer handle"), ("unknown keys", dict(keys=unknown), "key buffer handle"),
        ("null radiance", dict(radiance=null), "radiance buffer handle"), ("unknown radiance", dict(radiance=unknown), "radiance buffer handle"),
        ("null scene", dict(scene_buffers=SB(scene=null)), "SceneProperties"), ("null meshInfo", dict(scene_buffers=SB(meshInfo=null)), "meshInfo"),
        ("null index", dict(scene_buffers=SB(index=null)), "index"), ("null normal", dict(scene_buffers=SB(normal=null)), "normal"),
        ("null material", dict(scene_buffers=SB(material=null)), "material"),
        ("unknown uv", dict(scene_buffers=SB(uv=rd.Buffer(12345678, 64))), "uv"),
        ("unknown textureArray", dict(scene_buffers=SB(textureArray=rd.Buffer(12345678, 64))), "textureArray"),
        ("a scene buffer smaller than SceneProperties", dict(scene_buffers=SB(scene=rd.CreateBuffer(plt, 160))), "SceneProperties"),
        ("max_depth 63", dict(max_depth=63), "63"), ("max_depth 2^31", dict(max_depth=1 << 31), "62"),
        ("rays_offset 8", dict(rays_offset=8), "16"), ("keys_offset 4", dict(keys_offset=4), "16"), ("radiance_offset 8", dict(radiance_offset=8), "16"),
        ("rays past the end", dict(rays_offset=tail + 16), "ray buffer"), ("keys past the end", dict(keys_offset=tail + 16), "key buffer"),
        ("radiance past the end", dict(radiance_offset=tail + 16), "radiance buffer"),
        ("radiance one record short", dict(radiance=rd.CreateBuffer(plt, 16 * n - 16)), "radiance buffer"),
        ("an offset beyond the buffer", dict(keys_offset=1 << 30), "key buffer"),
        ("radiance over the rays' tail", dict(in_one, radiance=one, radiance_offset=32 * n - 16), "overlap"),
        ("radiance over the keys", dict(in_one, radiance=one, radiance_offset=32 * n), "overlap"),
        ("radiance wraps the rays' memory", dict(radiance=wrapped(bR, 0, 16 * n)), "overlap"),
        ("radiance over the SceneProperties", dict(scene_buffers=SB(scene=big_scene), radiance=big_scene, radiance_offset=160), "overlap"),
        ("radiance = the SceneProperties", dict(scene_buffers=SB(scene=big_scene), radiance=big_scene, radiance_offset=0), "overlap"),
        ("misaligned wrapped rays", dict(rays=wrapped(bR, 8, 32 * n + 64)), "aligned"),
        ("misaligned wrapped keys", dict(keys=wrapped(bK, 4, 16 * n + 64)), "aligned"),
        ("misaligned wrapped radiance", dict(radiance=wrapped(oR, 8, 16 * n + 64)), "aligned"),
        ("misaligned wrapped index stream", dict(scene_buffers=SB(index=wrapped(dev.indexData, 2, dev.indexData.size - 2))), "aligned"),
    ]
    scene_good = rc.whole(rd, plt, big_scene)
    for what, kw, word in cases_:
        with pytest.raises(rd.RadianceError) as e:
            run(**kw)
        assert word in str(e.value) and "rdx_trace_paths_lights" in str(e.value), (what, str(e.value))
        now = snapshot()
        for k in outs:
            assert np.array_equal(now[k], good[k]), (what, k)
    assert np.array_equal(rc.whole(rd, plt, big_scene), scene_good)
    from radiance_ray_tracing_amd import _lib
    L = _lib.lib()
    invalid = C.c_uint32(7)
    st = c.sb._struct()
    assert L.rdx_trace_paths_lights(tl.handle, bR.handle, 0, bK.handle, 0, n, DEPTH, 6, C.byref(st), oR.handle, 0, C.byref(invalid)) != 0
    assert "light_count" in _lib.last_error() and "rdx_trace_paths_lights" in _lib.last_error()
    assert L.rdx_trace_paths_lights(tl.handle, bR.handle, 0, bK.handle, 0, n, DEPTH, 0xffffffff, C.byref(st), oR.handle, 0, None) != 0
    assert "light_count" in _lib.last_error()
    assert L.rdx_trace_paths_lights(tl.handle, bR.handle, 0, bK.handle, 0, n, DEPTH, 3, None, oR.handle, 0, None) != 0
    assert "scene" in _lib.last_error() and "rdx_trace_paths_lights" in _lib.last_error()
    unknown_sampler = _lib.rdx_shading_buffers(c.scene.handle, dev.meshInfoData.handle, dev.indexData.handle, None, dev.normalData.handle,
                                              dev.materialData.handle, None, 12345678)
    assert L.rdx_trace_paths_lights(tl.handle, bR.handle, 0, bK.handle, 0, n, DEPTH, 3, C.byref(unknown_sampler), oR.handle, 0, None) != 0
    assert "sampler" in _lib.last_error() and "rdx_trace_paths_lights" in _lib.last_error()
    assert all(np.array_equal(v, good[k]) for k, v in snapshot().items())
    # the SceneProperties may sit beside the output in one buffer; adjacent ranges are fine, and the call still works after the refusals
    run(scene_buffers=SB(scene=big_scene), radiance=big_scene, radiance_offset=176)
    check_radiance(rd.ReadBuffer(plt, big_scene, 16 * n, offset=176).view(F).reshape(n, 4), c.want(3)[0][:n], "output behind the SceneProperties")
    run(**in_one, radiance=one, radiance_offset=48 * n)
    check_radiance(rd.ReadBuffer(plt, one, 16 * n, offset=48 * n).view(F).reshape(n, 4), c.want(3)[0][:n], "adjacent ranges")
    assert (rd.ReadBuffer(plt, one, 64 * n, offset=64 * n) == S).all()

"""GPU suite (-m gpu): rdx_denoise through radiance_ray_tracing_amd.denoise -- the edge-avoiding a-trous filter over a frame's colours,
guided by the primary hits' material and surface records.

The reference has no denoiser.  The comparand is denoise_cases.denoise_reference, the numpy restatement that takes one IEEE float32
operation at a time; every bar is equality of bits with it (a NaN compares as a NaN: IEEE 754 leaves the payload of a NaN an
operation produces to the implementation -- denoise_cases.canon), for the LDS-tiled form of the pass that steps 1 and 2 take and for
the direct one alike (rdx_debug_denoise_tiled chooses; 3 is the library's default).
The RGBA8 image is held to rd.Accumulate, byte for byte.  The quality test is a condition on the defaults, not a measurement."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_cases as dc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
OFF = dict(color=48, mat=64, surf=16, work=80, out=32, image=12)
TAIL = 80
DEPTH = 4


@pytest.fixture(scope="module")
def mods(gpu):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import _lib, denoise, rd, scenes
    yield rd, scenes, denoise, _lib
    _lib.lib().rdx_debug_denoise_tiled(3)       # the library's default


class Frame:
    """the six ranges of one call at non-zero offsets in buffers filled with 0xA5"""

    def __init__(self, rd, plt, W, H):
        self.rd, self.plt, self.W, self.H, n = rd, plt, W, H, W * H
        self.size = dict(color=16 * n, mat=64 * n, surf=64 * n, work=48 * n, out=16 * n, image=4 * n)
        self.B = {k: rd.CreateBuffer(plt, OFF[k] + self.size[k] + TAIL) for k in OFF}
        for k in self.B:
            self.fill(k)

    def fill(self, k):
        self.rd.WriteBuffer(self.plt, self.B[k], self.B[k].size, np.full(self.B[k].size, 0xA5, np.uint8))

    def load(self, color, mat, surf):
        for k, arr in (("color", color), ("mat", mat), ("surf", surf)):
            if self.size[k]:
                self.rd.WriteBuffer(self.plt, self.B[k], self.size[k], np.ascontiguousarray(arr), offset=OFF[k])
        self.inputs = {k: self.whole(k) for k in ("color", "mat", "surf")}

    def whole(self, k):
        return self.rd.ReadBuffer(self.plt, self.B[k], self.B[k].size).copy()

    def arguments(self, with_image=True, **kw):
        a = dict(color=self.B["color"], materials=self.B["mat"], surfaces=self.B["surf"], width=self.W, height=self.H, out=self.B["out"],
                 image=self.B["image"] if with_image else None, work=self.B["work"], color_offset=OFF["color"], materials_offset=OFF["mat"], surfaces_offset=OFF["surf"],
                 out_offset=OFF["out"], image_offset=OFF["image"], work_offset=OFF["work"])
        a.update(kw)
        return a

    def run(self, dn, settings, image=True, refill=True):
        """-> (out (n, 4) float32, image (n, 4) uint8 or None); nothing outside the three written ranges has changed"""
        if refill:
            for k in ("work", "out", "image"):
                self.fill(k)
        a = self.arguments(image)
        assert dn.Denoise(a.pop("color"), a.pop("materials"), a.pop("surfaces"), a.pop("width"), a.pop("height"), settings, **a) is self.B["out"]
        for k in ("color", "mat", "surf"):
            assert np.array_equal(self.whole(k), self.inputs[k]), k
        got = {}
        for k in ("work", "out", "image"):
            raw = self.whole(k)
            lo, hi = OFF[k], OFF[k] + self.size[k]
            assert (raw[:lo] == 0xA5).all() and (raw[hi:] == 0xA5).all(), k
            got[k] = raw[lo:hi]
        if not image:
            assert (got["image"] == 0xA5).all()
        return got["out"].view(F).reshape(-1, 4), got["image"].reshape(-1, 4) if image else None


def show(got, want, W):
    bad = np.flatnonzero((dc.canon(got) != dc.canon(want)).any(1))
    return [(int(p % W), int(p // W), got[p].tolist(), want[p].tolist()) for p in bad[:4]], int(bad.size)


# ---- 1. synthetic records ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", dc.GPU_SIZES, ids=lambda s: "%dx%d" % s)
def test_synthetic_records_have_the_restatements_bits(mods, gpu, size):
    """every size around the 64 x 4 block and the tile halos, 0 .. 8 passes (steps 8 and up leave every tap outside the small images),
    every term off, each alone and all of them, on records a caller may have filled with anything -- by the direct form and by
    the tiled one"""
    rd, _, dn, _lib = mods
    W, H = size
    color, mat, surf = dc.hostile(W, H, 100 + W)
    if W * H >= 37 * 19:
        valid = dc.validity(mat, surf)
        assert valid.sum() > W * H // 2 and (mat["hit"] == 2).any() and (surf["hit"] == 2).any() and np.isnan(color[valid, :3]).any() and np.isinf(color[valid, :3]).any()
    fr = Frame(rd, gpu, W, H)
    fr.load(color, mat, surf)
    moved = 0
    for passes in dc.GPU_PASSES:
        for name, terms in dc.GPU_TERMS:
            st = dn.DenoiseSettings(passes=passes, **terms)
            want = dc.denoise_reference(color, mat, surf, W, H, st)
            assert np.array_equal(dc.bits(want[:, 3]), dc.bits(color[:, 3]))
            moved += int(not dc.same(want, color))
            for tiled in ((3, 0) if passes else (3,)):
                _lib.lib().rdx_debug_denoise_tiled(tiled)
                got, _ = fr.run(dn, st, image=False)
                assert dc.same(got, want), (size, passes, name, tiled, show(got, want, W))
                assert np.array_equal(dc.bits(got[:, 3]), dc.bits(color[:, 3])), "w keeps its bits"
                invalid = ~dc.validity(mat, surf)
                assert np.array_equal(dc.bits(got[invalid]), dc.bits(color[invalid])), "an invalid pixel keeps its bits"
            _lib.lib().rdx_debug_denoise_tiled(3)
    assert moved >= (20 if W * H > 15 else 0), moved
    assert rd.GetTraceStats().ms_accumulate > 0.0


# ---- 2. real records ---------------------------------------------------------------------------------------------------------------------
def scene_diagonal(rd, dev):
    blob = rd.ReadBuffer(dev.plt, dev.topAccelStruct, dev.topAccelStruct.size).tobytes()
    s = rd.DebugAccelLayout(blob)[0]
    return float(np.linalg.norm(np.array(s["sceneHi"], np.float64) - np.array(s["sceneLo"], np.float64)))


def read(rd, plt, buf, n, dtype):
    """n records of a structured dtype; float4 records as an (n, 4) float32 array"""
    raw = rd.ReadBuffer(plt, buf, n * dtype.itemsize)
    return raw.view(F).reshape(n, 4).copy() if dtype.subdtype else raw.view(dtype).reshape(-1).copy()


class RealFrame:
    """a W x H frame of a stock scene through the public calls: GenerateRays -> QueryRays -> ResolveHits + ResolveMaterials ->
    TracePaths at depth 4; the buffers stay on the device, the records are downloaded once"""

    def __init__(self, rd, scenes, name, W, H):
        make = dict(c1=lambda: scenes.c1_cornell(W, H, spp=1, depth=DEPTH, sphere_subdiv=3), c2=lambda: scenes.c2_atrium(W, H, spp=1, depth=DEPTH, detail=0.2))[name]
        self.dev = dev = scenes.DeviceScene(make())
        self.rd, self.plt, self.W, self.H, self.n = rd, dev.plt, W, H, W * H
        self.tlas, self.sb, self.cam = dev.topAccelStruct, dev.shading_buffers(), dev.frame_buffers()[0]
        self.rays, self.keys = rd.GenerateRays(self.cam, self.n, 0, 0)
        hits = rd.QueryRays(self.tlas, self.rays, self.n, rd.QUERY_CLOSEST)
        self.bS, inv_s = rd.ResolveHits(self.tlas, self.rays, hits, self.n, dev.surface_buffers())
        self.bM, inv_m = rd.ResolveMaterials(self.tlas, self.rays, hits, self.n, self.sb)
        assert inv_s == 0 and inv_m == 0
        self.bC = rd.TracePaths(self.tlas, self.rays, self.keys, self.n, DEPTH, self.sb)
        self.mat, self.surf = read(rd, self.plt, self.bM, self.n, dc.MATERIAL_DTYPE), read(rd, self.plt, self.bS, self.n, dc.SURFACE_DTYPE)
        self.color = read(rd, self.plt, self.bC, self.n, np.dtype(("<f4", 4)))
        self.sigma = 0.01 * scene_diagonal(rd, dev)

    def sample(self, frame):
        """the colours of sample `frame` of every pixel, through the same calls"""
        rd = self.rd
        if not hasattr(self, "own"):
            self.own = [rd.CreateBuffer(self.plt, k * self.n) for k in (32, 16, 16)]
        rays, keys, radiance = self.own
        rd.GenerateRays(self.cam, self.n, frame, frame, rays=rays, keys=keys)
        return read(rd, self.plt, rd.TracePaths(self.tlas, rays, keys, self.n, DEPTH, self.sb, radiance=radiance), self.n, np.dtype(("<f4", 4)))


@pytest.fixture(scope="module")
def real(mods):
    rd, scenes, _, _ = mods
    cache = {}

    def get(name, W, H):
        if (name, W, H) not in cache:
            cache[(name, W, H)] = RealFrame(rd, scenes, name, W, H)
        return cache[(name, W, H)]
    return get


@pytest.mark.parametrize("name", ("c1", "c2"))
def test_real_records_have_the_restatements_bits(mods, real, name):
    """a 64 x 32 frame of a stock scene with every term on, sigma_position 1 % of the scene's diagonal; the primary misses of c2 pass
    through"""
    rd, _, dn, _lib = mods
    r = real(name, 64, 32)
    valid = dc.validity(r.mat, r.surf)
    assert np.array_equal(r.mat["hit"] == 1, r.surf["hit"] == 1) and valid.sum() >= r.n // 4
    if name == "c2":
        assert (~valid).sum() >= 16, "c2 has primary misses"
    st = dn.DenoiseSettings(sigma_position=r.sigma, sigma_colour=0.5)
    want = dc.denoise_reference(r.color, r.mat, r.surf, r.W, r.H, st)
    for tiled in (3, 0):
        _lib.lib().rdx_debug_denoise_tiled(tiled)
        got = read(rd, r.plt, dn.Denoise(r.bC, r.bM, r.bS, r.W, r.H, st), r.n, np.dtype(("<f4", 4)))
        assert dc.same(got, want), (name, tiled, show(got, want, r.W))
    _lib.lib().rdx_debug_denoise_tiled(3)
    assert np.array_equal(dc.bits(got[~valid]), dc.bits(r.color[~valid])) and not dc.same(got[valid], r.color[valid])
    assert np.array_equal(read(rd, r.plt, r.bC, r.n, np.dtype(("<f4", 4))).view(np.uint32), r.color.view(np.uint32)), "the colours are not written"


# ---- 3. the RGBA8 image ------------------------------------------------------------------------------------------------------------------
def test_the_image_is_accumulates(mods, gpu, real):
    """image = what rd.Accumulate writes for the denoised colours at frameID 0 into a fresh scratch, with and without the debug bit"""
    rd, _, dn, _ = mods
    r = real("c1", 64, 32)
    W, H = 65, 5
    color, mat, surf = dc.noisy_wall(W, H, 9)
    color[:, :3] *= F(3.0)           # above 1: the debug image wraps, the tone-mapped one saturates
    cases = [(W, H, color, mat, surf, dn.DenoiseSettings(passes=2)), (r.W, r.H, r.color, r.mat, r.surf, dn.DenoiseSettings(sigma_position=r.sigma)),
             (W, H, color, mat, surf, dn.DenoiseSettings(passes=0))]
    for w, h, c, m, s, st in cases:
        fr = Frame(rd, gpu, w, h)
        fr.load(c, m, s)
        images = []
        for debug in (False, True):
            st.debug = debug
            out, image = fr.run(dn, st, image=True)
            assert dc.same(out, dc.denoise_reference(c, m, s, w, h, st))
            n = w * h
            scratch, ref = rd.CreateBuffer(gpu, 16 * n), rd.CreateBuffer(gpu, 4 * n)
            assert rd.Accumulate(fr.B["out"], n, 0, scratch, ref, debug=debug, colors_offset=OFF["out"]) == 0
            want = rd.ReadBuffer(gpu, ref, 4 * n).reshape(n, 4)
            assert np.array_equal(image, want), (w, h, debug, np.flatnonzero((image != want).any(1))[:8])
            assert (image[:, 3] == 255).all()
            images.append(image)
        assert not np.array_equal(images[0], images[1])


# ---- 4. determinism and state ------------------------------------------------------------------------------------------------------------
def test_determinism_and_state(mods, gpu):
    rd, _, dn, _ = mods
    W, H = 130, 33
    color, mat, surf = dc.hostile(W, H, 41)
    fr = Frame(rd, gpu, W, H)
    fr.load(color, mat, surf)
    a, b = dn.DenoiseSettings(passes=3, sigma_position=0.08, sigma_colour=0.5), dn.DenoiseSettings(passes=2, normal_squarings=1, demodulate=False)
    first, _ = fr.run(dn, a)
    again, _ = fr.run(dn, a, refill=False)
    assert np.array_equal(dc.bits(first), dc.bits(again)), "two calls give equal bits"
    fresh, _ = fr.run(dn, b)                          # work, out and image refilled with 0xA5
    fr.run(dn, a)
    used, _ = fr.run(dn, b, refill=False)             # the work range the call with other settings left behind
    assert np.array_equal(dc.bits(used), dc.bits(fresh)), "nothing of an earlier call is read"
    # colours and records rewritten between two calls are seen by the second
    color2, mat2, surf2 = dc.hostile(W, H, 42)
    fr.load(color2, mat2, surf2)
    second, _ = fr.run(dn, a, refill=False)
    assert dc.same(second, dc.denoise_reference(color2, mat2, surf2, W, H, a)) and not dc.same(second, first)


# ---- 5. shapes and refusals --------------------------------------------------------------------------------------------------------------
def test_shapes_and_refusals(mods, gpu):
    rd, _, dn, _lib = mods
    L = _lib.lib()
    W, H = 37, 19
    n = W * H
    color, mat, surf = dc.hostile(W, H, 77)
    fr = Frame(rd, gpu, W, H)
    fr.load(color, mat, surf)
    st = dn.DenoiseSettings(passes=2)
    untouched = lambda: all((fr.whole(k) == 0xA5).all() for k in ("work", "out", "image")) and all(np.array_equal(fr.whole(k), fr.inputs[k]) for k in ("color", "mat", "surf"))

    def raw(settings="default", **kw):
        """the library itself: no wrapper decides anything"""
        a = fr.arguments(**kw)
        s = st._struct() if isinstance(settings, str) else settings
        h = lambda b: b.handle if b is not None else None
        return L.rdx_denoise(h(a["color"]), a["color_offset"], h(a["materials"]), a["materials_offset"], h(a["surfaces"]), a["surfaces_offset"], a["width"], a["height"],
                             C.byref(s) if s is not None else None, h(a["work"]), a["work_offset"], h(a["out"]), a["out_offset"], h(a["image"]), a["image_offset"])

    # a frame of no pixels succeeds and touches nothing, in the library and through the wrapper
    for w, h in ((0, H), (W, 0), (0, 0), (0, 100000)):
        assert raw(width=w, height=h) == 0, _lib.last_error()
        a = fr.arguments(width=w, height=h)
        dn.Denoise(a.pop("color"), a.pop("materials"), a.pop("surfaces"), a.pop("width"), a.pop("height"), st, **a)
    assert untouched()

    def settings(**kw):
        s = st._struct()
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    padded = st._struct()
    padded._0[1] = 1
    null, unknown = rd.Buffer(None, 1 << 20), rd.Buffer(12345678, 1 << 20)
    wrapped = lambda k, shift: rd.WrapDeviceMemory(gpu, fr.B[k].device_ptr + shift, fr.B[k].size - shift, keepalive=fr.B[k])
    cases = [
        ("a null colour", dict(color=null), "colour buffer handle"), ("an unknown material buffer", dict(materials=unknown), "material-record buffer handle"),
        ("a null surface buffer", dict(surfaces=null), "surface-record buffer handle"), ("a null work", dict(work=null), "work buffer handle"),
        ("a null out", dict(out=null), "output buffer handle"), ("an unknown image", dict(image=unknown), "image buffer handle"),
        ("no settings", dict(settings=None), "settings"), ("nine passes", dict(settings=settings(passes=9)), "passes"),
        ("eight squarings", dict(settings=settings(normal_squarings=8)), "normal_squarings"),
        ("a negative sigma_position", dict(settings=settings(sigma_position=-1.0)), "sigma_position"),
        ("an infinite sigma_position", dict(settings=settings(sigma_position=float("inf"))), "sigma_position"),
        ("a NaN sigma_colour", dict(settings=settings(sigma_colour=float("nan"))), "sigma_colour"),
        ("non-zero padding", dict(settings=padded), "padding"), ("an unknown flag", dict(settings=settings(flags=4)), "flags"),
        ("a width above the limit", dict(width=16385, height=1), "outside the supported"), ("too many pixels", dict(width=16384, height=4097), "outside the supported"),
        ("a colour offset off 16", dict(color_offset=OFF["color"] + 8), "16"), ("a material offset off 16", dict(materials_offset=OFF["mat"] + 4), "16"),
        ("a surface offset off 16", dict(surfaces_offset=OFF["surf"] + 8), "16"), ("a work offset off 16", dict(work_offset=OFF["work"] + 8), "16"),
        ("an out offset off 16", dict(out_offset=OFF["out"] + 4), "16"), ("an image offset off 4", dict(image_offset=OFF["image"] + 2), "4"),
        ("colours that overrun", dict(color_offset=OFF["color"] + TAIL + 16), "colour buffer"), ("materials that overrun", dict(materials_offset=OFF["mat"] + TAIL + 16), "material-record buffer"),
        ("surfaces that overrun", dict(surfaces_offset=OFF["surf"] + TAIL + 16), "surface-record buffer"), ("a work range that overruns", dict(work_offset=OFF["work"] + TAIL + 16), "work buffer"),
        ("an out that overruns", dict(out_offset=OFF["out"] + TAIL + 16), "output buffer"), ("an image that overruns", dict(image_offset=OFF["image"] + TAIL + 4), "image buffer"),
        ("a frame larger than the buffers", dict(height=2 * H), "buffer"),
        ("out over the colours", dict(out=fr.B["color"], out_offset=OFF["color"] + 16), "overlap"), ("work over the materials", dict(work=fr.B["mat"], work_offset=0), "overlap"),
        ("the image over the surfaces", dict(image=fr.B["surf"], image_offset=OFF["surf"] + 64), "overlap"),
        ("out over the work range", dict(out=fr.B["work"], out_offset=OFF["work"] + 32 * n), "overlap"),
        ("the image over out", dict(image=fr.B["out"], image_offset=OFF["out"]), "overlap"),
        ("misaligned wrapped colours", dict(color=wrapped("color", 8), color_offset=0), "aligned"), ("a misaligned wrapped out", dict(out=wrapped("out", 4), out_offset=0), "aligned"),
        ("a misaligned wrapped image", dict(image=wrapped("image", 2), image_offset=0), "aligned"),
    ]
    for what, kw, text in cases:
        kw = dict(kw)
        s = kw.pop("settings", "default")
        assert raw(settings=s, **kw) != 0, what
        err = _lib.last_error()
        assert "rdx_denoise" in err and text in err, (what, err)
        assert untouched(), what
    # the wrapper carries the library's refusals, and refuses what it can decide itself
    for kw in (dict(color=null), dict(out=fr.B["color"], out_offset=OFF["color"] + 16), dict(width=2 * W), dict(work=wrapped("work", 8), work_offset=0)):
        a = fr.arguments(**kw)
        with pytest.raises(rd.RadianceError, match="[Dd]enoise"):
            dn.Denoise(a.pop("color"), a.pop("materials"), a.pop("surfaces"), a.pop("width"), a.pop("height"), st, **a)
    assert untouched()
    got, _ = fr.run(dn, st)
    assert dc.same(got, dc.denoise_reference(color, mat, surf, W, H, st)), "after the refusals the call is what it was"
    # created outputs: out and work are the call's own when None
    out = dn.Denoise(fr.B["color"], fr.B["mat"], fr.B["surf"], W, H, st, color_offset=OFF["color"], materials_offset=OFF["mat"], surfaces_offset=OFF["surf"])
    assert out.size == 16 * n and dc.same(read(rd, gpu, out, n, np.dtype(("<f4", 4))), got)


# ---- 6. quality, as a condition ----------------------------------------------------------------------------------------------------------
def test_the_defaults_lower_the_error_of_a_sample(mods, real):
    """c1 at 64 x 64, DenoiseSettings(sigma_position = 1 % of the diagonal) and the other defaults: the mean squared error of the
    denoised sample of frame 0 against the mean of 256 samples, over the valid pixels, is strictly below that of the sample itself"""
    rd, _, dn, _ = mods
    r = real("c1", 64, 64)
    mean = np.zeros((r.n, 3), np.float64)
    for f in range(256):
        mean += r.sample(f)[:, :3]
    mean /= 256.0
    assert np.array_equal(r.sample(0).view(np.uint32), r.color.view(np.uint32)), "sample 0 is the frame's"
    st = dn.DenoiseSettings(sigma_position=r.sigma, sigma_colour=0.0)
    got = read(rd, r.plt, dn.Denoise(r.bC, r.bM, r.bS, r.W, r.H, st), r.n, np.dtype(("<f4", 4)))
    valid = dc.validity(r.mat, r.surf)
    mse = lambda a: float(((a[valid, :3].astype(np.float64) - mean[valid]) ** 2).mean())
    raw, den = mse(r.color), mse(got)
    print("mean squared error over %d valid pixels: sample %.6g, denoised %.6g (ratio %.3f)" % (int(valid.sum()), raw, den, den / raw))
    assert den < raw, (den, raw)


# ---- 7. torch tensors and the README's snippet -------------------------------------------------------------------------------------------
_TORCH_CHILD = r"""
import os, sys
ROOT = sys.argv[1]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
assert torch.cuda.is_available()
torch.zeros(1, device="cuda").cpu()                      # torch initialises the GPU first
import numpy as np
import rrt_amd
from radiance_ray_tracing_amd import denoise, rd, scenes
import denoise_cases as dc
width, height, max_depth = 64, 32, 4
dev = scenes.DeviceScene(scenes.c1_cornell(width, height, spp=1, depth=max_depth, sphere_subdiv=3))
tlas, sb, sf, cam = dev.topAccelStruct, dev.shading_buffers(), dev.surface_buffers(), dev.frame_buffers()[0]
blob = rd.ReadBuffer(dev.plt, tlas, tlas.size).tobytes()
s = rd.DebugAccelLayout(blob)[0]
scene_diagonal = float(np.linalg.norm(np.array(s["sceneHi"], np.float64) - np.array(s["sceneLo"], np.float64)))
# ---- the README's snippet
rays, keys = rd.GenerateRaysTorch(cam, width * height, 0, 0)
hits = rd.QueryRaysTorch(tlas, rays, rd.QUERY_CLOSEST)
surfaces, _ = rd.ResolveHitsTorch(tlas, rays, hits, sf)
materials, _ = rd.ResolveMaterialsTorch(tlas, rays, hits, sb)
radiance = rd.TracePathsTorch(tlas, rays, keys, max_depth, sb)
settings = denoise.DenoiseSettings(sigma_position=0.01 * scene_diagonal)
image = torch.empty((width * height, 4), dtype=torch.uint8, device="cuda")
filtered = denoise.DenoiseTorch(radiance, materials, surfaces, width, height, settings, image=image)
# ----
n = width * height
assert isinstance(filtered, torch.Tensor) and filtered.dtype == torch.float32 and tuple(filtered.shape) == (n, 4) and filtered.is_cuda
mat = materials.cpu().numpy().view(dc.MATERIAL_DTYPE).reshape(-1)
surf = surfaces.cpu().numpy().view(dc.SURFACE_DTYPE).reshape(-1)
want = dc.denoise_reference(radiance.cpu().numpy(), mat, surf, width, height, settings)
assert dc.same(filtered.cpu().numpy(), want) and not dc.same(want, radiance.cpu().numpy())
# the Buffer route on the same memory, and the image against rd.Accumulate
up = lambda t: rd.WrapDeviceMemory(None, t.data_ptr(), t.numel() * t.element_size(), keepalive=t)
out = denoise.Denoise(up(radiance), up(materials), up(surfaces), width, height, settings)
assert np.array_equal(rd.ReadBuffer(dev.plt, out, 16 * n).view(np.uint32), filtered.cpu().numpy().view(np.uint32).reshape(-1))
scratch, ref = torch.zeros((n, 4), device="cuda"), torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
assert rd.AccumulateTorch(filtered, 0, scratch, ref) == 0 and torch.equal(ref, image) and int(image[:, :3].max()) > 0
assert tuple(denoise.DenoiseTorch(radiance[:0], materials[:0], surfaces[:0], 0, 0, settings).shape) == (0, 4)
assert tuple(denoise.DenoiseTorch(radiance[:0], materials[:0], surfaces[:0], 0, 7, settings).shape) == (0, 4)
bad = [lambda: denoise.DenoiseTorch(radiance, materials, surfaces, width, height + 1, settings), lambda: denoise.DenoiseTorch(radiance.double(), materials, surfaces, width, height, settings),
       lambda: denoise.DenoiseTorch(radiance, materials[:-1], surfaces, width, height, settings), lambda: denoise.DenoiseTorch(radiance, materials, surfaces[:, :8], width, height, settings),
       lambda: denoise.DenoiseTorch(radiance, materials.cpu(), surfaces, width, height, settings), lambda: denoise.DenoiseTorch(radiance, materials, surfaces, width, height, None),
       lambda: denoise.DenoiseTorch(radiance, materials, surfaces, width, height, settings, image=image[:-1]),
       lambda: denoise.DenoiseTorch(radiance, materials, surfaces, width, height, settings, image=image.float()),
       lambda: denoise.DenoiseTorch(radiance, materials, surfaces, 2.5, height, settings)]
for j, fn in enumerate(bad):
    try:
        fn()
    except rd.RadianceError:
        continue
    raise AssertionError("bad argument set %d was accepted" % j)
print("TORCH-DENOISE-OK", n)
"""


def test_torch_tensors_and_the_readme_snippet_in_a_fresh_process(gpu):
    """the torch route equals the restatement and the Buffer route bit for bit, through the README's snippet; a wrong dtype, shape or
    device is refused in Python.  torch is initialised first, in a process of its own (as tests/test_gpu_env.py)"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _TORCH_CHILD, ROOT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "TORCH-DENOISE-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])

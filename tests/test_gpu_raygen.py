"""GPU suite (-m gpu): rd.GenerateRays / rd.Accumulate and their torch routes (rdx_generate_rays, rdx_accumulate) -- the two ends
of a frame on device memory.

Comparands, in this order of authority:
  1. the reference's own device code, recorded (tests/golden/refgpu_c{0,1,2}.npz): its generateRay on gen_rnd (gen_o / gen_d, and
     lens_o / lens_d of c1 with fStop 2.8), and its two progressive frames scratch0 / image0, scratch1 / image1;
  2. the library's own seams and frame path, which the existing suite holds to those recordings: rd.GenerateBatch, TraceRays;
  3. the numpy restatement of the running mean (raygen_cases.running_mean), which tests/test_raygen_cpu.py holds to the CPU oracle.
Every bar is equality of bits.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_cases as gc
import raygen_cases as rc
import shade_cases as sh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U4 = np.float32, np.dtype("<u4")
S = rc.SENTINEL


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


def check_rays(rays, o, d, tmin=0.001, tmax=1000.0, tag=""):
    for name, got, want in (("origin", rays["origin"], o), ("direction", rays["direction"], d)):
        eq = (sh.bits(got) == sh.bits(want)).all(1)
        assert eq.all(), "%s: %s differs on %d of %d rays" % (tag, name, int((~eq).sum()), eq.shape[0])
    assert (sh.bits(rays["tmin"]) == sh.bits(F(tmin))).all() and (sh.bits(rays["tmax"]) == sh.bits(F(tmax))).all(), tag


def check_keys(keys, frame, pixels, tag=""):
    assert (keys["frameID"] == frame).all() and np.array_equal(keys["pixel"], np.asarray(pixels, np.uint32)), tag
    assert not keys["depth"].any() and not keys["_0"].any(), tag


# ---- 1. recorded rays ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.SCENES)
def test_recorded_rays(mods, golden, name):
    """seeds = the recorded random inputs over all pixels: origin and direction have the bits the reference's generateRay gave;
    tmin / tmax carry the bits passed in; the keys are (frameID, pixel, 0, 0).  c1 also through the thin lens"""
    rd, scenes = mods
    c = golden(name)
    npix = c.s.width * c.s.height
    cases = [(c.dev, c.G["gen_o"], c.G["gen_d"], "pinhole")]
    if name == "c1":
        cases.append((scenes.DeviceScene(gc.small_scene(scenes, name, fstop=2.8)), c.G["lens_o"], c.G["lens_d"], "thin lens"))
    for dev, o, d, tag in cases:
        plt = dev.plt
        seeds = sh.upload(rd, plt, rc.seeds_of(c.G["gen_rnd"]))
        rays, keys = rd.GenerateRays(dev.frame_buffers()[0], npix, 3, 1, seeds=seeds, tmin=0.25, tmax=77.5)
        check_rays(sh.read(rd, plt, rays, npix, rd.RAY_DTYPE), o, d, 0.25, 77.5, "%s %s" % (name, tag))
        check_keys(sh.read(rd, plt, keys, npix, rd.SHADE_KEY_DTYPE), 3, np.arange(npix), tag)
        rays, keys = rd.GenerateRays(dev.frame_buffers()[0], npix, 0, 0, seeds=seeds, keys=None)       # the reference's interval by default
        assert keys is None
        check_rays(sh.read(rd, plt, rays, npix, rd.RAY_DTYPE), o, d, tag="%s %s, default interval" % (name, tag))
    if name == "c1":
        assert not same(c.G["gen_o"], c.G["lens_o"])


# ---- 2. derived seeds and pixel selection -------------------------------------------------------------------------------------------
def test_derived_seeds_and_pixel_selection(mods, golden):
    """without seeds the random input is pcg3d(frameID, totalSamples, pixel): the rays equal rd.GenerateBatch on those inputs, for
    ranges of every size around a wave, from pixel 0 and from 700, for a shuffled pixel list, and at offsets into larger buffers"""
    rd, _ = mods
    c = golden("c0")
    dev, plt = c.dev, c.dev.plt
    dev.bind()
    cam = dev.frame_buffers()[0]
    npix = dev.width * dev.height
    rng = np.random.default_rng(20261019)
    for frame, total in ((0, 0), (5, 4)):
        px = np.arange(npix + 700, dtype=np.uint32)
        wo, wd = rd.GenerateBatch(px, np.stack([np.full_like(px, frame), np.full_like(px, total), px], 1))
        for first in (0, 700):
            for n in (1, 63, 64, 65, npix):
                tag = "frame %d total %d first %d n %d" % (frame, total, first, n)
                rays, keys = rd.GenerateRays(cam, n, frame, total, first_pixel=first)
                check_rays(sh.read(rd, plt, rays, n, rd.RAY_DTYPE), wo[first:first + n], wd[first:first + n], tag=tag)
                check_keys(sh.read(rd, plt, keys, n, rd.SHADE_KEY_DTYPE), frame, px[first:first + n], tag)
        # a shuffled list, read at an offset that is a multiple of 4 only; rays and keys at offsets of their own, slack all round
        n = 1000
        sel = rng.permutation(npix + 700)[:n].astype(np.uint32)
        po, ro, ko, tail = 20, 96, 48, 80
        bP = rc.filled(rd, plt, po + 4 * n + tail)
        rd.WriteBuffer(plt, bP, 4 * n, sel, offset=po)
        bR, bK = rc.filled(rd, plt, ro + 32 * n + tail), rc.filled(rd, plt, ko + 16 * n + tail)
        before = rc.whole(rd, plt, bP)
        ret = rd.GenerateRays(cam, n, frame, total, first_pixel=123, pixels=bP, rays=bR, keys=bK, pixels_offset=po, rays_offset=ro, keys_offset=ko)
        assert ret[0] is bR and ret[1] is bK
        r, k = rc.whole(rd, plt, bR), rc.whole(rd, plt, bK)
        check_rays(r[ro:ro + 32 * n].view(rd.RAY_DTYPE), wo[sel], wd[sel], tag="shuffled")
        check_keys(k[ko:ko + 16 * n].view(rd.SHADE_KEY_DTYPE), frame, sel, "shuffled")
        assert (r[:ro] == S).all() and (r[ro + 32 * n:] == S).all() and (k[:ko] == S).all() and (k[ko + 16 * n:] == S).all()
        assert np.array_equal(rc.whole(rd, plt, bP), before)
        # seeds at an offset: the pixel list still names the pixel, the seed record the random input
        so = 32
        seeds = rc.seeds_of(np.stack([np.full(n, frame, np.uint32), np.full(n, total, np.uint32), sel[::-1]], 1))
        bS = rc.filled(rd, plt, so + 16 * n + tail)
        rd.WriteBuffer(plt, bS, 16 * n, seeds, offset=so)
        mo, md = rd.GenerateBatch(sel, seeds["in"])
        rays, _ = rd.GenerateRays(cam, n, frame, total, pixels=bP, seeds=bS, pixels_offset=po, seeds_offset=so, keys=False)
        check_rays(sh.read(rd, plt, rays, n, rd.RAY_DTYPE), mo, md, tag="pixels and seeds")
        assert not same(md, wd[sel])


# ---- 3. the camera is read by every call --------------------------------------------------------------------------------------------
def test_camera_changes_are_seen(mods, golden):
    """another rotation and fStop written into the same camera buffer: the next call equals GenerateBatch with that camera bound"""
    rd, _ = mods
    c = golden("c1")
    dev, plt = c.dev, c.dev.plt
    dev.bind()
    cam = dev.frame_buffers()[0]
    npix = dev.width * dev.height
    px = np.arange(npix, dtype=np.uint32)
    rnd = np.stack([np.full_like(px, 2), np.full_like(px, 2), px], 1)
    first = sh.read(rd, plt, rd.GenerateRays(cam, npix, 2, 2)[0], npix, rd.RAY_DTYPE)
    check_rays(first, *rd.GenerateBatch(px, rnd), tag="the scene's camera")
    old = np.array(c.s.camera).copy()
    try:
        for wx, wy, wz, fstop in ((-1.1, 2.9, 0.3, 2.8), (0.4, -0.7, 1.9, 0.0)):
            new = old.copy()
            new["wx"], new["wy"], new["wz"], new["fStop"] = wx, wy, wz, fstop
            rd.WriteBuffer(plt, cam, 48, new)
            got = sh.read(rd, plt, rd.GenerateRays(cam, npix, 2, 2)[0], npix, rd.RAY_DTYPE)
            check_rays(got, *rd.GenerateBatch(px, rnd), tag="camera %r" % ((wx, wy, wz, fstop),))
            assert not same(got["direction"], first["direction"])
            assert same(got["origin"], first["origin"]) == (fstop == 0.0)
    finally:
        rd.WriteBuffer(plt, cam, 48, old)
    check_rays(sh.read(rd, plt, rd.GenerateRays(cam, npix, 2, 2)[0], npix, rd.RAY_DTYPE), first["origin"], first["direction"], tag="restored")


# ---- 4. accumulate alone ------------------------------------------------------------------------------------------------------------
class Frame:
    """a frame of npix pixels in the MIDDLE of two sentinel-filled allocations: scratch / image wrap the middle, the slack on
    either side lies outside them"""
    LEAD, TAIL = 256, 512

    def __init__(self, rd, plt, npix, image_pixels=None):
        self.rd, self.plt, self.npix = rd, plt, npix
        self.nimg = npix if image_pixels is None else image_pixels
        self.allS = rc.filled(rd, plt, self.LEAD + 16 * npix + self.TAIL)
        self.allI = rc.filled(rd, plt, self.LEAD + 4 * self.nimg + self.TAIL)
        self.scratch = rd.WrapDeviceMemory(plt, self.allS.device_ptr + self.LEAD, 16 * npix, keepalive=self.allS)
        self.image = rd.WrapDeviceMemory(plt, self.allI.device_ptr + self.LEAD, 4 * self.nimg, keepalive=self.allI)

    def set_scratch(self, a):
        self.rd.WriteBuffer(self.plt, self.allS, 16 * self.npix, np.ascontiguousarray(a, F), offset=self.LEAD)

    def read(self):
        s, i = rc.whole(self.rd, self.plt, self.allS), rc.whole(self.rd, self.plt, self.allI)
        for a, n in ((s, 16 * self.npix), (i, 4 * self.nimg)):
            assert (a[:self.LEAD] == S).all() and (a[self.LEAD + n:] == S).all(), "a byte outside the frame was written"
        return s[self.LEAD:self.LEAD + 16 * self.npix].view(F).reshape(-1, 4).copy(), i[self.LEAD:self.LEAD + 4 * self.nimg].reshape(-1, 4).copy()


def _colors(rng, n):
    """negatives, zeros, values above 1, tiny and large magnitudes; w is junk"""
    c = rng.normal(0.5, 1.5, (n, 4)).astype(F)
    c[rng.integers(0, n, n // 8), rng.integers(0, 3, n // 8)] = 0.0
    c[rng.integers(0, n, n // 8)] *= F(1e-6)
    c[rng.integers(0, n, n // 8)] *= F(300.0)
    c[:, 3] = rng.normal(size=n).astype(F)
    return c


def test_accumulate_alone(mods):
    rd, _ = mods
    plt = rd.Platform.GetPlatform()
    rng = np.random.default_rng(1019)
    npix = 1000                                     # four blocks, the last one partial, its last wave partial
    fr = Frame(rd, plt, npix)
    start = rng.normal(size=(npix, 4)).astype(F)
    fr.set_scratch(start)
    want = start.copy()
    untouched_image = np.full((npix, 4), S, np.uint8)
    # frameID 0 overwrites rgb and keeps w; without `image` the image is untouched
    c0 = _colors(rng, npix)
    assert rd.Accumulate(sh.upload(rd, plt, c0), npix, 0, fr.scratch) == 0
    rc.running_mean(want, c0, 0)
    got, img = fr.read()
    assert same(got, want) and same(got[:, 3], start[:, 3]) and same(got[:, :3], c0[:, :3]) and same(img, untouched_image)
    # later frames: the restated mean, on what the frame before left
    for frame in (1, 7):
        cf = _colors(rng, npix)
        assert rd.Accumulate(sh.upload(rd, plt, cf), npix, frame, fr.scratch) == 0
        rc.running_mean(want, cf, frame)
        got, img = fr.read()
        eq = (sh.bits(got) == sh.bits(want)).all(1)
        assert eq.all(), "frame %d: %d of %d pixels differ from the restated mean" % (frame, int((~eq).sum()), npix)
        assert same(img, untouched_image)
    # a range from first_pixel, colours read at an offset
    n, first, off = 130, 801, 48
    cf = _colors(rng, n)
    bC = rc.filled(rd, plt, off + 16 * n + 32)
    rd.WriteBuffer(plt, bC, 16 * n, cf, offset=off)
    assert rd.Accumulate(bC, n, 2, fr.scratch, first_pixel=first, colors_offset=off) == 0
    rc.running_mean(want, cf, 2, pixels=np.arange(first, first + n))
    assert same(fr.read()[0], want)
    # a shuffled subset: the pixels not named keep their value
    n = 333
    sel = rng.permutation(npix)[:n].astype(np.uint32)
    cf = _colors(rng, n)
    assert rd.Accumulate(sh.upload(rd, plt, cf), n, 3, fr.scratch, pixels=sh.upload(rd, plt, sel), first_pixel=55) == 0
    rc.running_mean(want, cf, 3, pixels=sel)
    got, img = fr.read()
    assert same(got, want) and same(img, untouched_image)
    # three pixel numbers at or past the end: counted, nothing written for them, the others done
    sel = np.array([3, npix, 999, npix + 5, 0xffffffff, 10], np.uint32)
    cf = _colors(rng, sel.shape[0])
    assert rd.Accumulate(sh.upload(rd, plt, cf), sel.shape[0], 4, fr.scratch, fr.image, pixels=sh.upload(rd, plt, sel)) == 3
    ok = sel < npix
    rc.running_mean(want, cf[ok], 4, pixels=sel[ok])
    got, img = fr.read()
    assert same(got, want)
    assert (img[sel[ok], 3] == 255).all() and same(np.delete(img, sel[ok], 0), np.delete(untouched_image, sel[ok], 0))
    assert rd.Accumulate(sh.upload(rd, plt, cf), sel.shape[0], 4, fr.scratch, fr.image, first_pixel=npix - 2) == 4      # a range that runs off the end
    rc.running_mean(want, cf[:2], 4, pixels=[npix - 2, npix - 1])
    assert same(fr.read()[0], want)
    # debug: (unsigned char)(int)(c * 255) of the mean, for means in [0, 1)
    unit = rng.uniform(0, 1, (npix, 4)).astype(F)
    unit[:3, :3] = [[0.0, 0.5, 0.99999994], [1 / 255, 2 / 255, 254.5 / 255], [0.25, 0.75, 0.1]]
    assert rd.Accumulate(sh.upload(rd, plt, unit), npix, 0, fr.scratch, fr.image, debug=True) == 0
    rc.running_mean(want, unit, 0)
    got, img = fr.read()
    assert same(got, want) and same(img, rc.debug_rgba8(unit))
    half = rng.uniform(0, 1, (npix, 4)).astype(F)
    assert rd.Accumulate(sh.upload(rd, plt, half), npix, 1, fr.scratch, fr.image, debug=True) == 0
    rc.running_mean(want, half, 1)
    got, img = fr.read()
    assert same(got, want) and same(img, rc.debug_rgba8(want))
    # an image of fewer pixels than the scratch buffer bounds the frame
    small = Frame(rd, plt, npix, image_pixels=npix - 10)
    small.set_scratch(start)
    assert rd.Accumulate(sh.upload(rd, plt, unit), npix, 0, small.scratch, small.image, debug=True) == 10
    got, img = small.read()
    assert same(got[:npix - 10, :3], unit[:npix - 10, :3]) and same(got[npix - 10:], start[npix - 10:]) and same(img, rc.debug_rgba8(unit)[:npix - 10])
    assert rd.Accumulate(sh.upload(rd, plt, unit), npix, 0, small.scratch, None) == 0       # without the image the scratch buffer alone does
    assert same(small.read()[0][:, :3], unit[:, :3])


# ---- 5. whole frames from the public calls ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.SCENES)
def test_frames_from_public_calls(mods, golden, name):
    """GenerateRays -> per bounce (QueryRays -> ShadeHits, compacting -> QueryRays on the shadow rays -> fold) -> Accumulate with
    the image, batchSize samples a frame, two frames: imageScratch and the RGBA8 image equal the reference's recorded frames and
    what this library's own TraceRays leaves in the scene's buffers"""
    rd, _ = mods
    c = golden(name)
    dev, p, plt = c.dev, c.s.rtprop, c.dev.plt
    npix = dev.width * dev.height
    dev.bind()
    scratch, image = rd.CreateBuffer(plt, 16 * npix), rd.CreateImage(plt, dev.width, dev.height)
    rd.WriteBuffer(plt, scratch, 16 * npix, np.zeros(4 * npix, F))
    got = rc.device_frames(rd, dev, scratch, image, 0, int(p["batchSize"]), int(p["depth"]), 2)
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


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(mods, golden):
    """every refusal of include/rdx.h returns an error that names the call, and leaves the outputs as they were; n == 0 succeeds"""
    rd, _ = mods
    c = golden("c0")
    dev, plt = c.dev, c.dev.plt
    cam = dev.frame_buffers()[0]
    n, tail = 200, 128
    bR, bK, bP, bS = (rc.filled(rd, plt, rec * n + tail) for rec in (32, 16, 4, 16))
    bC, scratch, image = rc.filled(rd, plt, 16 * n + tail, 0), rc.filled(rd, plt, 16 * n), rc.filled(rd, plt, 4 * n)
    rd.WriteBuffer(plt, bP, 4 * n, np.arange(n, dtype=np.uint32))
    one = rc.filled(rd, plt, 64 * n + 256)          # pixels | seeds | room for outputs, for the overlap cases
    rd.WriteBuffer(plt, one, 4 * n, np.arange(n, dtype=np.uint32))
    null, unknown = rd.Buffer(None, 1 << 20), rd.Buffer(12345678, 1 << 20)
    outs = dict(rays=bR, keys=bK, scratch=scratch, image=image, one=one)
    snapshot = lambda: {k: rc.whole(rd, plt, b) for k, b in outs.items()}
    good = snapshot()

    def gen(**kw):
        a = dict(camera=cam, n=n, frame_id=1, total_samples=0, first_pixel=0, pixels=bP, seeds=bS, rays=bR, keys=bK)
        a.update(kw)
        return rd.GenerateRays(a.pop("camera"), a.pop("n"), a.pop("frame_id"), a.pop("total_samples"), **a)

    def acc(**kw):
        a = dict(colors=bC, n=n, frame_id=1, scratch=scratch, image=image, pixels=bP)
        a.update(kw)
        return rd.Accumulate(a.pop("colors"), a.pop("n"), a.pop("frame_id"), a.pop("scratch"), **a)

    wrapped = lambda b, shift, size: rd.WrapDeviceMemory(plt, b.device_ptr + shift, size, keepalive=b)
    gen_cases = [
        ("null camera", dict(camera=null), "camera buffer handle"), ("unknown camera", dict(camera=unknown), "camera buffer handle"),
        ("null rays", dict(rays=null), "ray buffer handle"), ("unknown rays", dict(rays=unknown), "ray buffer handle"),
        ("unknown pixels", dict(pixels=unknown), "pixel buffer handle"), ("unknown seeds", dict(seeds=unknown), "seed buffer handle"),
        ("unknown keys", dict(keys=unknown), "key buffer handle"),
        ("a camera buffer of 32 bytes", dict(camera=rd.CreateBuffer(plt, 32)), "PhysicalCamera"),
        ("rays_offset 8", dict(rays_offset=8), "16"), ("keys_offset 24", dict(keys_offset=24), "16"), ("seeds_offset 4", dict(seeds_offset=4), "16"),
        ("pixels_offset 2", dict(pixels_offset=2), "4"),
        ("rays past the end", dict(rays_offset=tail + 16), "ray buffer"), ("keys past the end", dict(keys_offset=tail + 16), "key buffer"),
        ("seeds past the end", dict(seeds_offset=tail + 16), "seed buffer"), ("pixels past the end", dict(pixels_offset=tail + 4), "pixel buffer"),
        ("rays one record short", dict(rays=rd.CreateBuffer(plt, 32 * n - 16)), "ray buffer"),
        ("an offset beyond the buffer", dict(keys_offset=1 << 30), "key buffer"),
        ("first_pixel + n overflows", dict(pixels=None, first_pixel=0xffffffff - n + 2), "32 bits"),
        ("rays over the pixels", dict(pixels=one, rays=one, rays_offset=4 * n - 16 - (4 * n - 16) % 16), "overlap"),
        ("rays over the seeds", dict(seeds=one, seeds_offset=0, rays=one, rays_offset=16 * n - 16), "overlap"),
        ("keys over the pixels", dict(pixels=one, keys=one, keys_offset=0), "overlap"),
        ("keys = rays", dict(rays=one, rays_offset=32 * n, keys=one, keys_offset=32 * n), "overlap"),
        ("keys over the rays' tail", dict(rays=one, rays_offset=0, pixels=None, seeds=None, keys=one, keys_offset=32 * n - 16), "overlap"),
        ("rays over the camera", dict(rays=wrapped(cam, 0, 48), n=1, pixels=None, seeds=None, keys=None), "overlap"),
        ("misaligned wrapped rays", dict(rays=wrapped(bR, 8, 32 * n + 64)), "aligned"),
        ("misaligned wrapped pixels", dict(pixels=wrapped(bP, 2, 4 * n + 64)), "aligned"),
    ]
    acc_cases = [
        ("null colors", dict(colors=null), "colour buffer handle"), ("unknown colors", dict(colors=unknown), "colour buffer handle"),
        ("null scratch", dict(scratch=null), "scratch"), ("unknown scratch", dict(scratch=unknown), "scratch"),
        ("unknown image", dict(image=unknown), "image buffer handle"), ("unknown pixels", dict(pixels=unknown), "pixel buffer handle"),
        ("colors_offset 8", dict(colors_offset=8), "16"), ("pixels_offset 2", dict(pixels_offset=2), "4"),
        ("colors past the end", dict(colors_offset=tail + 16), "colour buffer"), ("pixels past the end", dict(pixels_offset=tail + 4), "pixel buffer"),
        ("first_pixel + n overflows", dict(pixels=None, first_pixel=0xffffffff - n + 2), "32 bits"),
        ("colors inside scratch", dict(colors=wrapped(scratch, 0, 16 * n)), "overlap"),
        ("colors inside the image", dict(colors=wrapped(image, 0, 4 * n), n=n // 4), "overlap"),
        ("pixels inside scratch", dict(pixels=wrapped(scratch, 16, 4 * n)), "overlap"),
        ("image inside scratch", dict(image=wrapped(scratch, 64, 4 * n)), "overlap"),
        ("misaligned wrapped scratch", dict(scratch=wrapped(scratch, 8, 16 * n - 16)), "aligned"),
        ("misaligned wrapped image", dict(image=wrapped(image, 2, 4 * n - 4)), "aligned"),
    ]
    for call, who, cases in ((gen, "rdx_generate_rays", gen_cases), (acc, "rdx_accumulate", acc_cases)):
        for what, kw, word in cases:
            with pytest.raises(rd.RadianceError) as e:
                call(**kw)
            assert word in str(e.value) and who in str(e.value), (what, str(e.value))
            now = snapshot()
            for k in outs:
                assert np.array_equal(now[k], good[k]), (what, k)
    from radiance_ray_tracing_amd import _lib
    L = _lib.lib()
    assert L.rdx_accumulate(bC.handle, 0, n, 0, None, 0, 1, scratch.handle, None, 2, None) != 0 and "flags" in _lib.last_error()
    for what, fn in (("camera not a Buffer", lambda: gen(camera=7)), ("rays not a Buffer", lambda: gen(rays=7)), ("pixels not a Buffer", lambda: gen(pixels=[1, 2])),
                     ("colors not a Buffer", lambda: acc(colors=np.zeros(4))), ("image not a Buffer", lambda: acc(image=7))):
        with pytest.raises(rd.RadianceError):
            fn()
    # n == 0 succeeds and touches nothing -- also at the very end of a buffer
    assert gen(n=0)[0] is bR and gen(n=0, rays_offset=32 * n + tail, pixels=None, seeds=None, keys=None)[1] is None
    assert acc(n=0) == 0 and acc(n=0, colors_offset=16 * n + tail, pixels=None, image=None) == 0
    assert all(np.array_equal(v, good[k]) for k, v in snapshot().items())
    # adjacent ranges of one buffer are fine, and the calls still work after the refusals
    gen(pixels=one, pixels_offset=0, seeds=None, rays=one, rays_offset=4 * n + (-4 * n) % 16, keys=one, keys_offset=4 * n + (-4 * n) % 16 + 32 * n)
    want, _ = rd.GenerateRays(cam, n, 1, 0)
    at = 4 * n + (-4 * n) % 16
    assert same(rd.ReadBuffer(plt, one, 32 * n, offset=at), rd.ReadBuffer(plt, want, 32 * n))
    check_keys(rd.ReadBuffer(plt, one, 16 * n, offset=at + 32 * n).view(rd.SHADE_KEY_DTYPE), 1, np.arange(n))
    assert acc(frame_id=0) == 0
    assert not rd.ReadBuffer(plt, scratch, 16 * n).view(F).reshape(-1, 4)[:, :3].any()        # the colours were zeros


# ---- 7. torch tensors -----------------------------------------------------------------------------------------------------------------
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
import raygen_cases as rc
import shade_cases as sh
F = np.float32
c = sh.Golden(rd, scenes, "c0")
dev, plt = c.dev, c.dev.plt
cam, scratch, image = dev.frame_buffers()
npix = dev.width * dev.height
# the buffer route
bR, bK = rd.GenerateRays(cam, npix, 5, 4)
want_r, want_k = sh.read(rd, plt, bR, npix, rd.RAY_DTYPE), sh.read(rd, plt, bK, npix, rd.SHADE_KEY_DTYPE)
rays, keys = rd.GenerateRaysTorch(cam, npix, 5, 4)
assert rays.dtype == torch.float32 and tuple(rays.shape) == (npix, 8) and keys.dtype == torch.int32 and tuple(keys.shape) == (npix, 4)
assert np.array_equal(rays.cpu().numpy().view(np.uint32), want_r.view(np.uint32).reshape(npix, 8))
assert np.array_equal(keys.cpu().numpy().view(np.uint32), want_k.view(np.uint32).reshape(npix, 4))
# a pixel tensor a torch op produced, and seeds
sel = torch.randperm(npix, device="cuda")[:777].to(torch.int32).contiguous()
rays2, keys2 = rd.GenerateRaysTorch(cam, sel, 5, 4)
idx = sel.cpu().numpy().astype(np.int64)
assert np.array_equal(rays2.cpu().numpy().view(np.uint32), want_r[idx].view(np.uint32).reshape(-1, 8))
assert np.array_equal(keys2.cpu().numpy()[:, 1], idx) and (keys2[:, 0] == 5).all() and not keys2[:, 2:].any()
seeds = torch.from_numpy(rc.seeds_of(c.G["gen_rnd"]).view(np.int32).reshape(npix, 4).copy()).cuda()
rays3, _ = rd.GenerateRaysTorch(cam, npix, 0, 0, seeds=seeds)
assert np.array_equal(rays3.cpu().numpy()[:, 0:3].view(np.uint32), c.G["gen_o"].view(np.uint32))
assert np.array_equal(rays3.cpu().numpy()[:, 4:7].view(np.uint32), c.G["gen_d"].view(np.uint32))
# the rays are what QueryRaysTorch / ShadeHitsTorch take
h = rd.QueryRaysTorch(dev.topAccelStruct, rays, 1)
shade = rd.ShadeHitsTorch(dev.topAccelStruct, rays, h, keys, dev.shading_buffers())[0]
# accumulate: tensors for the frame, against the buffer route on buffers of its own
rng = np.random.default_rng(7)
col = rng.normal(0.4, 0.6, (npix, 4)).astype(F)
ct = (torch.from_numpy(col).cuda() * torch.ones(4, device="cuda")).contiguous()
st = torch.zeros((npix, 4), dtype=torch.float32, device="cuda")
it = torch.zeros((npix, 4), dtype=torch.uint8, device="cuda")
bS, bI = rd.CreateBuffer(plt, 16 * npix), rd.CreateBuffer(plt, 4 * npix)
rd.WriteBuffer(plt, bS, 16 * npix, np.zeros(4 * npix, F)); rd.WriteBuffer(plt, bI, 4 * npix, np.zeros(4 * npix, np.uint8))
for frame in (0, 1, 2):
    assert rd.AccumulateTorch(ct, frame, st, it) == 0
    assert rd.Accumulate(sh.upload(rd, plt, col), npix, frame, bS, bI) == 0
    assert np.array_equal(st.cpu().numpy().view(np.uint32), rd.ReadBuffer(plt, bS, 16 * npix).view(np.uint32).reshape(npix, 4))
    assert np.array_equal(it.cpu().numpy(), rd.ReadBuffer(plt, bI, 4 * npix).reshape(npix, 4))
want = np.zeros((npix, 4), F)
for frame in (0, 1, 2):
    rc.running_mean(want, col, frame)
assert np.array_equal(st.cpu().numpy().view(np.uint32), want.view(np.uint32)) and (it[:, 3] == 255).all()
# a pixel tensor, the scene's own buffers, no image, debug; pixels outside the frame are counted
rd.WriteBuffer(plt, scratch, 16 * npix, np.zeros(4 * npix, F))
sub = torch.cat([sel[:100], torch.tensor([npix, -1], dtype=torch.int32, device="cuda")]).contiguous()
assert rd.AccumulateTorch(ct[:102].contiguous(), 0, scratch, pixels=sub) == 2
got = rd.ReadBuffer(plt, scratch, 16 * npix).view(F).reshape(npix, 4)
assert np.array_equal(got[idx[:100], :3].view(np.uint32), col[:100, :3].view(np.uint32)) and int((got != 0).any(1).sum()) <= 100
assert rd.AccumulateTorch(ct, 0, st, image=it, debug=True) == 0
# the loop of the README, line for line: one sample of every pixel from the camera ray to the image, tensors throughout
def readme_sample(scene, tlas, n, frame, total_samples, max_depth):
    sb = scene.shading_buffers()
    camera, scratch, image = scene.frame_buffers()
    rays, keys = rd.GenerateRaysTorch(camera, n, frame, total_samples)
    pixel = keys[:, 1].contiguous()
    color = torch.zeros((n, 4), device="cuda")
    weight = torch.ones((n, 3), device="cuda")
    path = torch.arange(n, device="cuda")
    for depth in range(max_depth):
        if depth:
            keys = torch.stack([torch.full_like(pixel, frame), pixel, torch.full_like(pixel, depth), torch.zeros_like(pixel)], 1).contiguous()
        hits = rd.QueryRaysTorch(tlas, rays, rd.QUERY_CLOSEST)
        shade, rays, shadow, src, live, _ = rd.ShadeHitsTorch(tlas, rays, hits, keys, sb)
        hit = shade.view(torch.int32)[:, 3] == 1
        if depth == 0:
            color[path[~hit], :3] = shade[~hit, 0:3]
        src = src.long()
        occluded = rd.QueryRaysTorch(tlas, shadow, rd.QUERY_ANY)[:, 3:4] == 1
        color[path[src], :3] += weight[path[src]] * torch.where(occluded, shade[src, 4:7], shade[src, 0:3])
        weight[path[src]] *= shade[src, 8:11]
        path, pixel = path[src], pixel[src].contiguous()
        if live == 0:
            break
    rd.AccumulateTorch(color, frame, scratch, image)
p = c.s.rtprop
dev.clear_scratch()
for f in range(2):
    for it_ in range(int(p["batchSize"])):
        readme_sample(dev, dev.topAccelStruct, npix, f * int(p["batchSize"]) + it_, f * int(p["batchSize"]), int(p["depth"]))
    assert np.array_equal(dev.read_scratch().reshape(-1).view(np.uint32), c.G["scratch%d" % f].view(np.uint32)), f
    assert np.array_equal(rd.ReadBuffer(plt, image, 4 * npix), c.G["image%d" % f]), f
dev.clear_scratch()
assert rd.AccumulateTorch(ct[:0], 0, st) == 0 and tuple(rd.GenerateRaysTorch(cam, 0, 0, 0)[0].shape) == (0, 8)
bad_gen = [(sel.long(), None), (sel.float(), None), (sel.cpu(), None), (torch.arange(2 * npix, device="cuda", dtype=torch.int32)[::2], None),
           (sel.view(-1, 1), None), (npix, seeds[:, :3]), (npix, seeds.float()), (npix, seeds[:-1]), (npix, seeds.cpu()), (-1, None), (2.5, None)]
for j, (p_, s_) in enumerate(bad_gen):
    try:
        rd.GenerateRaysTorch(cam, p_, 0, 0, seeds=s_)
    except rd.RadianceError:
        continue
    raise AssertionError("GenerateRaysTorch: bad argument set %d was accepted" % j)
wide = torch.zeros((npix, 8), dtype=torch.float32, device="cuda")
bad_acc = [dict(colors=ct[:, :3]), dict(colors=ct.double()), dict(colors=ct.cpu()), dict(colors=wide[:, ::2]), dict(colors=col),
           dict(scratch=st.double()), dict(scratch=st[:, :3]), dict(scratch=wide[:, ::2]), dict(scratch=st.cpu()), dict(scratch=None),
           dict(image=it.float()), dict(image=it[:, :3]), dict(image=it.cpu()), dict(pixels=sel), dict(pixels=sub.long()), dict(pixels=torch.arange(npix))]
for j, kw in enumerate(bad_acc):
    a = dict(colors=ct, frame_id=0, scratch=st, image=it, pixels=None)
    a.update(kw)
    try:
        rd.AccumulateTorch(a.pop("colors"), a.pop("frame_id"), a.pop("scratch"), **a)
    except rd.RadianceError:
        continue
    raise AssertionError("AccumulateTorch: bad argument set %d was accepted" % j)
print("TORCH-RAYGEN-OK", npix, int(shade.shape[0]))
"""


def test_torch_tensors_in_a_fresh_process(gpu):
    """rd.GenerateRaysTorch / rd.AccumulateTorch equal the buffer routes bit for bit; a non-contiguous tensor, a wrong dtype, shape
    or device is refused in Python.  torch is initialised first, in a process of its own (as tests/test_gpu_shade.py does)"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _TORCH_CHILD, ROOT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "TORCH-RAYGEN-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])

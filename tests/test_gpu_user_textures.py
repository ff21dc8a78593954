"""GPU suite (-m gpu): texture reads in user shader programs.  A user program reads the texture array bound in slot 11 through
the sampler bound in slot 12 with read_imageui / get_image_* (csrc/user_shader.cpp prelude, csrc/user_texture.hip -- the
stock shader's sampler, csrc/texture.h), in the megakernel and in stage mode.  Results are held BIT-EXACT against a numpy
float32 restatement of that sampler (tests/user_texture_ref.py).

Each test first compiles the program it is about to launch through the compile-only seam and asserts that the code object
holds no hardware image instruction: a library that would emit them (they read a descriptor the program does not have) fails
there, before anything is launched."""
import numpy as np
import pytest

import user_texture_ref as tr

pytestmark = pytest.mark.gpu
F = np.float32
W_IMG, H_IMG, L_IMG = 48, 32, 3          # non-square: swapped width / height would show


@pytest.fixture(scope="module")
def mods(gpu):
    import rrt_amd
    from radiance_ray_tracing_amd import _lib, rd, scenes
    return rd, scenes, tr.jit_lib(_lib.LIB_PATH)


def _kat_coords():
    """a grid over [-1.5, 2.5]^2, the texel boundaries of both filters (k / n and (k + 0.5) / n) and their neighbours 1 ulp
    away, layers {-1, -0.5, 0.49, 0.5, 1.5, 2, 9}"""
    g = np.linspace(-1.5, 2.5, 41, dtype=F)
    gu, gv = [a.ravel() for a in np.meshgrid(g, g)]

    def edges(n):
        k = np.arange(-n - 16, 2 * n + 17, dtype=F)
        e = np.concatenate([k / F(n), (k + F(0.5)) / F(n)]).astype(F)
        return np.concatenate([e, np.nextafter(e, F(-np.inf)), np.nextafter(e, F(np.inf))]).astype(F)
    eu, ev = edges(W_IMG), edges(H_IMG)
    rng = np.random.default_rng(11)
    u = np.concatenate([gu, eu, rng.uniform(-1.5, 2.5, ev.size).astype(F), eu[rng.integers(0, eu.size, ev.size)]])
    v = np.concatenate([gv, rng.uniform(-1.5, 2.5, eu.size).astype(F), ev, ev])
    layers = np.array([-1.0, -0.5, 0.49, 0.5, 1.5, 2.0, 9.0], F)
    lay = layers[np.arange(u.size) % layers.size]
    return np.ascontiguousarray(np.stack([u, v, lay, np.zeros_like(u)], 1).astype(F))


def _texel_coords(n):
    rng = np.random.default_rng(12)
    c = np.stack([rng.integers(-3, W_IMG + 3, n), rng.integers(-3, H_IMG + 3, n), rng.integers(-1, L_IMG + 2, n), np.zeros(n, np.int64)], 1)
    return np.ascontiguousarray(c.astype(np.int32))


class _Probe:
    """tests/golden/user_texture_probe.cl bound as a megakernel over n work-items, every other slot a small buffer"""

    def __init__(self, rd, coords, texels):
        self.rd = rd
        plt = self.plt = rd.Platform.GetPlatform()
        self.n = n = coords.shape[0]
        text = tr.probe_program()
        shader = rd.CreateShaderModule(plt, text, len(text), "texture probe")
        layout = [rd.BUFFER_TYPE, rd.BUFFER_TYPE, rd.IMAGE_TYPE] + [rd.BUFFER_TYPE] * 8 + [rd.TEX_ARRAY_TYPE, rd.IMAGE_SAMPLER_TYPE, rd.ACCEL_STRUCT_TYPE]
        self.pipeline = rd.CreatePipeline(rd.PipelineCreateInfo(1, layout, [shader], []))
        prop = np.array([0, n, 1, 0], np.uint32)
        self.rt = rd.CreateBuffer(plt, 16); rd.WriteBuffer(plt, self.rt, 16, prop)
        self.out_bytes = (2 * n + 2) * 16
        self.out = rd.CreateBuffer(plt, self.out_bytes)
        self.coords = rd.CreateBuffer(plt, coords.nbytes); rd.WriteBuffer(plt, self.coords, coords.nbytes, coords)
        self.texels = rd.CreateBuffer(plt, texels.nbytes); rd.WriteBuffer(plt, self.texels, texels.nbytes, texels)
        self.dummy = [rd.CreateBuffer(plt, 256) for _ in range(8)]

    def run(self, image, sampler):
        rd, d = self.rd, self.dummy
        rd.BindPipeline(self.plt, self.pipeline)
        rd.BindDescriptorSet(self.plt, [self.rt, self.out, d[0], d[1], d[2], d[3], self.texels, d[4], self.coords, d[5], d[6], image, sampler, d[7]])
        rd.WriteBuffer(self.plt, self.out, self.out_bytes, np.full(self.out_bytes // 4, 0xdeadbeef, np.uint32))
        rd.TraceRays(self.plt, 0, 0, 0, self.n, 1)
        o = rd.ReadBuffer(self.plt, self.out, self.out_bytes).view(np.uint32).reshape(-1, 4)
        return o[:self.n], o[self.n:2 * self.n], o[2 * self.n:]


def _image(rd, plt, tex):
    img = rd.CreateImageArray(plt, W_IMG, H_IMG, L_IMG)
    for l in range(L_IMG):
        rd.WriteImage(plt, img, W_IMG, H_IMG, l, tex[l])
    return img


def test_user_program_sampler_is_bit_exact(mods):
    """read_imageui(image2d_array_t, sampler_t, float4) in a user megakernel, all four addressing modes x nearest / linear,
    against the numpy restatement of texture.h bit for bit (any FMA contraction across the link would show); the samplerless
    int4 read and the queries; a NULL slot 11 or 12 gives zeros and the frame completes"""
    rd, scenes, lib = mods
    tr.assert_no_image_code(lib, tr.probe_program(), 0)
    plt = rd.Platform.GetPlatform()
    tex = tr.test_image(W_IMG, H_IMG, L_IMG)
    img = _image(rd, plt, tex)
    coords, texels = _kat_coords(), None
    texels = _texel_coords(coords.shape[0])
    probe = _Probe(rd, coords, texels)
    want_texels = tr.texel_read(tex, texels)
    queries = np.array([[W_IMG, H_IMG, L_IMG, 7], [W_IMG, H_IMG, 0, 7]], np.uint32)
    modes = [(tr.REPEAT, rd.RD_ADDRESS_REPEAT), (tr.CLAMP_TO_EDGE, rd.RD_ADDRESS_CLAMP_TO_EDGE), (tr.CLAMP, rd.RD_ADDRESS_CLAMP),
             (tr.MIRRORED, rd.RD_ADDRESS_MIRRORED_REPEAT)]
    seen = []
    for mode, addr in modes:
        for linear, filt in ((False, rd.RD_FILTER_NEAREST), (True, rd.RD_FILTER_LINEAR)):
            got, got_t, got_q = probe.run(img, rd.CreateSampler(plt, addr, filt))
            want = tr.sample(tex, mode, linear, coords)
            bad = np.nonzero((got != want).any(1))[0]
            assert bad.size == 0, (mode, linear, bad.size, coords[bad[:4]], got[bad[:4]], want[bad[:4]])
            assert np.array_equal(got_t, want_texels) and np.array_equal(got_q, queries), (mode, linear)
            seen.append(got)
    assert len({g.tobytes() for g in seen}) == len(seen), "two sampler settings gave the same reads"
    # NULL texture array: everything reads 0 (the live reference shader's stub), queries are 0
    smp = rd.CreateSampler(plt, rd.RD_ADDRESS_REPEAT, rd.RD_FILTER_LINEAR)
    got, got_t, got_q = probe.run(None, smp)
    assert not got.any() and not got_t.any() and np.array_equal(got_q, [[0, 0, 0, 7], [0, 0, 0, 7]])
    # NULL sampler: the sampled reads are 0; the samplerless read and the queries need no sampler
    got, got_t, got_q = probe.run(img, None)
    assert not got.any() and np.array_equal(got_t, want_texels) and np.array_equal(got_q, queries)
    # and the views follow a rebind: the image again, through another sampler
    got, _, _ = probe.run(img, rd.CreateSampler(plt, rd.RD_ADDRESS_CLAMP, rd.RD_FILTER_NEAREST))
    assert np.array_equal(got, tr.sample(tex, tr.CLAMP, False, coords))


def test_textured_closest_hit_in_stage_mode(mods):
    """tests/golden/user_texture_stages.cl under user_stages 2, depth 1, 1 spp: its closest-hit shader's colour is the texel at
    (b1, b2, primitiveIndex % 3).  imageScratch equals the numpy sampler applied to the trace-batch hits of the same primary
    rays, bit for bit (at totalSamples 0 the accumulator stores the sample, and colour = 0 + 1 * payload colour).  With the
    shadow query in the shader the frame is the same; with no image bound the hits are black"""
    rd, scenes, lib = mods
    plain, query = tr.stage_program(), tr.stage_program(query=True)
    for t in (plain, query):
        tr.assert_no_image_code(lib, t, 1)
    W, H = 160, 90
    s = scenes.c1_cornell(W, H, spp=1, depth=1, sphere_subdiv=2)
    rd.SetShaderIncludePath("")
    rd.SetOption("user_stages", 2)
    try:
        devs = [scenes.DeviceScene(s, shader_text=t) for t in (plain, query)]
    finally:
        rd.SetOption("user_stages", 1)
    plt = devs[0].plt
    tex = tr.test_image(W_IMG, H_IMG, L_IMG)
    img = _image(rd, plt, tex)
    smp = rd.CreateSampler(plt, rd.RD_ADDRESS_REPEAT, rd.RD_FILTER_LINEAR)

    def frame(dev, image):
        dev.bind()
        ds = list(dev.descSet); ds[11] = image; ds[12] = smp
        rd.BindDescriptorSet(plt, ds)
        dev.set_rtprop(totalSamples=0); dev.clear_scratch()
        rd.TraceRays(plt, 0, 0, 0, W, H)
        st = rd.GetTraceStats()
        assert st.launches_extend >= 1 and st.launches_shadow == st.launches_extend, "the program did not run on the wavefront pipeline"
        return dev.read_scratch().reshape(-1, 4).copy()

    got = frame(devs[0], img)
    px = np.arange(W * H, dtype=np.uint32)
    o, d = rd.GenerateBatch(px, np.stack([np.zeros_like(px), np.zeros_like(px), px], 1))
    hits = rd.TraceBatch(devs[0].topAccelStruct, o, d)
    k = hits["hit"] == 1
    assert k.sum() > W * H // 2
    c = np.stack([hits["barycentric"][:, 1], hits["barycentric"][:, 2], (hits["primitiveIndex"] % 3).astype(F), np.zeros(W * H, F)], 1)
    want = np.zeros((W * H, 4), F)
    want[:, :3] = tr.sample(tex, tr.REPEAT, True, c)[:, :3].astype(F)
    want[~k] = 0.0
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    assert bad.size == 0, (bad.size, got[bad[:4]], want[bad[:4]])
    got_q = frame(devs[1], img)
    assert np.array_equal(got_q.view(np.uint32), want.view(np.uint32))
    dark = frame(devs[0], None)
    assert not dark.any() and not np.array_equal(dark, got)

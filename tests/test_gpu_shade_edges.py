"""GPU suite (-m gpu): the shading calls held to the reference at the edges of their inputs.

Inputs: tests/shade_edge_cases.py -- a scene of one quad per case (Material records with out-of-range and NaN parameters, vertex
normals that are zero, cancelling, denormal, huge and on either side of GetNormalSpace's 1e-6 threshold, transforms scaled by
1e-15 .. 1e15), rays from the front, from behind, grazing and with directions scaled by 1e-25 / 1e25, RNG keys searched for the
extremes of every random number the BRDF sampler branches on, lights with zero / tiny / huge directions and zero / negative / inf
/ NaN colours, caller-filled material records, cameras with degenerate lenses and frames, and colours of 20 decades, both signs
and every special value for the tone map.

Comparand: tests/golden/refgpu_shade_edges.npz -- what the reference's own device code (oracle/_ref, build p, run on an MI355X by
tests/golden/make_golden_gpu.py shadeedges) answers -- and, where the code object is present, the same recordings made afresh
next to the product (fixture `live`; they must equal the committed ones).  THE RULE (shade_edge_cases.compare): equal bits, signs
of zero and infinities included; a component that is NaN in the reference must be NaN in the product.

What is left out, and only this: where the interpolated vertex normal is exactly (0, 0, 0) the reference's G_pbrt reads an
uninitialised matrix (InverseMat4x4 leaves its output unwritten when det == 0, math.cl:176; the product zeroes it).  Those rows --
shade_edge_cases.zero_normal_rows, found from the inputs and the reference's barycentrics -- do not compare `color`, `nextFactor`
and `lit`; their hit flag, colorOccluded, materialIndex, material record, shadow ray and next ray are compared like any other's.

Why NaN / inf / zero next rays may go back into the walk (tests a, e, f): family F of test_gpu_ray_edges.py states why every
engine ends on such rays (a ray's floats decide which children are entered, never whether a loop continues); rdx_trace_paths and
the frame path share one bounce loop (rdx_runtime.cpp trace_bounces: a host-side `for` over max_depth around k_shade and the
traversal launches, the live paths counted in integers), k_shade has no loop, and the per-bounce ray sort clamps a ray's cell with
fminf(fmaxf(x, 0), 15) before it becomes an index, which sends a NaN to cell 0.

That these tests notice a wrong kernel was checked with local mutations (never committed), each run against this file and against
the GPU suite as it was before this file:
  normalize3 (device_math.h) without its zero-vector exit: tests a (main, s-25, s+25, every light buffer), b, f and h fail -- the
      zero normals, the zero light direction and the camera without focal length and sensor; the earlier suite passes
  roughness clamped to 0.05 instead of 0 in the untextured path of `material` (stages.h): tests a, b, c and f fail; the earlier
      suite passes
  `frameID + 1.0f` for `frameID + 1` in the running mean (raygen_device.h): test g fails at frameID 2^24 + 1 and 0xffffffff; the
      earlier suite passes
  make_frame's 1e-6 made 1e-5 (stages.h): tests a, b and f fail -- but so do 17 earlier tests, all on the atrium scene, whose
      curved surfaces meet the threshold by chance; here the 5e-7 and 2e-6 normals meet it by construction.
"""
import os

import numpy as np
import pytest

import golden_cases as gc
import material_cases as mc
import oracle_bind as ob
import paths_cases as pc
import refgpu_bind as rg
import shade_cases as sh
import shade_edge_cases as se

pytestmark = pytest.mark.gpu
F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
bits, compare = se.bits, se.compare


@pytest.fixture(scope="module")
def mods(gpu):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd, scenes
    return rd, scenes


@pytest.fixture(scope="module")
def G():
    return dict(np.load(os.path.join(GOLD, "refgpu_shade_edges.npz")))


@pytest.fixture(scope="module")
def live(mods):
    """the recordings made afresh by the live reference code object, or None where oracle/_ref is absent"""
    rd, scenes = mods
    return se.reference_recordings(rg.RefGpu("p"), rg, rd, scenes) if rg.available("p") else None


def check_live(G, live, *prefixes):
    """the committed recordings under `prefixes` equal the live reference's"""
    if live is None:
        return "fixture only"
    pick = lambda R: {k: v for k, v in R.items() if k.startswith(prefixes)}
    a, b = pick(G), pick(live)
    assert a and not se.recordings_differ(a, b), "the live reference differs from the fixture in %s" % se.recordings_differ(a, b)
    return "fixture and live reference (%d arrays)" % len(a)


class Ctx:
    def __init__(self, rd, scenes, G):
        self.rd = rd
        self.s, self.inst, self.B = se.batches(scenes)
        self.dev = scenes.DeviceScene(self.s)
        self.plt, self.tlas = self.dev.plt, self.dev.topAccelStruct
        blob = rd.ReadBuffer(self.plt, self.tlas, self.tlas.size).tobytes()
        assert np.array_equal(gc.sha(blob), G["blob_sha256"]), "the TLAS blob of the edge scene changed"
        self.L = se.light_buffers(rd)
        self.bL = [sh.upload(rd, self.plt, self.L[j:j + 1]) for j in range(self.L.shape[0])]
        self.U = {name: se.unpack_batch(G, name, b.n, ob.PAYLOAD_DTYPE) for name, b in self.B.items()}
        self.left_out = {}
        for name, b in self.B.items():
            u = self.U[name]
            m = np.zeros(b.n, bool)
            m[u["hit"]] = se.zero_normal_rows(self.s, self.inst, u["inst"], u["prim"], u["bary"])
            self.left_out[name] = m
        self._shaded = {}

    def sb(self, j=0):
        sb = self.dev.shading_buffers()
        sb.scene = self.bL[j]
        return sb

    def rays(self, name):
        b = self.B[name]
        return sh.rays_of(self.rd, b.o, b.d, b.tmin, b.tmax)

    def keys(self, name):
        b = self.B[name]
        return sh.keys_of(b.frames, b.pixels, b.depths.view(np.uint32))

    def shaded(self, name, j=0):
        """query + ShadeHits + shadow query of a batch under light buffer j, not compacting; computed once"""
        if (name, j) not in self._shaded:
            self._shaded[name, j] = sh.shade_batch(self.rd, self.plt, self.tlas, self.sb(j), self.rays(name), self.keys(name))
        return self._shaded[name, j]


@pytest.fixture(scope="module")
def ctx(mods, G):
    return Ctx(mods[0], mods[1], G)


def report(tag, rows, want, left_out=0, how=""):
    """the line every test prints: rows compared, NaN and inf shares of the reference's values, rows left out"""
    w = np.ascontiguousarray(want, F)
    print("%s: %d rows compared, reference NaN share %.4f, inf share %.4f, %d rows left out; %s"
          % (tag, rows, float(np.isnan(w).mean()) if w.size else 0.0, float(np.isinf(w).mean()) if w.size else 0.0, left_out, how))


def floats_of(pay):
    return np.concatenate([pay[f] for f in ("color", "nextFactor", "nextRayOrigin", "nextRayDirection")], 1)


def table_checks(c, name, r):
    """what the payload does not carry, on every hit (the rows left out included): materialIndex is the instance's, colorOccluded is
    0 + albedo * 0.1f of the Material table"""
    u, s = c.U[name], r["shade"]
    mi = c.s.buffers()["meshInfo"]["materialIndex"][u["inst"]]
    assert np.array_equal(s["materialIndex"][u["hit"]], mi.astype(np.uint32)), name
    albedo = np.array(c.s.materials)["albedo"][mi][:, :3]
    ok = compare(s["colorOccluded"][u["hit"]], mc.color_occluded(albedo))[0]
    assert ok.all(), "%s: colorOccluded differs on %d hits" % (name, int((~ok).sum()))


# ---- a. rd.ShadeHits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("main", "s-25", "s+25", "keys"))
def test_a_shade_hits_on_the_edge_scene(ctx, G, live, name):
    c = ctx
    how = check_live(G, live, name + "/")
    b, u = c.B[name], c.U[name]
    hits = np.zeros(b.n, [("hit", "<u4")]); hits["hit"] = u["hit"]
    r = c.shaded(name)
    assert r["invalid"] == 0
    q = r["q"][u["hit"]]
    assert np.array_equal(q["instanceIndex"], u["inst"]) and np.array_equal(q["primitiveIndex"], u["prim"]) and np.array_equal(bits(q["t"]), bits(u["t"]))
    lit, occ = sh.check_against_payloads(r, hits, se.full_payloads(u, b.n, ob.PAYLOAD_DTYPE), name, compare=compare, leave_out=c.left_out[name])
    table_checks(c, name, r)
    report("a/" + name, int(u["hit"].sum()), floats_of(u["pay"]), int(c.left_out[name].sum()), "%s; lit %d, occluded %d" % (how, lit, occ))
    if name == "main":
        assert lit >= 16 and occ >= 16


def test_a_shade_hits_under_every_light_buffer(ctx, G, live):
    """batch "light" once per light buffer: every buffer changes light 0"""
    c = ctx
    how = check_live(G, live, "light/")
    b, u = c.B["light"], c.U["light"]
    hits = np.zeros(b.n, [("hit", "<u4")]); hits["hit"] = u["hit"]
    variants = se.light_variants()
    for j in range(c.L.shape[0]):
        pay = se.full_payloads(u, b.n, ob.PAYLOAD_DTYPE)
        pay["color"][u["hit"]] = G["light/color"][j]
        r = c.shaded("light", j)
        assert r["invalid"] == 0
        sh.check_against_payloads(r, hits, pay, "light buffer %d (%s)" % (j, variants[j][0]), compare=compare, leave_out=c.left_out["light"])
        table_checks(c, "light", r)
    report("a/light buffers", c.L.shape[0] * int(u["hit"].sum()), G["light/color"], c.L.shape[0] * int(c.left_out["light"].sum()), how)


# ---- b. rd.MaterialBatch: the frame path's `material` --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("main", "s-25", "s+25", "keys"))
def test_b_material_seam(mods, ctx, G, name):
    rd, _ = mods
    c = ctx
    b, u = c.B[name], c.U[name]
    c.dev.bind()
    rd.WriteBuffer(c.plt, c.dev.rdSceneData, 176, c.L[0:1])
    try:
        h = rd.TraceBatch(c.tlas, b.o, b.d, b.tmin, b.tmax)
        k = h["hit"] == 1
        assert np.array_equal(k, u["hit"]) and np.array_equal(h["instanceIndex"][k], u["inst"]) and np.array_equal(h["primitiveIndex"][k], u["prim"])
        assert np.array_equal(bits(h["distance"][k]), bits(u["t"])) and np.array_equal(bits(h["barycentric"][k]), bits(u["bary"]))
        got = rd.MaterialBatch(h[k], b.d[k], b.pixels[k], b.frames[k], b.depths[k])
    finally:
        rd.WriteBuffer(c.plt, c.dev.rdSceneData, 176, np.array(c.s.sceneProps).reshape(1))
    want, out = u["pay"], c.left_out[name][k]
    assert (got["hit"] == 1).all() and (want["hit"] == 1).all()
    # the seam reports the light-visible colour (the frame path's shadow query is a stage of its own): it is the payload's colour
    # where the shadow ray of test a was not occluded, and rd.ShadeHits' `color` -- the same term -- where it was
    r = c.shaded(name)
    occluded = r["occluded"][k]
    want_color = np.where(occluded[:, None], r["shade"]["color"][k], want["color"])
    for f, w in (("color", want_color), ("nextFactor", want["nextFactor"]), ("nextRayOrigin", want["nextRayOrigin"]),
                 ("nextRayDirection", want["nextRayDirection"])):
        ok = compare(got[f], w)[0]
        if f in ("color", "nextFactor"):
            ok = ok | out
        assert ok.all(), "%s: %s differs on %d of %d hits" % (name, f, int((~ok).sum()), ok.shape[0])
    report("b/" + name, int(k.sum()), floats_of(want), int(out.sum()), "fixture; %d colours against rd.ShadeHits (occluded)" % int(occluded.sum()))


# ---- c. rd.ResolveMaterials + rd.LightHits ---------------------------------------------------------------------------------------------
def identity_with_shade(m, r, left_out, tag):
    """material_cases.check_against_shade under THE rule: the two colours of rd.ShadeHits follow from the material record and the lit
    colour, the shadow rays are the same, `above` is the shadow origin"""
    mat, s = m["mat"], r["shade"]
    k = mat["hit"] == 1
    assert np.array_equal(mat["hit"], s["hit"]) and np.array_equal(mat["materialIndex"], s["materialIndex"]), tag
    assert not mat[~k].view(np.uint8).any() and not m["lit"][~k].view(np.uint8).any(), "%s: a miss is not zero bytes" % tag
    assert not mat["_0"].any() and not bits(m["lit"]["w"]).any(), tag
    ok = compare(mc.color_occluded(mat["albedo"][k]), s["colorOccluded"][k])[0]
    assert ok.all(), "%s: colorOccluded differs on %d hits" % (tag, int((~ok).sum()))
    with np.errstate(invalid="ignore", over="ignore"):
        ok = compare(mc.color_lit(m["lit"]["rgb"][k], mat["albedo"][k]), s["color"][k])[0] | left_out[k]
    assert ok.all(), "%s: color differs on %d hits" % (tag, int((~ok).sum()))
    for f in ("origin", "direction", "tmin", "tmax"):
        assert compare(m["shadow"][f], r["shadow"][f])[0].all(), "%s: shadow %s" % (tag, f)
    assert compare(mat["above"][k], m["shadow"]["origin"][k])[0].all(), "%s: above is not the shadow origin" % tag
    assert np.array_equal(m["occluded"], r["occluded"]), tag
    return int(k.sum())


@pytest.mark.parametrize("name", ("main", "keys"))
def test_c_material_records_and_light_0(mods, ctx, name):
    rd, _ = mods
    c = ctx
    r = c.shaded(name)
    m = mc.material_batch(rd, c.plt, c.tlas, c.sb(0), c.rays(name))
    assert m["invalid"] == 0
    n = identity_with_shade(m, r, c.left_out[name], name)
    report("c/" + name, n, r["shade"]["color"], int(c.left_out[name].sum()), "against rd.ShadeHits of test a")


def test_c_every_light_of_every_buffer(mods, ctx):
    """light k of buffer j gives the lit colour and the shadow ray of the same variant in slot 0 (which test a holds to the reference
    through rd.ShadeHits under that buffer)"""
    rd, _ = mods
    c = ctx
    nv = c.L.shape[0]
    n = c.B["light"].n
    base = mc.material_batch(rd, c.plt, c.tlas, c.sb(0), c.rays("light"), want_shadow=False)
    in_slot0 = []
    for v in range(nv):
        m = dict(base, **mc.light_batch(rd, c.plt, c.tlas, base["bR"], base["bM"], n, c.bL[v], 0))
        identity_with_shade(m, c.shaded("light", v), c.left_out["light"], "variant %d in slot 0" % v)
        in_slot0.append(m)
    rows = 0
    for j in range(nv):
        for k in range(1, 5):
            m, w = mc.light_batch(rd, c.plt, c.tlas, base["bR"], base["bM"], n, c.bL[j], k), in_slot0[(j + k) % nv]
            assert compare(m["lit"]["rgb"], w["lit"]["rgb"])[0].all() and not bits(m["lit"]["w"]).any(), (j, k)
            for f in ("origin", "direction", "tmin", "tmax"):
                assert compare(m["shadow"][f], w["shadow"][f])[0].all(), (j, k, f)
            assert np.array_equal(m["occluded"], w["occluded"]), (j, k)
            rows += n
    report("c/lights 1-4", rows, np.concatenate([w["lit"]["rgb"] for w in in_slot0]), 0, "against light 0 of the buffer that holds the variant there")


# ---- d. rd.LightHits on caller-filled records -----------------------------------------------------------------------------------------
def test_d_light_hits_on_caller_filled_records(mods, ctx, G, live):
    rd, _ = mods
    c = ctx
    plt = c.plt
    how = check_live(G, live, "brdf")
    g = se.brdf_grid()
    n = g["l"].shape[0]
    rays = sh.rays_of(rd, np.zeros((n, 3), F), -g["V"][g["v"]])
    mat = np.zeros(n, mc.MATERIAL_RECORD_DTYPE)
    mat["hit"] = 1
    for f in ("albedo", "metallic", "roughness", "transmission", "ior"):
        mat[f] = g[f]
    mat["normal"] = g["N"]

    def scene_of(directions):
        sp = np.zeros(1, rd.SceneProperties)
        sp[0]["lightCount"][0] = 5
        for k, d in enumerate(directions):
            sp[0]["lights"][k]["direction"][:3] = -np.asarray(d, F)
            sp[0]["lights"][k]["color"] = (1.0, 1.0, 1.0, 1.0)
        return sh.upload(rd, plt, sp)
    # the directions ARE unit for normalize: what comes back as the shadow ray's direction has the bits that went in
    one_ray, one_mat = sh.upload(rd, plt, rays[:1]), sh.upload(rd, plt, mat[:1])
    for name, vecs in (("L", g["L"]), ("V", g["V"])):
        for at in range(0, vecs.shape[0], 5):
            scene = scene_of(vecs[at:at + 5])
            for k in range(min(5, vecs.shape[0] - at)):
                _, bSh = rd.LightHits(one_ray, one_mat, 1, scene, k)
                back = sh.read(rd, plt, bSh, 1, rd.RAY_DTYPE)["direction"][0]
                assert np.array_equal(bits(back), bits(vecs[at + k])), "%s[%d] is not left alone by normalize" % (name, at + k)
    lit = np.zeros((n, 3), F)
    for li in range(se.N_BRDF_L):
        rows = np.flatnonzero(g["l"] == li)
        scene = scene_of([g["L"][li]])
        bL, bSh = rd.LightHits(sh.upload(rd, plt, rays[rows]), sh.upload(rd, plt, mat[rows]), rows.shape[0], scene, 0)
        out = sh.read(rd, plt, bL, rows.shape[0], mc.LIT_DTYPE)
        shadow = sh.read(rd, plt, bSh, rows.shape[0], rd.RAY_DTYPE)
        assert (bits(shadow["direction"]) == bits(g["L"][li])).all() and not bits(out["w"]).any()
        lit[rows] = out["rgb"]
    with np.errstate(invalid="ignore"):
        want = (np.zeros(3, F) + G["brdf"]).astype(F)
    ok = compare(lit, want)[0]
    assert ok.all(), "lit differs from 0 + microfacetBRDF on %d of %d rows (first: row %d, got %r, want %r)" % (
        int((~ok).sum()), n, int(np.flatnonzero(~ok)[0]), lit[~ok][0].tolist(), want[~ok][0].tolist())
    report("d", n, want, 0, how)


# ---- e. rd.TracePaths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", (1, 4))
def test_e_trace_paths_on_the_edge_rays(mods, ctx, depth):
    rd, _ = mods
    c = ctx
    for name in ("main", "s-25", "s+25", "keys"):
        rays, keys = c.rays(name), c.keys(name)
        want, counts, first = pc.public_loop(rd, c.plt, c.tlas, c.sb(0), rays, keys, depth)
        got, hits = pc.trace_paths(rd, c.plt, c.tlas, c.sb(0), rays, keys, depth)
        ok = compare(got, want)[0]
        assert ok.all(), "%s, depth %d: radiance differs from the loop over the public calls on %d of %d rays (first: %s)" % (
            name, depth, int((~ok).sum()), ok.shape[0], np.flatnonzero(~ok)[:8].tolist())
        assert np.array_equal(np.ascontiguousarray(hits).view(np.uint8), np.ascontiguousarray(first).view(np.uint8))
        report("e/%s depth %d" % (name, depth), rays.shape[0], want[:, :3], 0, "against the fold of rd.QueryRays / rd.ShadeHits, counts %s" % counts)


# ---- f. the frame path ------------------------------------------------------------------------------------------------------------------
def test_f_frames_of_the_edge_scene(mods, ctx, G, live):
    rd, _ = mods
    c = ctx
    how = check_live(G, live, "frame/")
    dev = c.dev
    dev.bind()
    dev.set_rtprop(totalSamples=0); dev.clear_scratch()
    try:
        for f in range(2):
            img = dev.render()
            want = G["frame/scratch%d" % f].reshape(-1, 4)
            ok = compare(dev.read_scratch().reshape(-1, 4), want)[0]
            assert ok.all(), "frame %d: imageScratch differs on %d of %d pixels (first: %s)" % (f, int((~ok).sum()), ok.shape[0], np.flatnonzero(~ok)[:8].tolist())
            eq = (img.reshape(-1, 4) == G["frame/image%d" % f].reshape(-1, 4)).all(1)
            assert eq.all(), "frame %d: the image differs on %d pixels" % (f, int((~eq).sum()))
            report("f/frame %d" % f, want.shape[0], want[:, :3], 0, how)
    finally:
        dev.set_rtprop(totalSamples=0); dev.clear_scratch()


# ---- g. the tone map and the running mean ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tone(mods):
    rd, scenes = mods
    return scenes.DeviceScene(se.tone_scene(scenes))


@pytest.mark.parametrize("debug", (0, 1))
def test_g_tone_map(mods, tone, G, live, debug):
    rd, _ = mods
    how = check_live(G, live, "tone/")
    plt, n = tone.plt, se.TONE_NPIX
    frame = se.tone_frame(bool(debug))
    want = G["tone/image%d" % debug].reshape(n, 4)
    scratch, image = sh.upload(rd, plt, np.full((n, 4), 3.0, F)), sh.upload(rd, plt, np.zeros(4 * n, np.uint8))
    assert rd.Accumulate(sh.upload(rd, plt, frame), n, 0, scratch, image, debug=bool(debug)) == 0
    got = rd.ReadBuffer(plt, image, 4 * n).reshape(n, 4)
    eq = (got == want).all(1)
    assert eq.all(), "rd.Accumulate: %d pixels differ (first: pixel %d, mean %r, got %r, want %r)" % (
        int((~eq).sum()), int(np.flatnonzero(~eq)[0]), frame[~eq][0].tolist(), got[~eq][0].tolist(), want[~eq][0].tolist())
    sc = rd.ReadBuffer(plt, scratch, 16 * n).view(F).reshape(n, 4)
    assert compare(sc[:, :3], frame[:, :3])[0].all() and (bits(sc[:, 3]) == bits(F(3.0))).all()       # frame 0: the colour; w kept
    # the frame path at the same RTProp: the tone map alone, imageScratch untouched
    tone.bind()
    tone.set_rtprop(totalSamples=0, batchSize=0, depth=0, debug=debug)
    rd.WriteBuffer(plt, tone.rdImageScratch, 16 * n, frame)
    rd.TraceRays(plt, 0, 0, 0, n, 1)
    got = rd.ReadBuffer(plt, tone.rdImage, 4 * n).reshape(n, 4)
    eq = (got == want).all(1)
    assert eq.all(), "rd.TraceRays: %d pixels differ (first: pixel %d)" % (int((~eq).sum()), int(np.flatnonzero(~eq)[0]))
    assert np.array_equal(bits(tone.read_scratch().reshape(-1)), bits(frame.reshape(-1)))
    report("g/tone debug %d" % debug, n, frame[:, :3], 0, how)


@pytest.mark.parametrize("frame_id", se.FRAME_IDS)
def test_g_running_mean(mods, tone, G, live, frame_id):
    rd, _ = mods
    how = check_live(G, live, "mean/")
    plt, n = tone.plt, se.TONE_NPIX
    start = se.mean_frame()
    want, want_img = G["mean/%d" % frame_id], G["mean/image%d" % frame_id].reshape(n, 4)
    scratch, image = sh.upload(rd, plt, start), sh.upload(rd, plt, np.zeros(4 * n, np.uint8))
    assert rd.Accumulate(sh.upload(rd, plt, np.zeros((n, 4), F)), n, frame_id, scratch, image) == 0
    sc = rd.ReadBuffer(plt, scratch, 16 * n).view(F).reshape(n, 4)
    ok = compare(sc[:, :3], want)[0]
    assert ok.all(), "rd.Accumulate, frame %d: %d pixels differ (first: pixel %d, was %r, got %r, want %r)" % (
        frame_id, int((~ok).sum()), int(np.flatnonzero(~ok)[0]), start[~ok][0].tolist(), sc[~ok][0].tolist(), want[~ok][0].tolist())
    assert np.array_equal(bits(sc[:, 3]), bits(start[:, 3]))
    assert (rd.ReadBuffer(plt, image, 4 * n).reshape(n, 4) == want_img).all()
    tone.bind()
    tone.set_rtprop(totalSamples=frame_id, batchSize=1, depth=0, debug=0)
    rd.WriteBuffer(plt, tone.rdImageScratch, 16 * n, start)
    rd.TraceRays(plt, 0, 0, 0, n, 1)
    sc = tone.read_scratch().reshape(n, 4)
    ok = compare(sc[:, :3], want)[0]
    assert ok.all(), "rd.TraceRays, totalSamples %d: %d pixels differ (first: pixel %d)" % (frame_id, int((~ok).sum()), int(np.flatnonzero(~ok)[0]))
    assert np.array_equal(bits(sc[:, 3]), bits(start[:, 3]))
    assert (rd.ReadBuffer(plt, tone.rdImage, 4 * n).reshape(n, 4) == want_img).all()
    report("g/mean frame %d" % frame_id, n, want, 0, how)


# ---- h. rd.GenerateRays ------------------------------------------------------------------------------------------------------------------
def test_h_generate_rays_of_every_camera(mods, ctx, G, live):
    rd, _ = mods
    plt = ctx.plt
    how = check_live(G, live, "cam/")
    cams, n = se.cameras(rd), se.N_CAMERA_RAYS
    seeds = np.zeros(n, rd.RAYGEN_SEED_DTYPE)
    seeds["in"] = se.camera_seeds()
    bSeeds = sh.upload(rd, plt, seeds)
    assert G["cam/o"].shape == (len(cams), n, 3)
    all_nan = []
    for k, (name, cam) in enumerate(cams):
        rays, _ = rd.GenerateRays(sh.upload(rd, plt, np.array(cam).reshape(1)), n, 5, 3, seeds=bSeeds, keys=None)
        got = sh.read(rd, plt, rays, n, rd.RAY_DTYPE)
        for f, want in (("origin", G["cam/o"][k]), ("direction", G["cam/d"][k])):
            ok = compare(got[f], want)[0]
            assert ok.all(), "camera %s: %s differs on %d of %d rays (first: ray %d, got %r, want %r)" % (
                name, f, int((~ok).sum()), n, int(np.flatnonzero(~ok)[0]), got[f][~ok][0].tolist(), want[~ok][0].tolist())
        assert (bits(got["tmin"]) == bits(F(0.001))).all() and (bits(got["tmax"]) == bits(F(1000.0))).all()
        if se.nan_rows(G["cam/o"][k], G["cam/d"][k]).all():
            all_nan.append(name)
    assert set(all_nan) <= set(se.MAY_BE_ALL_NAN)
    report("h", len(cams) * n, np.concatenate([G["cam/o"], G["cam/d"]], 2), 0, "%s; all-NaN cameras: %s" % (how, all_nan))

"""GPU suite (-m gpu): the environment calls of radiance_ray_tracing_amd.env (rdx_env_build, rdx_env_light_hits, rdx_env_lookup,
rdx_trace_paths_env) -- a lat-long image that lights the scene, importance-sampled at one direction per hit.

The reference has no environment light.  Comparands, in this order of authority:
  1. env_cases.build_table: the table's bytes from numpy.cumsum, byte for byte (rowCos taken from the table under test and held
     separately to numpy's cosine within 1 ulp);
  2. env_cases.sampled_env: x, y, fx, fy, q, E and the dark rule in numpy, one IEEE operation at a time -- E with equal bits; the
     direction L = (st cos phi, ct, st sin phi) within 2^-20 of numpy's and of unit length (DESIGN 4.16's bound, for OCML's sinf /
     cosf in the place of v_rsq_f32);
  3. rd.LightHits (tests/test_gpu_materials.py holds it to the reference's recorded payloads) on the DirLight {-L, E}: that call
     normalises L once more, which may move its last place.  Where it does not, `lit` has equal bits; for the other rows the bar is
     LIT_REL, measured on these fixed rows, gated at 4 times that;
  4. area_cases.randoms_of, pcg3d in numpy: the keys route is the randoms route on it;
  5. rd.QueryRays for what the shadow interval does;
  6. env_cases.public_loop_env, the README's loop over the per-hit calls, for the path call.
The per-hit tests run on the 2048 recorded primary rays of c1 and c2, the path tests on paths_cases.arbitrary_batch (n = 2048 + 37)
with the seeds of test_gpu_paths.py, at depth 4.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import area_cases as ar
import env_cases as ec
import light_paths_cases as lp
import material_cases as mc
import paths_cases as pc
import punctual_cases as pu
import scatter_cases as sc
import shade_cases as sh
from test_gpu_paths import DEFAULTS, SEED, scene_box

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
DEPTH = 4
N_PATHS = 2048 + 37
COUNTS = ((0, 0), (3, 2), (15, 0))        # (punctual, area) records beside the environment
EPS = 2.0 ** -20
SKY = (64, 32)
SUN = (0.3, 0.8, 0.52)
# the largest per-channel relative difference between `lit` and rd.LightHits on the DirLight {-L, E} over the lit rows of c1 and c2
# whose shadow direction rd.LightHits moved by normalising it again, as measured on an MI355X (the rows are deterministic; the
# gate is 4 times this and only covers a rebuilt toolchain)
LIT_REL = 1.68e-5        # measured: 1.6780e-05 (173 moved rows of 3968; the other 3795 have equal bits)
same = mc.same


@pytest.fixture(scope="module")
def mods(gpu):
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import env, rd, scenes
    return rd, scenes, env


@pytest.fixture(scope="module")
def golden(mods):
    rd, scenes, _ = mods
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = sh.Golden(rd, scenes, name)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def sky(mods, golden):
    """the 64 x 32 procedural sky on the device, its table read back once"""
    rd, _, env = mods
    plt = golden("c1").dev.plt
    image = env.ProceduralSky(SKY[0], SKY[1], SUN)
    e = env.CreateEnvironment(plt, image)
    return dict(e=e, image=image, parts=ec.parts(ec.read_table(rd, plt, e), *SKY))


@pytest.fixture(scope="module")
def recs(mods, golden, sky):
    """per golden scene: the material records of its 2048 recorded primary rays, resolved once and left unchanged, and the
    environment call on them (keys route, stream 0) with numpy's restatement beside it"""
    rd, _, env = mods
    cache = {}

    def get(name):
        if name not in cache:
            g = golden(name)
            r = sc.records(rd, g.dev, g.mat_rays)
            r["keys"] = g.keys
            r["w"] = ec.env_batch(rd, env, g.dev.plt, g.dev.topAccelStruct, r["bR"], r["bM"], r["n"], sky["e"], keys=g.keys, stream=0)
            rnd = ar.randoms_of(g.keys["frameID"], g.keys["pixel"], g.keys["depth"], 0)["xyz"]
            r["s"] = ec.sampled_env(sky["image"], sky["parts"], rnd[:, 0], rnd[:, 1], rnd[:, 2])
            cache[name] = r
        return cache[name]
    return get


# ---- 1. the table's bytes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ((1, 1), (8, 4), (37, 19), (64, 32), (257, 3), (1024, 512), (16384, 1)), ids=lambda s: "%dx%d" % s)
def test_the_table_is_numpys(mods, golden, size):
    """rdx_env_build's table equals env_cases.build_table byte for byte, for an image with a sun, a zero row and NaN / inf / negative
    texels and for a black one, at non-zero offsets in buffers filled with 0xA5 of which nothing else changes"""
    rd, _, env = mods
    plt = golden("c1").dev.plt
    W, H = size
    nbytes, off_i, off_t, tail = ec.layout(W, H)["size"], 48, 112, 80
    assert nbytes == env.TableSize(W, H)
    for kind, image in (("hostile", ec.hostile_sky(W, H, 7 + W)), ("black", np.zeros((H, W, 4), F))):
        bI, bT = rd.CreateBuffer(plt, off_i + image.nbytes + tail), rd.CreateBuffer(plt, off_t + nbytes + tail)
        for b in (bI, bT):
            rd.WriteBuffer(plt, b, b.size, np.full(b.size, 0xA5, np.uint8))
        rd.WriteBuffer(plt, bI, image.nbytes, image, offset=off_i)
        before = rd.ReadBuffer(plt, bI, bI.size).copy()
        e = env.BuildEnvironment(bI, W, H, bT, image_offset=off_i, table_offset=off_t)
        assert (e.image, e.table, e.width, e.height, e.image_offset, e.table_offset) == (bI, bT, W, H, off_i, off_t)
        got = rd.ReadBuffer(plt, bT, bT.size).copy()
        assert (got[:off_t] == 0xA5).all() and (got[off_t + nbytes:] == 0xA5).all() and np.array_equal(rd.ReadBuffer(plt, bI, bI.size), before), kind
        table = got[off_t:off_t + nbytes]
        p = ec.parts(table, W, H)
        ec.check_row_cos(p["rowCos"], H)
        want = ec.build_table(image, p["rowCos"])
        differ = np.flatnonzero(table != want)
        if differ.size:          # say where: the first texels whose quantised weight differs
            pw = ec.parts(want, W, H)
            q_got, q_want = (np.diff(np.concatenate([np.zeros((H, 1), np.int64), t["C"].astype(np.int64)], 1), axis=1) for t in (p, pw))
            print(kind, size, [(tuple(a), int(q_got[tuple(a)]), int(q_want[tuple(a)]), image[tuple(a)].tolist()) for a in np.argwhere(q_got != q_want)[:6]])
        assert differ.size == 0, (kind, size, differ[:8].tolist(), ec.layout(W, H))
        if kind == "black":
            assert p["header"]["total"] == 0 and not p["C"].any()
        else:
            assert p["header"]["total"] == p["M"][-1] > 0 and p["header"]["wmax"] > 0
        # built again, the same bytes: nothing is left over from the first build
        env.BuildEnvironment(bI, W, H, bT, image_offset=off_i, table_offset=off_t)
        assert np.array_equal(rd.ReadBuffer(plt, bT, bT.size), got), kind


# ---- 2. E, L and lit ---------------------------------------------------------------------------------------------------------------------
def test_e_l_and_lit(mods, golden, recs, sky):
    rd, _, env = mods
    worst, moved_rows, exact_rows = 0.0, 0, 0
    for name in ("c1", "c2"):
        dev, rec = golden(name).dev, recs(name)
        plt, n, mat, w, s = dev.plt, rec["n"], rec["mat"], rec["w"], rec["s"]
        hit = mat["hit"] == 1
        dark = pu.is_dark(w)
        lit_rows = hit & ~s["dark"]
        assert np.array_equal(dark, ~lit_rows) and lit_rows.sum() >= 512, (name, int(lit_rows.sum()))
        assert (w["lit"].view(np.uint8).reshape(n, 16).any(1) <= ~dark).all() and (w["shadow"].view(np.uint8).reshape(n, 32).any(1) == ~dark).all()
        sd = w["shadow"][lit_rows]
        # the shadow ray: origin and tmin are rd.LightHits', the interval is the stock one, L is numpy's direction and of unit length
        assert same(sd["origin"], mat["above"][lit_rows]) and (sh.bits(sd["tmin"]) == sh.bits(F(0.001))).all() and (sh.bits(sd["tmax"]) == sh.bits(F(1000.0))).all()
        L64 = sd["direction"].astype(np.float64)
        assert np.abs(L64 - s["L"][lit_rows]).max() <= EPS and np.abs((L64 * L64).sum(1) - 1.0).max() <= EPS, name
        assert same(sd["direction"][:, 1], s["ct"][lit_rows])
        # lit: ONE rd.LightHits call per row on the DirLight {-L, E}
        scene = rd.CreateBuffer(plt, 176)
        bL, bS = rd.CreateBuffer(plt, 16), rd.CreateBuffer(plt, 32)
        for i in np.flatnonzero(lit_rows):
            i = int(i)
            rd.WriteBuffer(plt, scene, 176, np.array(pu.as_dir_light(rd, -w["shadow"]["direction"][i], s["E"][i])).reshape(1))
            rd.LightHits(rec["bR"], rec["bM"], 1, scene, 0, lit=bL, shadow=bS, rays_offset=32 * i, materials_offset=64 * i)
            want_l, want_s = sh.read(rd, plt, bL, 1, mc.LIT_DTYPE)[0], sh.read(rd, plt, bS, 1, rd.RAY_DTYPE)[0]
            assert same(w["shadow"]["origin"][i], want_s["origin"])
            if same(w["shadow"]["direction"][i], want_s["direction"]):
                exact_rows += 1
                assert same(w["lit"][i], want_l), (name, i, w["lit"][i], want_l)       # E has sampled_env's bits
            else:
                moved_rows += 1
                a, b = w["lit"]["rgb"][i].astype(np.float64), want_l["rgb"].astype(np.float64)
                assert np.array_equal(b == 0, a == 0), (name, i, a, b)
                rel = np.abs(a - b)[b != 0] / np.abs(b[b != 0])
                worst = max(worst, float(rel.max()) if rel.size else 0.0)
        assert (w["lit"]["rgb"][lit_rows] != 0).any(1).sum() >= 256, name
        assert not w["lit"]["w"].any()
    print("lit: %d rows with rd.LightHits' shadow direction (equal bits), %d rows moved by its second normalize; largest relative difference %.3e (LIT_REL %.3e)"
          % (exact_rows, moved_rows, worst, LIT_REL))
    assert exact_rows >= 64
    assert worst <= 4 * LIT_REL, worst


# ---- 3. keys and randoms -----------------------------------------------------------------------------------------------------------------
def test_the_keys_route_is_the_randoms_route(mods, golden, recs, sky):
    rd, _, env = mods
    dev, rec = golden("c1").dev, recs("c1")
    plt, tlas, n, keys = dev.plt, dev.topAccelStruct, rec["n"], rec["keys"]
    seen = []
    for stream in (0, 1, 15, 0xfffe):
        by_keys = ec.env_batch(rd, env, plt, tlas, rec["bR"], rec["bM"], n, sky["e"], keys=keys, stream=stream, query=False)
        rnd = ar.randoms_of(keys["frameID"], keys["pixel"], keys["depth"], stream)
        by_randoms = ec.env_batch(rd, env, plt, tlas, rec["bR"], rec["bM"], n, sky["e"], randoms=rnd, query=False)
        assert same(by_keys["lit"], by_randoms["lit"]) and same(by_keys["shadow"], by_randoms["shadow"]), stream
        assert (~pu.is_dark(by_keys)).sum() >= 256, stream
        seen.append(by_keys)
    assert same(seen[0]["lit"], rec["w"]["lit"]) and same(seen[0]["shadow"], rec["w"]["shadow"])
    assert not same(seen[1]["shadow"], seen[2]["shadow"]) and not same(seen[0]["shadow"], seen[3]["shadow"])      # another stream, other directions
    lit_only, none = env.EnvLightHits(rec["bR"], rec["bM"], n, sky["e"], keys=sh.upload(rd, plt, keys), stream=1, shadow=None)
    assert none is None and same(sh.read(rd, plt, lit_only, n, mc.LIT_DTYPE), seen[1]["lit"])
    # a caller's own randoms outside [0, 1] and NaN are held to the table's ends
    wild = sc.randoms_of(np.tile(np.array([[7.0, -3.0, 0.5], [np.nan, np.nan, 0.5], [np.inf, 1.0, 0.25], [-0.0, 2.0, 0.75]], F), (n // 4, 1)))
    got = ec.env_batch(rd, env, plt, tlas, rec["bR"], rec["bM"], n, sky["e"], randoms=wild, query=False)
    s = ec.sampled_env(sky["image"], sky["parts"], wild["xyz"][:, 0], wild["xyz"][:, 1], wild["xyz"][:, 2])
    rows = ~pu.is_dark(got)
    assert rows.sum() >= 256 and same(got["shadow"]["direction"][rows][:, 1], s["ct"][rows])


# ---- 4. lookup ---------------------------------------------------------------------------------------------------------------------------
def test_the_lookup_returns_the_texel(mods, golden, recs, sky):
    rd, _, env = mods
    plt = golden("c1").dev.plt
    W, H = 37, 19
    image = ec.hostile_sky(W, H, 3)
    e = env.CreateEnvironment(plt, image)
    p = ec.parts(ec.read_table(rd, plt, e), W, H)
    d = ec.texel_centres(p, W, H)
    scale = np.random.default_rng(4).uniform(0.01, 50.0, d.shape[0])[:, None]          # the direction need not be of unit length
    got = ec.lookup(rd, env, plt, e, sh.rays_of(rd, np.zeros_like(d), d * scale))
    want = image.reshape(-1, 4).copy()
    want[:, 3] = 0
    assert same(got, want)
    y, x = ec.lookup_texel(p, W, H, d)
    assert np.array_equal(y * W + x, np.arange(W * H))
    # zero and non-finite directions show nothing
    bad = np.array([[0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 1], [0, -np.inf, 0], [-0.0, 0.0, -0.0]], F)
    assert not ec.lookup(rd, env, plt, e, sh.rays_of(rd, np.zeros_like(bad), bad)).view(np.uint8).any()
    poles = np.array([[0, 1, 0], [0, -1, 0], [0, 1e-30, 0], [1e30, 0, 0]], F)
    got = ec.lookup(rd, env, plt, e, sh.rays_of(rd, np.zeros_like(poles), poles))
    assert same(got[0, :3], image[0, 0, :3]) and same(got[1, :3], image[H - 1, 0, :3]) and same(got[2, :3], image[0, 0, :3])
    # the call's own shadow directions show the texel they were drawn from
    left_out = total = 0
    for name in ("c1", "c2"):
        rec = recs(name)
        w, s = rec["w"], rec["s"]
        rows = ~pu.is_dark(w)
        got = ec.lookup(rd, env, plt, sky["e"], w["shadow"])
        inner = rows & (s["fx"] >= 0.01) & (s["fx"] <= 0.99) & (s["fy"] >= 0.01) & (s["fy"] <= 0.99)
        assert same(got[inner, :3], sky["image"][s["y"][inner], s["x"][inner], :3]), name
        assert not got[~rows].view(np.uint8).any()              # a dark record's shadow direction is zero
        left_out += int((rows & ~inner).sum())
        total += int(rows.sum())
    print("lookup: %d of %d lit rows lie within 0.01 of a texel edge and are left out (%.1f %%)" % (left_out, total, 100.0 * left_out / total))
    assert left_out <= 0.10 * total


# ---- 5. occlusion ------------------------------------------------------------------------------------------------------------------------
def test_occlusion_is_the_stock_interval(mods, golden, recs):
    rd, _, env = mods
    for name in ("c1", "c2"):
        dev, rec = golden(name).dev, recs(name)
        plt, tlas, w = dev.plt, dev.topAccelStruct, rec["w"]
        rows = ~pu.is_dark(w)
        far = w["shadow"][rows]
        q = sh.read(rd, plt, rd.QueryRays(tlas, sh.upload(rd, plt, far), far.shape[0], rd.QUERY_CLOSEST), far.shape[0], rd.RAY_HIT_DTYPE)
        occluded = w["occluded"][rows]
        assert np.array_equal(occluded, (q["hit"] == 1) & (q["t"] < F(1000.0))), name
        assert not w["occluded"][~rows].any()
        print("%s: %d lit rows, %d occluded, %d open to the sky" % (name, int(rows.sum()), int(occluded.sum()), int((~occluded).sum())))
        if name == "c2":        # its nave is open to the sky
            assert occluded.sum() >= 64 and (~occluded).sum() >= 64


# ---- 6. the path call is the loop ----------------------------------------------------------------------------------------------------
class PathCase:
    """one golden scene: the arbitrary batch of 2048 + 37 paths, the two tables, the sky, and per pair of table sizes the answer of
    the README's loop over the per-hit calls, computed once and left unchanged"""

    def __init__(self, rd, env, dev, name, sky):
        self.rd, self.env, self.dev, self.plt, self.tlas, self.sky = rd, env, dev, dev.plt, dev.topAccelStruct, sky
        plt, tlas = self.plt, self.tlas

        def first_t(rays):
            h = sh.read(rd, plt, rd.QueryRays(tlas, sh.upload(rd, plt, rays), rays.shape[0], rd.QUERY_CLOSEST), rays.shape[0], rd.RAY_HIT_DTYPE)
            return h["hit"] == 1, h["t"]
        lo, hi = scene_box(rd, dev)
        self.rays, self.keys, _ = pc.arbitrary_batch(rd, lo, hi, first_t, SEED[name], n=N_PATHS)
        self.n = self.rays.shape[0]
        self.sp = lp.five_lights(rd)
        self.scene = lp.scene_buffer(rd, plt, self.sp)
        self.sb = lp.buffers_with_scene(rd, dev, self.scene)
        self.table = pu.mixed_table(rd, lo, hi, self.sp, SEED[name])
        self.area = ar.area_table(rd, lo, hi, SEED[name])
        self._want = {}

    def want(self, counts, depth=DEPTH):
        if (counts, depth) not in self._want:
            self._want[(counts, depth)] = ec.public_loop_env(self.rd, self.env, self.plt, self.tlas, self.sb, self.dev.surface_buffers(), self.table[:counts[0]],
                                                             self.area[:counts[1]], self.sky["e"], self.rays, self.keys["frameID"], self.keys["pixel"], depth)
        return self._want[(counts, depth)]

    def run(self, counts, depth=DEPTH, e=None, rows=slice(None)):
        return ec.trace(self.rd, self.env, self.plt, self.tlas, self.sb, self.rays[rows], self.keys[rows], depth, self.table[:counts[0]], self.area[:counts[1]],
                        e or self.sky["e"])


@pytest.fixture(scope="module")
def paths(mods, golden, sky):
    rd, _, env = mods
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = PathCase(rd, env, golden(name).dev, name, sky)
        return cache[name]
    return get


def check_radiance(got, want_color, tag):
    eq = (sh.bits(got[:, :3]) == sh.bits(want_color)).all(1)
    assert eq.all(), "%s: radiance differs from the loop on %d of %d paths (first: %s)" % (tag, int((~eq).sum()), eq.shape[0], np.flatnonzero(~eq)[:8].tolist())
    assert not sh.bits(got[:, 3]).any(), "%s: radiance.w is not 0" % tag


@pytest.mark.parametrize("counts", COUNTS)
@pytest.mark.parametrize("name", ("c1", "c2"))
def test_the_path_call_is_the_loop(mods, paths, name, counts):
    rd, _, env = mods
    c = paths(name)
    color, lives, invalid, first_miss = c.want(counts)
    got, got_invalid = c.run(counts)
    bounce = rd.GetBounceCounts(DEPTH + 2).copy()
    st = rd.GetTraceStats()
    check_radiance(got, color, "%s, %d + %d records and the sky" % (name, counts[0], counts[1]))
    assert invalid == 0 and got_invalid == 0 and c.n == N_PATHS
    want_counts = np.zeros(DEPTH + 2, np.uint64)
    want_counts[0], want_counts[1:1 + len(lives)] = c.n, lives
    assert np.array_equal(bounce, want_counts), (bounce.tolist(), lives)
    assert len(lives) >= 2 and lives[1] >= 0.25 * c.n
    assert st.rays_shadow == (sum(counts) + 1) * sum(lives) and st.closest_hits == sum(lives)
    # primary misses show EnvLookup's bits, and the stock miss colour is gone
    assert first_miss.sum() >= 16
    look = ec.lookup(rd, env, c.plt, c.sky["e"], c.rays)
    assert same(got[first_miss], look[first_miss]) and look[first_miss, :3].any()
    assert not (sh.bits(got[first_miss, :3]) == sh.bits(sh.ENVIRONMENT)).all(1).any()
    # the sky matters: the same tables without it give other colours on the hits -- on many in c2, whose nave is open to the sky, on
    # few in c1, a closed room with windows
    without, _ = ar.trace(rd, c.plt, c.tlas, c.sb, c.rays, c.keys, DEPTH, c.table[:counts[0]], c.area[:counts[1]])
    changed = int((sh.bits(without[~first_miss, :3]) != sh.bits(got[~first_miss, :3])).any(1).sum())
    print("%s, %d + %d records: the sky changes %d of %d paths that hit" % (name, counts[0], counts[1], changed, int((~first_miss).sum())))
    assert changed >= (256 if name == "c2" else 16)


def test_chunks_do_not_matter(mods, paths):
    rd, _, env = mods
    c = paths("c2")
    rad, _ = c.run((3, 2))
    try:
        rd.SetOption("chunk_paths", 512)
        got, invalid = c.run((3, 2))
        st = rd.GetTraceStats()
    finally:
        rd.SetOption("chunk_paths", DEFAULTS["chunk_paths"])
    assert same(got, rad) and invalid == 0 and st.rays_primary == c.n and st.launches_extend >= 5
    check_radiance(got, c.want((3, 2))[0], "3 + 2 records and the sky in chunks of 512")


def test_the_image_and_table_are_read_by_every_call(mods, paths, sky):
    """another sky written over the image and built again into the same two buffers between two calls: the second call is the loop on
    the new environment.  rd.TraceAreaPaths on the same tables is the call it was"""
    rd, _, env = mods
    c = paths("c2")
    area_before, _ = ar.trace(rd, c.plt, c.tlas, c.sb, c.rays, c.keys, DEPTH, c.table[:3], c.area[:2])
    image = sky["image"].copy()
    e = env.CreateEnvironment(c.plt, image)
    first, _ = c.run((3, 2), e=e)
    check_radiance(first, c.want((3, 2))[0], "before the rewrite")
    evening = env.ProceduralSky(SKY[0], SKY[1], (-0.5, 0.3, 0.1), sun_radiance=(3000.0, 1500.0, 600.0), zenith=(0.3, 0.2, 0.5))
    rd.WriteBuffer(c.plt, e.image, evening.nbytes, evening)
    assert env.BuildEnvironment(e.image, SKY[0], SKY[1], e.table).table is e.table
    second, _ = c.run((3, 2), e=e)
    want = ec.public_loop_env(rd, env, c.plt, c.tlas, c.sb, c.dev.surface_buffers(), c.table[:3], c.area[:2], e, c.rays, c.keys["frameID"], c.keys["pixel"], DEPTH)[0]
    check_radiance(second, want, "after the rewrite")
    assert not same(first, second)
    area_after, _ = ar.trace(rd, c.plt, c.tlas, c.sb, c.rays, c.keys, DEPTH, c.table[:3], c.area[:2])
    assert same(area_before, area_after) and (sh.bits(area_after[:, :3]) == sh.bits(sh.ENVIRONMENT)).all(1).sum() >= 16


# ---- 7. small shapes, offsets, refusals, hostile tables ----------------------------------------------------------------------------------
def test_shapes(mods, golden, recs, paths, sky):
    """n in {0, 1, 63, 64, 65, 255, 256, 257} for the three calls: the rows of the full run.  max_depth 0 gives zeros"""
    rd, _, env = mods
    dev, rec = golden("c2").dev, recs("c2")
    plt, keys, full = dev.plt, rec["keys"], rec["w"]
    c = paths("c2")
    rad, _ = c.run((3, 2))
    look = ec.lookup(rd, env, plt, sky["e"], c.rays)
    first = 300
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        rows = slice(first, first + n)
        w = ec.env_batch(rd, env, plt, dev.topAccelStruct, rec["bR"], rec["bM"], n, sky["e"], keys=keys[rows] if n else np.zeros(1, keys.dtype), query=False,
                         rays_offset=32 * first, materials_offset=64 * first)
        assert same(w["lit"], full["lit"][rows]) and same(w["shadow"], full["shadow"][rows]), n
        got, invalid = c.run((3, 2), rows=rows)
        assert got.shape == (n, 4) and invalid == 0 and same(got, rad[rows]), n
        assert same(ec.lookup(rd, env, plt, sky["e"], c.rays[rows]), look[rows]), n
    dark = pu.is_dark(full)[first:first + 257]
    assert 0 < int(dark.sum()) < 257
    got, invalid = c.run((3, 2), depth=0)
    assert got.shape == (c.n, 4) and not got.view(np.uint8).any() and invalid == 0


def _refusals(rd, run, cases, snapshot, good, symbol):
    for what, kw, word in cases:
        with pytest.raises(rd.RadianceError) as err:
            run(**kw)
        assert word in str(err.value) and symbol in str(err.value), (what, str(err.value))
        now = snapshot()
        for k in now:
            assert np.array_equal(now[k], good[k]), (what, k)


def test_offsets_and_refusals(mods, golden, recs, paths, sky):
    """n = 200 records / paths of c1 at distinct non-zero offsets in buffers filled with 0xA5: the results are the plain calls' and no
    byte outside the written ranges changes; one refusal of each kind per call, after each of which every buffer is unchanged"""
    rd, _, env = mods
    dev, rec, c = golden("c1").dev, recs("c1"), paths("c1")
    plt, tl = dev.plt, dev.topAccelStruct
    W, H = SKY
    n, tail, lcount, acount = 200, 128, 3, 2
    tbytes = ec.layout(W, H)["size"]
    table, area = c.table[:lcount], c.area[:acount]
    hkeys = rec["keys"][:n]
    off = dict(rays=96, mat=192, table=128, area=64, image=80, etab=208, hkeys=48, rnd=80, lit=48, shadow=32, prays=64, keys=80, rad=112, look=16)
    size = dict(rays=32 * n, mat=64 * n, table=64 * lcount, area=64 * acount, image=16 * W * H, etab=tbytes, hkeys=16 * n, rnd=16 * n, lit=16 * n, shadow=32 * n,
                prays=32 * n, keys=16 * n, rad=16 * n, look=16 * n)
    B = {k: rd.CreateBuffer(plt, off[k] + size[k] + tail) for k in off}
    fill = lambda buf: rd.WriteBuffer(plt, buf, buf.size, np.full(buf.size, 0xA5, np.uint8))
    for buf in B.values():
        fill(buf)
    rnd = ar.randoms_of(hkeys["frameID"], hkeys["pixel"], hkeys["depth"], acount)
    for k, arr in (("rays", golden("c1").mat_rays[:n]), ("mat", rec["mat"][:n]), ("table", table), ("area", area), ("image", sky["image"]), ("hkeys", hkeys),
                   ("rnd", rnd), ("prays", c.rays[:n]), ("keys", c.keys[:n])):
        rd.WriteBuffer(plt, B[k], size[k], arr, offset=off[k])
    e = env.BuildEnvironment(B["image"], W, H, B["etab"], image_offset=off["image"], table_offset=off["etab"])
    assert np.array_equal(rd.ReadBuffer(plt, B["etab"], tbytes, offset=off["etab"]), ec.read_table(rd, plt, sky["e"]))
    snapshot = lambda: {k: rd.ReadBuffer(plt, B[k], B[k].size).copy() for k in B}

    def hits(**kw):
        a = dict(rays=B["rays"], materials=B["mat"], n=n, environment=e, keys=B["hkeys"], randoms=None, stream=acount, lit=B["lit"], shadow=B["shadow"],
                 rays_offset=off["rays"], materials_offset=off["mat"], keys_offset=off["hkeys"], randoms_offset=off["rnd"], lit_offset=off["lit"],
                 shadow_offset=off["shadow"])
        a.update(kw)
        return env.EnvLightHits(a.pop("rays"), a.pop("materials"), a.pop("n"), a.pop("environment"), **a)

    def look(**kw):
        a = dict(rays=B["prays"], n=n, environment=e, radiance=B["look"], rays_offset=off["prays"], radiance_offset=off["look"])
        a.update(kw)
        return env.EnvLookup(a.pop("rays"), a.pop("n"), a.pop("environment"), **a)

    def trace(**kw):
        a = dict(tlas=tl, rays=B["prays"], keys=B["keys"], n=n, max_depth=DEPTH, lights=B["table"], light_count=lcount, area=B["area"], area_count=acount,
                 environment=e, scene_buffers=c.sb, radiance=B["rad"], rays_offset=off["prays"], keys_offset=off["keys"], lights_offset=off["table"],
                 area_offset=off["area"], radiance_offset=off["rad"])
        a.update(kw)
        return env.TraceEnvPaths(a.pop("tlas"), a.pop("rays"), a.pop("keys"), a.pop("n"), a.pop("max_depth"), a.pop("lights"), a.pop("light_count"), a.pop("area"),
                                 a.pop("area_count"), a.pop("environment"), a.pop("scene_buffers"), **a)

    plain = ec.env_batch(rd, env, plt, tl, rec["bR"], rec["bM"], n, sky["e"], keys=hkeys, stream=acount, query=False)
    plain_rad, _ = c.run((lcount, acount), rows=slice(0, n))
    plain_look = ec.lookup(rd, env, plt, sky["e"], c.rays[:n])
    before = snapshot()
    assert hits() == (B["lit"], B["shadow"]) and trace() == (B["rad"], 0) and look() is B["look"]
    after = snapshot()
    for k in ("rays", "mat", "table", "area", "image", "etab", "hkeys", "rnd", "prays", "keys"):
        assert np.array_equal(after[k], before[k]), k
    for k, want in (("lit", plain["lit"]), ("shadow", plain["shadow"]), ("rad", plain_rad.reshape(-1)), ("look", plain_look.reshape(-1))):
        lo, hi = off[k], off[k] + size[k]
        assert same(after[k][lo:hi], want), k
        assert (after[k][:lo] == 0xA5).all() and (after[k][hi:] == 0xA5).all(), k
    assert plain["lit"]["rgb"].any() and plain_rad[:, :3].any()
    fill(B["lit"]); fill(B["shadow"])
    hits(keys=None, randoms=B["rnd"])                       # the randoms route at its offset is the keys route
    now = snapshot()
    assert same(now["lit"][off["lit"]:off["lit"] + size["lit"]], plain["lit"]) and same(now["shadow"][off["shadow"]:off["shadow"] + size["shadow"]], plain["shadow"])
    for k in ("lit", "shadow", "rad", "look"):             # n == 0 touches nothing
        fill(B[k])
    assert hits(n=0) == (B["lit"], B["shadow"]) and trace(n=0) == (B["rad"], 0) and look(n=0) is B["look"]
    assert all((rd.ReadBuffer(plt, B[k], B[k].size) == 0xA5).all() for k in ("lit", "shadow", "rad", "look"))
    hits(); trace(); look()
    good = snapshot()

    null, unknown = rd.Buffer(None, 1 << 20), rd.Buffer(12345678, 1 << 20)
    wrapped = lambda buf, shift, nbytes: rd.WrapDeviceMemory(plt, buf.device_ptr + shift, nbytes, keepalive=buf)
    E = lambda **kw: env.Environment(**dict(dict(image=B["image"], table=B["etab"], width=W, height=H, image_offset=off["image"], table_offset=off["etab"]), **kw))
    common = [
        ("an image offset that is no multiple of 16", dict(environment=E(image_offset=off["image"] + 8)), "16"),
        ("a table offset that is no multiple of 16", dict(environment=E(table_offset=off["etab"] + 4)), "16"),
        ("an image that overruns its buffer", dict(environment=E(image_offset=off["image"] + tail + 16)), "environment-image buffer"),
        ("a table that overruns its buffer", dict(environment=E(table_offset=off["etab"] + tail + 16)), "environment-table buffer"),
        ("a size larger than the buffers", dict(environment=E(width=2 * W)), "environment-image buffer"),
        ("null image", dict(environment=E(image=null)), "environment-image buffer handle"),
        ("unknown table", dict(environment=E(table=unknown)), "environment-table buffer handle"),
        ("a misaligned wrapped image", dict(environment=E(image=wrapped(B["image"], 8, 16 * W * H + 64), image_offset=0)), "aligned"),
        ("a misaligned wrapped table", dict(environment=E(table=wrapped(B["etab"], 4, tbytes + 64), table_offset=0)), "aligned"),
    ]
    _refusals(rd, hits, common + [
        ("lit over the image", dict(lit=B["image"], lit_offset=off["image"] + 64), "overlap"),
        ("shadow over the table", dict(n=1, shadow=B["etab"], shadow_offset=off["etab"] + tbytes - 32), "overlap"),
        ("keys_offset 8", dict(keys_offset=8), "16"), ("keys past the end", dict(keys_offset=off["hkeys"] + tail + 16), "key buffer"),
        ("unknown keys", dict(keys=unknown), "key buffer handle"),
        ("randoms past the end", dict(keys=None, randoms=B["rnd"], randoms_offset=off["rnd"] + tail + 16), "randoms buffer"),
        ("lit over the keys", dict(n=4, lit=B["hkeys"], lit_offset=off["hkeys"] + 48), "overlap"),
        ("rays_offset 8", dict(rays_offset=8), "16"), ("lit past the end", dict(lit_offset=off["lit"] + tail + 16), "lit buffer"),
        ("null rays", dict(rays=null), "ray buffer handle"), ("unknown shadow", dict(shadow=unknown), "shadow-ray buffer handle"),
    ], snapshot, good, "rdx_env_light_hits")
    _refusals(rd, look, common + [
        ("radiance over the image", dict(radiance=B["image"], radiance_offset=off["image"]), "overlap"),
        ("radiance over the table", dict(radiance=B["etab"], radiance_offset=off["etab"] + 64), "overlap"),
        ("rays_offset 8", dict(rays_offset=8), "16"), ("radiance past the end", dict(radiance_offset=off["look"] + tail + 16), "radiance buffer"),
        ("null rays", dict(rays=null), "ray buffer handle"), ("radiance over the rays", dict(radiance=B["prays"], radiance_offset=off["prays"]), "overlap"),
    ], snapshot, good, "rdx_env_lookup")
    _refusals(rd, trace, common + [
        ("radiance over the image", dict(radiance=B["image"], radiance_offset=off["image"] + 16 * W * H - 16, n=4), "overlap"),
        ("radiance over the table", dict(radiance=B["etab"], radiance_offset=off["etab"], n=4), "overlap"),
        ("radiance over the area table", dict(radiance=B["area"], radiance_offset=off["area"], n=4), "overlap"),
        ("null area", dict(area=null), "area-light-table buffer handle"), ("null lights", dict(lights=null), "light-table buffer handle"),
        ("max_depth 63", dict(max_depth=63), "63"), ("null tlas", dict(tlas=null), "TLAS"), ("keys_offset 4", dict(keys_offset=4), "16"),
        ("radiance past the end", dict(radiance_offset=off["rad"] + tail + 16), "radiance buffer"),
        ("null material", dict(scene_buffers=rd.ShadingBuffers(c.scene, dev.meshInfoData, dev.indexData, dev.uvData, dev.normalData, null)), "material"),
    ], snapshot, good, "rdx_trace_paths_env")
    # rdx_env_build: its own refusals leave the table as it was
    build = lambda **kw: env.BuildEnvironment(**dict(dict(image=B["image"], width=W, height=H, table=B["etab"], image_offset=off["image"], table_offset=off["etab"]), **kw))
    _refusals(rd, build, [
        ("image_offset 8", dict(image_offset=8), "16"), ("table_offset 4", dict(table_offset=4), "16"),
        ("a table that does not fit", dict(table_offset=off["etab"] + tail + 16), "environment-table buffer"),
        ("an image that does not fit", dict(width=2 * W, table=rd.CreateBuffer(plt, ec.layout(2 * W, H)["size"]), table_offset=0), "environment-image buffer"),
        ("the table over the image's first rows", dict(table=B["image"], table_offset=off["image"] + 16 * W), "overlap"),
        ("the table inside the image", dict(image=B["etab"], image_offset=0, width=4, height=2, table=B["etab"], table_offset=64), "overlap"),
        ("null image", dict(image=null), "environment-image buffer handle"), ("unknown table", dict(table=unknown), "environment-table buffer handle"),
    ], snapshot, good, "rdx_env_build")
    # what the wrappers refuse before the library sees it, at the C ABI: sizes, the sum rule, both / neither of keys and randoms, the stream
    from radiance_ray_tracing_amd import _lib
    L = _lib.lib()
    st = c.sb._struct()
    ea = (B["image"].handle, off["image"], B["etab"].handle, off["etab"])
    for w_, h_ in ((0, H), (W, 0), (16385, 1), (1, 8193), (0xffffffff, 0xffffffff)):
        assert L.rdx_env_build(ea[0], ea[1], w_, h_, ea[2], ea[3]) != 0 and "rdx_env_build" in _lib.last_error() and "outside" in _lib.last_error()
        assert L.rdx_env_lookup(B["prays"].handle, off["prays"], n, *ea, w_, h_, B["look"].handle, off["look"]) != 0 and "outside" in _lib.last_error()
        assert L.rdx_env_light_hits(B["rays"].handle, off["rays"], B["mat"].handle, off["mat"], n, *ea, w_, h_, B["hkeys"].handle, off["hkeys"], 0, None, 0, B["lit"].handle,
                                    off["lit"], None, 0) != 0 and "outside" in _lib.last_error()
        assert L.rdx_trace_paths_env(tl.handle, B["prays"].handle, off["prays"], B["keys"].handle, off["keys"], n, DEPTH, None, 0, 0, None, 0, 0, *ea, w_, h_, C.byref(st),
                                     B["rad"].handle, off["rad"], None) != 0 and "outside" in _lib.last_error()
    for lc, acnt in ((15, 1), (8, 8), (0, 16), (16, 0), (0xffffffff, 1), (1, 0xffffffff), (0x80000000, 0x80000000)):
        assert L.rdx_trace_paths_env(tl.handle, B["prays"].handle, off["prays"], B["keys"].handle, off["keys"], n, DEPTH, B["table"].handle, off["table"], lc,
                                     B["area"].handle, off["area"], acnt, *ea, W, H, C.byref(st), B["rad"].handle, off["rad"], None) != 0
        assert "area_count" in _lib.last_error() and "rdx_trace_paths_env" in _lib.last_error()
    raw_hits = lambda keys, stream, randoms: L.rdx_env_light_hits(B["rays"].handle, off["rays"], B["mat"].handle, off["mat"], n, *ea, W, H, keys, off["hkeys"], stream,
                                                                  randoms, off["rnd"], B["lit"].handle, off["lit"], B["shadow"].handle, off["shadow"])
    for keys, stream, randoms, word in ((B["hkeys"].handle, 0, B["rnd"].handle, "both"), (None, 0, None, "neither"), (B["hkeys"].handle, 0xffff, None, "stream"),
                                        (B["hkeys"].handle, 0xffffffff, None, "stream")):
        assert raw_hits(keys, stream, randoms) != 0
        assert word in _lib.last_error() and "rdx_env_light_hits" in _lib.last_error(), _lib.last_error()
    assert raw_hits(B["hkeys"].handle, 0xfffe, None) == 0          # the largest stream is accepted
    hits(); trace(); look()
    assert all(np.array_equal(v, good[k]) for k, v in snapshot().items())


def test_hostile_tables_give_no_fault(mods, golden, recs, paths, sky):
    """a table of random bytes and a table built for another size: zeros, the header is not the call's.  Random bytes under a header
    that IS the call's: unspecified colours -- every index formed from them is held inside the table and the image, and both searches
    end after log2 steps whatever they read -- and the library answers the next call as before"""
    rd, _, env = mods
    dev, rec, c = golden("c1").dev, recs("c1"), paths("c1")
    plt, tlas, n = dev.plt, dev.topAccelStruct, rec["n"]
    W, H = SKY
    tbytes = ec.layout(W, H)["size"]
    rng = np.random.default_rng(12)
    garbage = rng.integers(0, 256, tbytes, dtype=np.uint8)
    small = np.zeros(tbytes, np.uint8)
    other = env.CreateEnvironment(plt, env.ProceduralSky(W // 2, H // 2, SUN))
    small[:ec.layout(W // 2, H // 2)["size"]] = ec.read_table(rd, plt, other)
    for kind, bytes_ in (("random bytes", garbage), ("another size", small)):
        e = env.Environment(sky["e"].image, sh.upload(rd, plt, bytes_), W, H)
        w = ec.env_batch(rd, env, plt, tlas, rec["bR"], rec["bM"], n, e, keys=rec["keys"], query=False)
        assert not w["lit"].view(np.uint8).any() and not w["shadow"].view(np.uint8).any(), kind
        assert not ec.lookup(rd, env, plt, e, c.rays).view(np.uint8).any(), kind
        got, invalid = c.run((3, 2), e=e)
        plain, _ = ar.trace(rd, plt, c.tlas, c.sb, c.rays, c.keys, DEPTH, c.table[:3], c.area[:2])
        hit = ~c.want((3, 2))[3]
        assert invalid == 0 and same(got[hit], plain[hit]) and not got[~hit].view(np.uint8).any(), kind      # a dark record adds (0 + x) + 0
    hostile = garbage.copy()
    hd = np.zeros((), ec.HEADER_DTYPE)
    hd["magic"], hd["version"], hd["width"], hd["height"], hd["twoPiOverW"], hd["wOverTwoPi"] = ec.MAGIC, 1, W, H, 0.1, 10.0
    for total in (0xffffffffffffffff, 12345, 1):
        hd["total"] = total
        hostile[:64] = np.frombuffer(hd.tobytes(), np.uint8)
        e = env.Environment(sky["e"].image, sh.upload(rd, plt, hostile), W, H)
        w = ec.env_batch(rd, env, plt, tlas, rec["bR"], rec["bM"], n, e, keys=rec["keys"], query=False)
        assert w["lit"].shape == (n,) and not w["lit"][rec["mat"]["hit"] != 1].view(np.uint8).any()
        assert ec.lookup(rd, env, plt, e, c.rays).shape == (c.n, 4)
        got, invalid = c.run((0, 0), e=e, rows=slice(0, 300))
        assert got.shape == (300, 4) and invalid == 0
    again = ec.env_batch(rd, env, plt, tlas, rec["bR"], rec["bM"], n, sky["e"], keys=rec["keys"], query=False)
    assert same(again["lit"], rec["w"]["lit"]) and same(again["shadow"], rec["w"]["shadow"])


# ---- 8. torch tensors and the README's loop ------------------------------------------------------------------------------------------
_TORCH_CHILD = r"""
import os, sys
ROOT = sys.argv[1]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
assert torch.cuda.is_available()
torch.zeros(1, device="cuda").cpu()                      # torch initialises the GPU first (tests/test_cpu_oracle._gpu_present)
import numpy as np
import rrt_amd
from radiance_ray_tracing_amd import env, rd, scenes
import area_cases as ar
import env_cases as ec
import light_paths_cases as lp
import punctual_cases as pu
import scatter_cases as sc
import shade_cases as sh
from test_gpu_paths import scene_box
c = sh.Golden(rd, scenes, "c0")
dev, plt, tlas = c.dev, c.dev.plt, c.dev.topAccelStruct
sp = lp.five_lights(rd)
sb = lp.buffers_with_scene(rd, dev, lp.scene_buffer(rd, plt, sp))
sf = dev.surface_buffers()
lo, hi = scene_box(rd, dev)
table = pu.mixed_table(rd, lo, hi, sp, 3)[:2]
area = ar.area_table(rd, lo, hi, 3)[:3]
as_t = lambda a: torch.from_numpy(a.view(np.float32).reshape(-1, 16).copy()).cuda()
lights_t, area_t = as_t(table), as_t(area)
image = env.ProceduralSky(64, 32, (0.3, 0.8, 0.52))
sky = env.CreateEnvironment(plt, image)
sky_t = env.BuildEnvironmentTorch(torch.from_numpy(image).cuda())
assert np.array_equal(sky_t.keepalive[1].cpu().numpy(), ec.read_table(rd, plt, sky)) and (sky_t.width, sky_t.height) == (64, 32)
# ---- the per-hit call and the lookup, both routes
n = c.mat_rays.shape[0]
rec = sc.records(rd, dev, c.mat_rays)
t = torch.from_numpy(c.mat_rays.view(np.float32).reshape(n, 8).copy()).cuda()
mat0, _ = rd.ResolveMaterialsTorch(tlas, t, rd.QueryRaysTorch(tlas, t, rd.QUERY_CLOSEST), sb)
keys_t = torch.from_numpy(c.keys.view(np.int32).reshape(n, 4).copy()).cuda()
for stream in (0, 3):
    want = ec.env_batch(rd, env, plt, tlas, rec["bR"], rec["bM"], n, sky, keys=c.keys, stream=stream, query=False)
    lit, shadow = env.EnvLightHitsTorch(t, mat0, sky_t, keys=keys_t, stream=stream)
    assert lit.dtype == torch.float32 and tuple(lit.shape) == (n, 4) and tuple(shadow.shape) == (n, 8) and lit.is_cuda
    assert np.array_equal(lit.cpu().numpy().view(np.uint32), want["lit"].view(np.uint32).reshape(n, 4)), stream
    assert np.array_equal(shadow.cpu().numpy().view(np.uint32), want["shadow"].view(np.uint32).reshape(n, 8)), stream
    rnd_t = torch.from_numpy(ar.randoms_of(c.keys["frameID"], c.keys["pixel"], c.keys["depth"], stream).view(np.float32).reshape(n, 4).copy()).cuda()
    lit2, none = env.EnvLightHitsTorch(t, mat0, sky, randoms=rnd_t, want_shadow=False)
    assert none is None and torch.equal(lit2.view(torch.int32), lit.view(torch.int32))
    assert want["lit"]["rgb"].any()
look = env.EnvLookupTorch(t, sky_t)
assert np.array_equal(look.cpu().numpy().view(np.uint32), ec.lookup(rd, env, plt, sky, c.mat_rays).view(np.uint32))
e0 = env.EnvLightHitsTorch(t[:0], mat0[:0], sky_t, keys=keys_t[:0])
assert tuple(e0[0].shape) == (0, 4) and tuple(e0[1].shape) == (0, 8) and tuple(env.EnvLookupTorch(t[:0], sky_t).shape) == (0, 4)
# ---- the path call, and the README's fifth loop
cam = dev.frame_buffers()[0]
npix = dev.width * dev.height
max_depth, frame, total_samples = 3, 5, 4
rays, keys = rd.GenerateRaysTorch(cam, npix, frame, total_samples)
rn, kn = rays.cpu().numpy().view(rd.RAY_DTYPE).reshape(-1), keys.cpu().numpy().view(rd.SHADE_KEY_DTYPE).reshape(-1)
for L, A in ((0, 0), (0, 3), (2, 2)):
    want, invalid = ec.trace(rd, env, plt, tlas, sb, rn, kn, max_depth, table[:L], area[:A], sky)
    got = env.TraceEnvPathsTorch(tlas, rays, keys, max_depth, lights_t[:L] if L else None, area_t[:A] if A else None, sky_t, sb)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == (npix, 4) and got.is_cuda
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)) and invalid == 0 and want[:, :3].any(), (L, A)
call = env.TraceEnvPathsTorch(tlas, rays, keys, max_depth, lights_t, area_t, sky_t, sb)
n = npix
pixel = keys[:, 1].contiguous()
color = torch.zeros((n, 4), device="cuda")
weight = torch.ones((n, 3), device="cuda")
path = torch.arange(n, device="cuda")
for depth in range(max_depth):
    if depth:
        keys = torch.stack([torch.full_like(pixel, frame), pixel, torch.full_like(pixel, depth), torch.zeros_like(pixel)], 1).contiguous()
    hits = rd.QueryRaysTorch(tlas, rays, rd.QUERY_CLOSEST)
    surf, _ = rd.ResolveHitsTorch(tlas, rays, hits, sf)
    mat, _ = rd.ResolveMaterialsTorch(tlas, rays, hits, sb)
    if depth == 0:
        missed = mat.view(torch.int32)[:, 3] != 1
        color[path[missed], :3] = env.EnvLookupTorch(rays, sky_t)[missed, :3]
    direct = torch.zeros((rays.shape[0], 3), device="cuda")
    for j in range(lights_t.shape[0]):
        lit, shadow = rd.PunctualLightHitsTorch(rays, mat, lights_t, j)
        occluded = rd.QueryRaysTorch(tlas, shadow, rd.QUERY_ANY)[:, 3:4] == 1
        direct += torch.where(occluded, torch.zeros_like(lit[:, :3]), lit[:, :3])
    for j in range(area_t.shape[0]):
        lit, shadow = rd.AreaLightHitsTorch(rays, mat, area_t, j, keys=keys)       # stream = j
        occluded = rd.QueryRaysTorch(tlas, shadow, rd.QUERY_ANY)[:, 3:4] == 1
        direct += torch.where(occluded, torch.zeros_like(lit[:, :3]), lit[:, :3])
    lit, shadow = env.EnvLightHitsTorch(rays, mat, sky_t, keys=keys, stream=area_t.shape[0])
    occluded = rd.QueryRaysTorch(tlas, shadow, rd.QUERY_ANY)[:, 3:4] == 1
    direct += torch.where(occluded, torch.zeros_like(lit[:, :3]), lit[:, :3])
    radiance = direct + mat[:, 4:7] * 0.1
    scatter, rays, src, live = rd.ScatterHitsTorch(rays, mat, surf, keys)
    src = src.long()
    color[path[src], :3] += weight[path[src]] * radiance[src]
    weight[path[src]] *= scatter[src, 0:3]
    path, pixel = path[src], pixel[src].contiguous()
    if live == 0:
        break
assert torch.equal(color.view(torch.int32), call.view(torch.int32)), "the README's loop differs from env.TraceEnvPathsTorch"
rays, keys = rd.GenerateRaysTorch(cam, npix, frame, total_samples)
assert tuple(env.TraceEnvPathsTorch(tlas, rays[:0], keys[:0], max_depth, lights_t, area_t, sky_t, sb).shape) == (0, 4)
big = torch.zeros((14, 16), dtype=torch.float32, device="cuda")
rnd_t = torch.zeros((t.shape[0], 4), dtype=torch.float32, device="cuda")
bad = [lambda: env.TraceEnvPathsTorch(tlas, rays, keys, max_depth, lights_t, big, sky_t, sb), lambda: env.TraceEnvPathsTorch(tlas, rays, keys, max_depth, lights_t, area_t.double(), sky_t, sb),
       lambda: env.TraceEnvPathsTorch(tlas, rays, keys, max_depth, lights_t, area_t.cpu(), sky_t, sb), lambda: env.TraceEnvPathsTorch(tlas, rays, keys, max_depth, None, None, None, sb),
       lambda: env.TraceEnvPathsTorch(tlas, rays[:, :7], keys, max_depth, lights_t, area_t, sky_t, sb), lambda: env.TraceEnvPathsTorch(tlas, rays, keys[:-1], max_depth, lights_t, area_t, sky_t, sb),
       lambda: env.TraceEnvPathsTorch(tlas, rays, keys, -1, lights_t, area_t, sky_t, sb), lambda: env.TraceEnvPathsTorch(tlas, rays, keys, max_depth, lights_t, area_t, sky_t, (1, 2)),
       lambda: env.EnvLightHitsTorch(t, mat0, sky_t), lambda: env.EnvLightHitsTorch(t, mat0, sky_t, keys=keys_t, randoms=rnd_t),
       lambda: env.EnvLightHitsTorch(t, mat0, sky_t, keys=keys_t[:-1]), lambda: env.EnvLightHitsTorch(t, mat0, sky_t, keys=keys_t.float()),
       lambda: env.EnvLightHitsTorch(t, mat0, sky_t, randoms=rnd_t[:, :3]), lambda: env.EnvLightHitsTorch(t, mat0, sky_t, keys=keys_t, stream=0xffff),
       lambda: env.EnvLightHitsTorch(t.cpu(), mat0, sky_t, keys=keys_t), lambda: env.EnvLightHitsTorch(t, mat0[:-1], sky_t, keys=keys_t),
       lambda: env.EnvLookupTorch(t.double(), sky_t), lambda: env.EnvLookupTorch(t, image),
       lambda: env.BuildEnvironmentTorch(torch.zeros((4, 4, 3), device="cuda")), lambda: env.BuildEnvironmentTorch(torch.zeros((4, 4, 4), device="cuda").double())]
for j, fn in enumerate(bad):
    try:
        fn()
    except rd.RadianceError:
        continue
    raise AssertionError("bad argument set %d was accepted" % j)
print("TORCH-ENV-OK", npix)
"""


def test_torch_tensors_in_a_fresh_process(gpu):
    """the torch routes equal the Buffer routes bit for bit, and the README's fifth loop equals env.TraceEnvPathsTorch; a wrong dtype,
    shape or device is refused in Python.  torch is initialised first, in a process of its own (as tests/test_gpu_area.py)"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _TORCH_CHILD, ROOT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "TORCH-ENV-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])

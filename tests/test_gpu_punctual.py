"""GPU suite (-m gpu): rd.PunctualLightHits / rd.TracePunctualPaths and their torch routes (rdx_punctual_light_hits,
rdx_trace_paths_punctual) -- point and spot lights from a caller-owned light table, per hit and per path.

Comparands, in this order of authority:
  1. rd.LightHits (tests/test_gpu_materials.py holds it to the reference's recorded payloads): a directional record IS that call,
     and a point or spot record at a hit is that call on the DirLight {direction = -(position - above), color = E}, where E is
     punctual_cases.emitted -- the record's d2, att, cone factor and dark rule in numpy float32, one IEEE operation at a time.
     normalize3 is built on v_rsq_f32, so emitted takes the unit vectors from the call's own shadow records; they are held to
     numpy's v / |v| within 2^-20 (1 ulp of v_rsq_f32, three roundings in d2, one product);
  2. rd.QueryRays for what the shadow interval does;
  3. punctual_cases.public_loop_punctual, the README's loop over the per-hit call, for the path call; rd.TraceLightPaths for a
     table of directional records.
Every bar but the unit-length one is equality of bits.  The per-hit tests run on the 2048 recorded primary rays of c1 and c2, the
path tests on paths_cases.arbitrary_batch (n = 2048 + 37) with the seeds of test_gpu_paths.py, at depth 4.
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
import punctual_cases as pu
import scatter_cases as sc
import shade_cases as sh
from test_gpu_paths import DEFAULTS, SEED, scene_box

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
DEPTH = 4
N_PATHS = 2048 + 37
COUNTS = (0, 1, 5, 6, 16)
EPS = 2.0 ** -20
same = mc.same


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
def recs(mods, golden):
    """per golden scene: the geometry and material records of its 2048 recorded primary rays, resolved once and left unchanged"""
    rd, _ = mods
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = sc.records(rd, golden(name).dev, golden(name).mat_rays)
        return cache[name]
    return get


# the lights of tests 3 and 4, per scene: a point light, the same with a range, a spot
def scene_lights(rd, name):
    if name == "c1":       # the Cornell box: x, z in -3 .. 3, the ceiling at y = 6; the floor is farther than 4 from the light, the upper walls nearer
        return dict(point=pu.light(rd, pu.POINT, (0, 5.5, 0), color=(30.0, 28.0, 24.0)),
                    ranged=pu.light(rd, pu.POINT, (0, 5.5, 0), range=4.0, color=(30.0, 28.0, 24.0)),
                    spot=pu.light(rd, pu.SPOT, (0, 5.9, 0), (0, -1, 0), 0.0, (40.0, 40.0, 30.0), rd.SpotCone(np.radians(15.0), np.radians(35.0))))
    return dict(point=pu.light(rd, pu.POINT, (0, 4, 2), color=(60.0, 50.0, 40.0)),      # the atrium: x in -12 .. 12, y in 0 .. 9, z in -20 .. 20
                ranged=pu.light(rd, pu.POINT, (0, 4, 2), range=9.0, color=(60.0, 50.0, 40.0)),
                spot=pu.light(rd, pu.SPOT, (0, 8, 4), (0, -1, 0), 0.0, (90.0, 90.0, 70.0), rd.SpotCone(np.radians(25.0), np.radians(45.0))))


def spot_axis(rd, plt, rec, light):
    """S = normalize3(direction), from one rd.LightHits call with direction = -light.direction: its shadow rays point along S"""
    scene = sh.upload(rd, plt, np.array(pu.as_dir_light(rd, -np.ascontiguousarray(light["direction"], F), (1, 1, 1))).reshape(1))
    k = int(np.flatnonzero(rec["mat"]["hit"] == 1)[0])
    _, bSh = rd.LightHits(rec["bR"], rec["bM"], 1, scene, 0, rays_offset=32 * k, materials_offset=64 * k)
    return sh.read(rd, plt, bSh, 1, rd.RAY_DTYPE)["direction"][0].copy()


# ---- 1. directional records are rdx_light_hits ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c1", "c2"))
def test_directional_records_are_light_hits(mods, golden, recs, name):
    rd, _ = mods
    dev, rec = golden(name).dev, recs(name)
    plt, n = dev.plt, rec["n"]
    sp = lp.five_lights(rd)
    scene, bT = lp.scene_buffer(rd, plt, sp), sh.upload(rd, plt, pu.directional_table(rd, sp))
    for j in range(lp.N_LIGHTS):
        bL, bSh = rd.LightHits(rec["bR"], rec["bM"], n, scene, j)
        w = pu.punctual_batch(rd, plt, dev.topAccelStruct, rec["bR"], rec["bM"], n, bT, j, query=False)
        assert same(w["lit"], sh.read(rd, plt, bL, n, mc.LIT_DTYPE)), (name, j)
        assert same(w["shadow"], sh.read(rd, plt, bSh, n, rd.RAY_DTYPE)), (name, j)
        assert w["lit"]["rgb"].any()
        lit_only, none = rd.PunctualLightHits(rec["bR"], rec["bM"], n, bT, j, shadow=None)
        assert none is None and same(sh.read(rd, plt, lit_only, n, mc.LIT_DTYPE), w["lit"])


# ---- 2. point and spot, whole array, exact -------------------------------------------------------------------------------------------
def test_point_and_spot_at_one_point(mods, golden, recs):
    """c1's material records with `above` of every row overwritten by one point A: L and E are uniform, so ONE rd.LightHits call on
    the DirLight {-v, E} is the comparand of every row"""
    rd, _ = mods
    dev, rec = golden("c1").dev, recs("c1")
    plt, n = dev.plt, rec["n"]
    A = np.array([1.8, 1.0, 0.6], F)
    mat = rec["mat"].copy()
    hit = mat["hit"] == 1
    mat["above"][hit] = A
    bM = sh.upload(rd, plt, mat)
    lights = scene_lights(rd, "c1")
    for kind in ("point", "spot"):
        light = lights[kind]
        w = pu.punctual_batch(rd, plt, dev.topAccelStruct, rec["bR"], bM, n, sh.upload(rd, plt, pu.table(rd, [light])), 0, query=False)
        L = w["shadow"]["direction"][hit]
        assert hit.sum() >= 1024 and (sh.bits(L) == sh.bits(L[0])).all(), "L is not uniform"
        S = spot_axis(rd, plt, rec, light) if kind == "spot" else None
        e = pu.emitted(light, A.reshape(1, 3), L[0], S)
        assert not e["dark"][0]
        if kind == "spot":
            print("spot: f = %r at A" % float(e["f"][0]))
            assert 0.0 < e["f"][0] < 1.0, "A is not in the penumbra"
        v = (np.ascontiguousarray(light["position"], F) - A).astype(F)
        scene = sh.upload(rd, plt, np.array(pu.as_dir_light(rd, -v, e["E"][0])).reshape(1))
        bL, bSh = rd.LightHits(rec["bR"], bM, n, scene, 0)
        want_lit, want_sh = sh.read(rd, plt, bL, n, mc.LIT_DTYPE), sh.read(rd, plt, bSh, n, rd.RAY_DTYPE)
        assert same(w["lit"], want_lit), kind
        assert same(w["shadow"]["direction"], want_sh["direction"]) and same(w["shadow"]["origin"], want_sh["origin"]), kind
        assert same(w["shadow"]["tmin"], want_sh["tmin"]) and (sh.bits(w["shadow"]["tmax"][hit]) == sh.bits(np.sqrt(e["d2"][0]))).all(), kind
        assert not w["shadow"][~hit].view(np.uint8).any() and not w["lit"][~hit].view(np.uint8).any()
        assert (w["lit"]["rgb"][hit] != 0).any(1).sum() >= 256, "%s: the light shows on too few rows" % kind


# ---- 3. real `above`, sampled rows, exact --------------------------------------------------------------------------------------------
def classify(light, above, hit):
    """the classes of the rows by numpy alone (float64 directions): full, penumbra, dark_cone, dark_range; `unsure`: within 1e-4 of
    a cone edge, where the call's own L decides"""
    v = np.ascontiguousarray(light["position"], F)[None, :].astype(F) - above
    e = pu.emitted(light, above, np.zeros(3, F), np.zeros(3, F))          # d2 and the range rule are exact in numpy
    in_range = hit & (e["d2"] > 0) & ~((F(light["range"]) > 0) & ~(e["d2"] < F(light["range"]) * F(light["range"])))
    out = dict(dark_range=hit & ~in_range, unsure=np.zeros(hit.shape, bool))
    if int(light["type"]) == pu.SPOT:
        v64 = v.astype(np.float64)
        s64 = np.ascontiguousarray(light["direction"], np.float64)
        c = -(v64 / np.linalg.norm(v64, axis=1, keepdims=True)) @ (s64 / np.linalg.norm(s64))
        f = c * float(light["coneScale"]) + float(light["coneOffset"])
        out.update(unsure=in_range & ((np.abs(f) < 1e-4) | (np.abs(f - 1.0) < 1e-4)), full=in_range & (f >= 1.0 + 1e-4),
                   penumbra=in_range & (f > 1e-4) & (f < 1.0 - 1e-4), dark_cone=in_range & (f <= -1e-4))
    else:
        out["full"] = in_range
    return out, v


@pytest.mark.parametrize("name", ("c1", "c2"))
def test_real_hit_points_sampled_rows(mods, golden, recs, name):
    rd, _ = mods
    dev, rec = golden(name).dev, recs(name)
    plt, n, mat = dev.plt, rec["n"], rec["mat"]
    hit = mat["hit"] == 1
    rng = np.random.default_rng(11)
    scene = rd.CreateBuffer(plt, 176)
    expected = dict(point=("full",), ranged=("full", "dark_range"), spot=("full", "penumbra", "dark_cone"))
    for kind, light in scene_lights(rd, name).items():
        bT = sh.upload(rd, plt, pu.table(rd, [light]))
        w = pu.punctual_batch(rd, plt, dev.topAccelStruct, rec["bR"], rec["bM"], n, bT, 0, query=False)
        cls, v = classify(light, mat["above"], hit)
        print("%s %s: %s" % (name, kind, {k: int(m.sum()) for k, m in cls.items()}))
        for k in expected[kind]:
            assert cls[k].sum() >= 16, "%s %s: class %s has %d rows" % (name, kind, k, int(cls[k].sum()))
        dark = pu.is_dark(w)
        want_dark = ~hit | cls["dark_range"] | cls.get("dark_cone", np.zeros(n, bool))
        want_lit = cls["full"] | cls.get("penumbra", np.zeros(n, bool))
        assert dark[want_dark].all() and not dark[want_lit].any() and (want_dark | want_lit | cls["unsure"]).all(), (name, kind)
        # dark rows are 16 + 32 zero bytes (is_dark); a row is never half dark
        assert (w["lit"].view(np.uint8).reshape(n, 16).any(1) <= ~dark).all() and (w["shadow"].view(np.uint8).reshape(n, 32).any(1) == ~dark).all()
        lit_rows = ~dark
        S = spot_axis(rd, plt, rec, light) if kind == "spot" else None
        L = w["shadow"]["direction"]
        e = pu.emitted(light, mat["above"], L, S)
        assert not e["dark"][lit_rows].any() and e["dark"][dark & hit].all(), (name, kind)      # emitted on the call's own L agrees row for row
        assert (sh.bits(w["shadow"]["tmax"][lit_rows]) == sh.bits(np.sqrt(e["d2"][lit_rows]))).all()
        assert same(w["shadow"]["origin"][lit_rows], mat["above"][lit_rows]) and (sh.bits(w["shadow"]["tmin"][lit_rows]) == sh.bits(F(0.001))).all()
        L64, v64 = L[lit_rows].astype(np.float64), v[lit_rows].astype(np.float64)
        assert np.abs((L64 * L64).sum(1) - 1.0).max() <= EPS
        assert np.abs(L64 - v64 / np.linalg.norm(v64, axis=1, keepdims=True)).max() <= EPS
        if kind == "spot":
            assert (e["f"][cls["full"]] == 1).all() and ((e["f"][cls["penumbra"]] > 0) & (e["f"][cls["penumbra"]] < 1)).all()
        # 16 rows of every lit class: the construction of test 2 as an n = 1 rd.LightHits call
        for k in expected[kind]:
            if k.startswith("dark"):
                continue
            for i in rng.choice(np.flatnonzero(cls[k]), 16, replace=False):
                i = int(i)
                rd.WriteBuffer(plt, scene, 176, np.array(pu.as_dir_light(rd, -v[i], e["E"][i])).reshape(1))
                bL, bSh = rd.LightHits(rec["bR"], rec["bM"], 1, scene, 0, rays_offset=32 * i, materials_offset=64 * i)
                want_l, want_s = sh.read(rd, plt, bL, 1, mc.LIT_DTYPE), sh.read(rd, plt, bSh, 1, rd.RAY_DTYPE)
                assert same(w["lit"][i], want_l[0]), (name, kind, k, i, w["lit"][i], want_l[0])
                assert same(w["shadow"]["direction"][i], want_s["direction"][0]) and same(w["shadow"]["origin"][i], want_s["origin"][0]), (name, kind, k, i)
        assert (w["lit"]["rgb"][lit_rows] != 0).any(1).sum() >= 16, (name, kind)


# ---- 4. the interval does its work ---------------------------------------------------------------------------------------------------
def test_the_shadow_ray_ends_at_the_light(mods, golden, recs):
    """c1, the point light half a unit under the ceiling: a shadow ray reaches the ceiling behind the light only with the stock
    interval"""
    rd, _ = mods
    dev, rec = golden("c1").dev, recs("c1")
    plt, tlas, n = dev.plt, dev.topAccelStruct, rec["n"]
    w = pu.punctual_batch(rd, plt, tlas, rec["bR"], rec["bM"], n, sh.upload(rd, plt, pu.table(rd, [scene_lights(rd, "c1")["point"]])), 0)
    rows = ~pu.is_dark(w)
    assert rows.sum() >= 1024
    far = w["shadow"][rows].copy()
    far["tmax"] = 1000.0
    q = sh.read(rd, plt, rd.QueryRays(tlas, sh.upload(rd, plt, far), far.shape[0], rd.QUERY_CLOSEST), far.shape[0], rd.RAY_HIT_DTYPE)
    tmax, occluded = w["shadow"]["tmax"][rows], w["occluded"][rows]
    assert np.array_equal(occluded, (q["hit"] == 1) & (q["t"] < tmax))
    behind = (q["hit"] == 1) & (q["t"] >= tmax) & ~occluded
    print("shadow interval: %d rows, %d occluded, %d whose first hit lies behind the light" % (int(rows.sum()), int(occluded.sum()), int(behind.sum())))
    assert behind.sum() >= 64 and occluded.sum() >= 1 and not w["occluded"][~rows].any()


# ---- 5. the path call is the loop ----------------------------------------------------------------------------------------------------
class PathCase:
    """one golden scene: the arbitrary batch of 2048 + 37 paths, the mixed table, and per table size the answer of the README's loop
    over rd.PunctualLightHits, computed once and left unchanged"""

    def __init__(self, rd, dev, name):
        self.rd, self.dev, self.plt, self.tlas = rd, dev, dev.plt, dev.topAccelStruct
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
        self._want = {}

    def want(self, count, depth=DEPTH):
        if (count, depth) not in self._want:
            self._want[(count, depth)] = pu.public_loop_punctual(self.rd, self.plt, self.tlas, self.sb, self.dev.surface_buffers(), self.table[:count], self.rays,
                                                                 self.keys["frameID"], self.keys["pixel"], depth)
        return self._want[(count, depth)]

    def run(self, count, depth=DEPTH, sb=None, table=None):
        return pu.trace(self.rd, self.plt, self.tlas, sb or self.sb, self.rays, self.keys, depth, self.table[:count] if table is None else table)


@pytest.fixture(scope="module")
def paths(mods, golden):
    rd, _ = mods
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = PathCase(rd, golden(name).dev, name)
        return cache[name]
    return get


def check_radiance(got, want_color, tag):
    eq = (sh.bits(got[:, :3]) == sh.bits(want_color)).all(1)
    assert eq.all(), "%s: radiance differs from the loop on %d of %d paths (first: %s)" % (tag, int((~eq).sum()), eq.shape[0], np.flatnonzero(~eq)[:8].tolist())
    assert not sh.bits(got[:, 3]).any(), "%s: radiance.w is not 0" % tag


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", ("c1", "c2"))
def test_the_path_call_is_the_loop(mods, paths, name, count):
    rd, _ = mods
    c = paths(name)
    color, lives, invalid, _, dark0 = c.want(count)
    got, got_invalid = c.run(count)
    counts = rd.GetBounceCounts(DEPTH + 2).copy()
    check_radiance(got, color, "%s, %d records" % (name, count))
    assert invalid == 0 and got_invalid == 0 and c.n == N_PATHS
    want_counts = np.zeros(DEPTH + 2, np.uint64)
    want_counts[0], want_counts[1:1 + len(lives)] = c.n, lives
    assert np.array_equal(counts, want_counts), (counts.tolist(), lives)
    assert len(lives) >= 2 and lives[1] >= 0.25 * c.n
    print("%s, %d records: (dark, lit) depth-0 hits per record %s" % (name, count, dark0))
    if count:       # the table matters, and holds a record that is dark for part of the hits; from 5 records on the type-3 record
        assert (sh.bits(c.want(0)[0]) != sh.bits(color)).any(1).sum() >= 20
        assert any(d >= 16 and l >= 16 for d, l in dark0), dark0
        assert int(c.table["type"][0]) == pu.POINT and c.table["range"][0] > 0
    if count >= 5:
        assert int(c.table["type"][3]) == 3 and dark0[3][1] == 0 and dark0[3][0] == lives[0]


@pytest.mark.parametrize("name", ("c1", "c2"))
def test_five_directional_records_are_trace_light_paths(mods, paths, name):
    rd, _ = mods
    c = paths(name)
    want, invalid = lp.trace(rd, c.plt, c.tlas, c.sb, c.rays, c.keys, DEPTH, 5)
    got, got_invalid = c.run(5, table=pu.directional_table(rd, c.sp))
    assert same(got, want) and invalid == 0 and got_invalid == 0 and want[:, :3].any()


def test_chunks_do_not_matter(mods, paths):
    rd, _ = mods
    c = paths("c2")
    rad, _ = c.run(16)
    check_radiance(rad, c.want(16)[0], "defaults")
    try:
        rd.SetOption("chunk_paths", 512)
        got, invalid = c.run(16)
        st = rd.GetTraceStats()
        got5, _ = c.run(5)
    finally:
        rd.SetOption("chunk_paths", DEFAULTS["chunk_paths"])
    # 16 records: a chunk is 512 * 592 / (192 + 80 * 16) = 205 paths, eleven chunks; 5 records: 512 paths, five chunks
    assert same(got, rad) and invalid == 0 and st.rays_primary == c.n and st.launches_extend >= 11
    check_radiance(got5, c.want(5)[0], "5 records in chunks of 512")
    assert same(c.run(16)[0], rad)


def test_the_table_is_read_by_every_call(mods, paths):
    rd, _ = mods
    c = paths("c1")
    table = c.table[:3].copy()
    bT = sh.upload(rd, c.plt, table)
    bR, bK = sh.upload(rd, c.plt, c.rays), sh.upload(rd, c.plt, c.keys)
    run = lambda: rd.ReadBuffer(c.plt, rd.TracePunctualPaths(c.tlas, bR, bK, c.n, DEPTH, bT, 3, c.sb)[0], 16 * c.n).view(F).reshape(c.n, 4).copy()
    first = run()
    check_radiance(first, c.want(3)[0], "before the rewrite")
    table[0] = c.table[4]
    rd.WriteBuffer(c.plt, bT, table.nbytes, table)
    second = run()
    want = pu.public_loop_punctual(rd, c.plt, c.tlas, c.sb, c.dev.surface_buffers(), table, c.rays, c.keys["frameID"], c.keys["pixel"], DEPTH)[0]
    check_radiance(second, want, "after the rewrite")
    assert not same(first, second)


# ---- 6. shapes -------------------------------------------------------------------------------------------------------------------------
def test_shapes(mods, golden, recs, paths):
    """n in {0, 1, 63, 64, 65, 255, 256, 257} for both calls: the rows of the full run (c2: rows 300 .. hold hits, misses and dark
    rows; a path's radiance does not depend on the other paths of its call).  max_depth 0 gives zeros"""
    rd, _ = mods
    dev, rec = golden("c2").dev, recs("c2")
    plt = dev.plt
    light = scene_lights(rd, "c2")["ranged"]
    bT = sh.upload(rd, plt, pu.table(rd, [light]))
    full = pu.punctual_batch(rd, plt, dev.topAccelStruct, rec["bR"], rec["bM"], rec["n"], bT, 0, query=False)
    c = paths("c2")
    rad, _ = c.run(6)
    first = 300
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        rows = slice(first, first + n)
        bL, bSh = rd.PunctualLightHits(rec["bR"], rec["bM"], n, bT, 0, rays_offset=32 * first, materials_offset=64 * first)
        assert same(sh.read(rd, plt, bL, n, mc.LIT_DTYPE), full["lit"][rows]) and same(sh.read(rd, plt, bSh, n, rd.RAY_DTYPE), full["shadow"][rows]), n
        got, invalid = pu.trace(rd, plt, c.tlas, c.sb, c.rays[rows], c.keys[rows], DEPTH, c.table[:6])
        assert got.shape == (n, 4) and invalid == 0 and same(got, rad[rows]), n
    dark = pu.is_dark(full)[first:first + 257]
    assert 0 < int(dark.sum()) < 257 and (rec["mat"]["hit"][first:first + 257] == 1).sum() > int((~dark).sum()) > 0
    got, invalid = c.run(6, depth=0)
    assert got.shape == (c.n, 4) and not got.view(np.uint8).any() and invalid == 0


# ---- 7. offsets, refusals, fencing -----------------------------------------------------------------------------------------------------
def _refusals(rd, run, cases, snapshot, good, symbol):
    for what, kw, word in cases:
        with pytest.raises(rd.RadianceError) as e:
            run(**kw)
        assert word in str(e.value) and symbol in str(e.value), (what, str(e.value))
        now = snapshot()
        for k in now:
            assert np.array_equal(now[k], good[k]), (what, k)


def test_offsets_and_refusals(mods, golden, recs, paths):
    """n = 200 records / paths of c1 at distinct non-zero offsets in buffers filled with 0xA5: the results are the plain calls' and no
    byte outside the written ranges changes; one refusal of each new kind, after each of which every buffer is unchanged"""
    rd, _ = mods
    dev, rec, c = golden("c1").dev, recs("c1"), paths("c1")
    plt, tl = dev.plt, dev.topAccelStruct
    n, tail, count, index = 200, 128, 6, 4       # record 4: the point light without a range, lit on every hit
    table = c.table[:count]
    off = dict(rays=96, mat=192, table=128, lit=48, shadow=32, prays=64, keys=80, rad=112)
    size = dict(rays=32 * n, mat=64 * n, table=64 * count, lit=16 * n, shadow=32 * n, prays=32 * n, keys=16 * n, rad=16 * n)
    B = {k: rd.CreateBuffer(plt, off[k] + size[k] + tail) for k in off}
    fill = lambda buf: rd.WriteBuffer(plt, buf, buf.size, np.full(buf.size, 0xA5, np.uint8))
    for buf in B.values():
        fill(buf)
    for k, arr in (("rays", golden("c1").mat_rays[:n]), ("mat", rec["mat"][:n]), ("table", table), ("prays", c.rays[:n]), ("keys", c.keys[:n])):
        rd.WriteBuffer(plt, B[k], size[k], arr, offset=off[k])
    snapshot = lambda: {k: rd.ReadBuffer(plt, B[k], B[k].size).copy() for k in B}

    def hits(**kw):
        a = dict(rays=B["rays"], materials=B["mat"], n=n, lights=B["table"], index=index, lit=B["lit"], shadow=B["shadow"], rays_offset=off["rays"],
                 materials_offset=off["mat"], lights_offset=off["table"], lit_offset=off["lit"], shadow_offset=off["shadow"])
        a.update(kw)
        return rd.PunctualLightHits(a.pop("rays"), a.pop("materials"), a.pop("n"), a.pop("lights"), a.pop("index"), **a)

    def trace(**kw):
        a = dict(tlas=tl, rays=B["prays"], keys=B["keys"], n=n, max_depth=DEPTH, lights=B["table"], light_count=count, scene_buffers=c.sb, radiance=B["rad"],
                 rays_offset=off["prays"], keys_offset=off["keys"], lights_offset=off["table"], radiance_offset=off["rad"])
        a.update(kw)
        return rd.TracePunctualPaths(a.pop("tlas"), a.pop("rays"), a.pop("keys"), a.pop("n"), a.pop("max_depth"), a.pop("lights"), a.pop("light_count"),
                                     a.pop("scene_buffers"), **a)

    plain = pu.punctual_batch(rd, plt, tl, rec["bR"], rec["bM"], n, sh.upload(rd, plt, table), index, query=False)
    plain_rad, _ = pu.trace(rd, plt, tl, c.sb, c.rays[:n], c.keys[:n], DEPTH, table)
    before = snapshot()
    assert hits() == (B["lit"], B["shadow"]) and trace() == (B["rad"], 0)
    after = snapshot()
    for k in ("rays", "mat", "table", "prays", "keys"):
        assert np.array_equal(after[k], before[k]), k
    for k, want in (("lit", plain["lit"]), ("shadow", plain["shadow"]), ("rad", plain_rad.reshape(-1))):
        lo, hi = off[k], off[k] + size[k]
        assert same(after[k][lo:hi], want), k
        assert (after[k][:lo] == 0xA5).all() and (after[k][hi:] == 0xA5).all(), k
    assert plain["lit"]["rgb"].any() and plain_rad[:, :3].any()
    for k in ("lit", "shadow", "rad"):      # n == 0 touches nothing
        fill(B[k])
    assert hits(n=0) == (B["lit"], B["shadow"]) and trace(n=0) == (B["rad"], 0)
    assert all((rd.ReadBuffer(plt, B[k], B[k].size) == 0xA5).all() for k in ("lit", "shadow", "rad"))
    hits(); trace()
    good = snapshot()

    null, unknown = rd.Buffer(None, 1 << 20), rd.Buffer(12345678, 1 << 20)
    wrapped = lambda buf, shift, nbytes: rd.WrapDeviceMemory(plt, buf.device_ptr + shift, nbytes, keepalive=buf)
    room = rd.CreateBuffer(plt, 64 * count + 64 * n + 256)      # a table followed by room for an output, for the overlap cases
    rd.WriteBuffer(plt, room, 64 * count, table)
    room_good = rd.ReadBuffer(plt, room, room.size).copy()
    _refusals(rd, hits, [
        ("a light offset that is no multiple of 16", dict(lights_offset=off["table"] + 8), "16"),
        ("a record past the table's buffer", dict(index=count + 2), "light buffer"),
        ("a record that ends past the buffer", dict(lights=wrapped(B["table"], 0, off["table"] + 64 + 32), index=1), "light buffer"),
        ("null lights", dict(lights=null), "light buffer handle"), ("unknown lights", dict(lights=unknown), "light buffer handle"),
        ("lit over the light", dict(lights=room, lights_offset=0, index=1, lit=room, lit_offset=112), "overlap"),
        ("shadow over the light", dict(lights=room, lights_offset=0, index=0, shadow=room, shadow_offset=32), "overlap"),
        ("a misaligned wrapped table", dict(lights=wrapped(B["table"], 8, 64 * count + 64), lights_offset=0), "aligned"),
        ("rays_offset 8", dict(rays_offset=8), "16"), ("lit past the end", dict(lit_offset=off["lit"] + tail + 16), "lit buffer"),
        ("null rays", dict(rays=null), "ray buffer handle"), ("unknown shadow", dict(shadow=unknown), "shadow-ray buffer handle"),
        ("shadow over lit", dict(lit=room, lit_offset=64 * count, shadow=room, shadow_offset=64 * count + 16 * n - 32), "overlap"),
    ], snapshot, good, "rdx_punctual_light_hits")
    _refusals(rd, trace, [
        ("a table offset that is no multiple of 16", dict(lights_offset=off["table"] + 4), "16"),
        ("a table that overruns its buffer", dict(lights_offset=off["table"] + tail + 16), "light-table buffer"),
        ("a table one record short", dict(lights=wrapped(B["table"], 0, off["table"] + 64 * count - 64)), "light-table buffer"),
        ("null lights", dict(lights=null), "light-table buffer handle"), ("unknown lights", dict(lights=unknown), "light-table buffer handle"),
        ("radiance over the table", dict(lights=room, lights_offset=0, radiance=room, radiance_offset=64 * count - 16), "overlap"),
        ("radiance = the table", dict(lights=room, lights_offset=0, radiance=room, radiance_offset=0), "overlap"),
        ("a misaligned wrapped table", dict(lights=wrapped(B["table"], 4, 64 * count + 64), lights_offset=0), "aligned"),
        ("max_depth 63", dict(max_depth=63), "63"), ("null tlas", dict(tlas=null), "TLAS"), ("keys_offset 4", dict(keys_offset=4), "16"),
        ("radiance past the end", dict(radiance_offset=off["rad"] + tail + 16), "radiance buffer"),
        ("radiance over the rays", dict(radiance=wrapped(B["prays"], 0, off["prays"] + 16 * n), radiance_offset=off["prays"]), "overlap"),
        ("null material", dict(scene_buffers=rd.ShadingBuffers(c.scene, dev.meshInfoData, dev.indexData, dev.uvData, dev.normalData, null)), "material"),
    ], snapshot, good, "rdx_trace_paths_punctual")
    # light_count > 16 at the C ABI (rd.TracePunctualPaths refuses it before the library sees it), and a NULL scene struct
    from radiance_ray_tracing_amd import _lib
    L = _lib.lib()
    st = c.sb._struct()
    for bad in (17, 0xffffffff):
        assert L.rdx_trace_paths_punctual(tl.handle, B["prays"].handle, off["prays"], B["keys"].handle, off["keys"], n, DEPTH, B["table"].handle, off["table"], bad,
                                          C.byref(st), B["rad"].handle, off["rad"], None) != 0
        assert "light_count" in _lib.last_error() and "rdx_trace_paths_punctual" in _lib.last_error()
    assert L.rdx_trace_paths_punctual(tl.handle, B["prays"].handle, off["prays"], B["keys"].handle, off["keys"], n, DEPTH, B["table"].handle, off["table"], count,
                                      None, B["rad"].handle, off["rad"], None) != 0
    assert "scene" in _lib.last_error() and "rdx_trace_paths_punctual" in _lib.last_error()
    assert all(np.array_equal(v, good[k]) for k, v in snapshot().items()) and np.array_equal(rd.ReadBuffer(plt, room, room.size), room_good)
    # outputs right behind the table are fine, and the calls still work after the refusals
    hits(lights=room, lights_offset=0, lit=room, lit_offset=64 * count, shadow=None)
    assert same(rd.ReadBuffer(plt, room, 16 * n, offset=64 * count), plain["lit"])
    trace(lights=room, lights_offset=0, radiance=room, radiance_offset=64 * count)
    assert same(rd.ReadBuffer(plt, room, 16 * n, offset=64 * count), plain_rad.reshape(-1))
    assert np.array_equal(rd.ReadBuffer(plt, room, 64 * count), room_good[:64 * count])


def test_scene_buffers_that_do_not_describe_the_scene_are_fenced(mods, paths):
    """the construction of test_gpu_light_paths.py: a material buffer that holds fewer Materials than the scene uses.  The hits whose
    Material lies past it are misses, counted as rd.ResolveMaterials counts them over the bounces of the loop on the same buffers"""
    rd, _ = mods
    c = paths("c1")
    dev = c.dev
    nmat = dev.materialData.size // 48
    keep = nmat // 2
    assert keep >= 1
    short = rd.WrapDeviceMemory(c.plt, dev.materialData.device_ptr, 48 * keep, keepalive=dev.materialData)
    sb = lp.buffers_with_scene(rd, dev, c.scene, material=short)
    color, lives, invalid, first_invalid, _ = pu.public_loop_punctual(rd, c.plt, c.tlas, sb, dev.surface_buffers(), c.table[:6], c.rays, c.keys["frameID"],
                                                                      c.keys["pixel"], DEPTH)
    print("fencing: %d of %d Materials kept, invalid %d, first hit invalid on %d paths, lives %s" % (keep, nmat, invalid, int(first_invalid.sum()), lives))
    assert invalid >= 20 and first_invalid.sum() >= 20 and lives[0] >= 100
    got, got_invalid = c.run(6, sb=sb)
    check_radiance(got, color, "short material buffer")
    assert got_invalid == invalid
    assert (sh.bits(got[first_invalid, :3]) == sh.bits(sh.ENVIRONMENT)).all()
    assert not same(got[:, :3], c.want(6)[0])


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
table = pu.mixed_table(rd, lo, hi, sp, 3)[:6]
lights_t = torch.from_numpy(table.view(np.float32).reshape(-1, 16).copy()).cuda()      # (L, 16) float32; `type` keeps its bits
assert np.array_equal(lights_t.cpu().numpy().view(np.uint32), table.view(np.uint32).reshape(-1, 16))
bT = sh.upload(rd, plt, table)
# ---- the per-hit call
n = c.mat_rays.shape[0]
rec = sc.records(rd, dev, c.mat_rays)
t = (torch.from_numpy(c.mat_rays.view(np.float32).reshape(n, 8).copy()).cuda() * torch.ones(8, device="cuda")).contiguous()
mat0, _ = rd.ResolveMaterialsTorch(tlas, t, rd.QueryRaysTorch(tlas, t, rd.QUERY_CLOSEST), sb)
shown = 0
for j in range(table.shape[0]):
    want = pu.punctual_batch(rd, plt, tlas, rec["bR"], rec["bM"], n, bT, j, query=False)
    lit, shadow = rd.PunctualLightHitsTorch(t, mat0, lights_t, j)
    assert lit.dtype == torch.float32 and tuple(lit.shape) == (n, 4) and tuple(shadow.shape) == (n, 8) and lit.is_cuda
    assert np.array_equal(lit.cpu().numpy().view(np.uint32), want["lit"].view(np.uint32).reshape(n, 4)), j
    assert np.array_equal(shadow.cpu().numpy().view(np.uint32), want["shadow"].view(np.uint32).reshape(n, 8)), j
    lit2, none = rd.PunctualLightHitsTorch(t, mat0, lights_t, j, want_shadow=False)
    assert none is None and torch.equal(lit2.view(torch.int32), lit.view(torch.int32))
    shown += int(want["lit"]["rgb"].any())
assert shown >= 2
e = rd.PunctualLightHitsTorch(t[:0], mat0[:0], lights_t, 0)
assert tuple(e[0].shape) == (0, 4) and tuple(e[1].shape) == (0, 8)
# ---- the path call, and the README's loop with the table
cam = dev.frame_buffers()[0]
npix = dev.width * dev.height
max_depth, frame, total_samples = 3, 5, 4
rays, keys = rd.GenerateRaysTorch(cam, npix, frame, total_samples)
rn, kn = rays.cpu().numpy().view(rd.RAY_DTYPE).reshape(-1), keys.cpu().numpy().view(rd.SHADE_KEY_DTYPE).reshape(-1)
for L in (0, 1, 6):
    want, invalid = pu.trace(rd, plt, tlas, sb, rn, kn, max_depth, table[:L])
    got = rd.TracePunctualPathsTorch(tlas, rays, keys, max_depth, lights_t[:L], sb)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == (npix, 4) and got.is_cuda
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)) and invalid == 0 and want[:, :3].any(), L
call = rd.TracePunctualPathsTorch(tlas, rays, keys, max_depth, lights_t, sb)
n = npix
pixel = keys[:, 1].contiguous()
color = torch.zeros((n, 4), device="cuda")
weight = torch.ones((n, 3), device="cuda")
path = torch.arange(n, device="cuda")
miss_colour = torch.tensor([0.2, 0.2, 0.5], device="cuda")
for depth in range(max_depth):
    if depth:
        keys = torch.stack([torch.full_like(pixel, frame), pixel, torch.full_like(pixel, depth), torch.zeros_like(pixel)], 1).contiguous()
    hits = rd.QueryRaysTorch(tlas, rays, rd.QUERY_CLOSEST)
    surf, _ = rd.ResolveHitsTorch(tlas, rays, hits, sf)
    mat, _ = rd.ResolveMaterialsTorch(tlas, rays, hits, sb)
    if depth == 0:
        color[path[mat.view(torch.int32)[:, 3] != 1], :3] = miss_colour
    direct = torch.zeros((rays.shape[0], 3), device="cuda")
    for j in range(lights_t.shape[0]):
        lit, shadow = rd.PunctualLightHitsTorch(rays, mat, lights_t, j)
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
assert torch.equal(color.view(torch.int32), call.view(torch.int32)), "the README's loop differs from rd.TracePunctualPathsTorch"
assert tuple(rd.TracePunctualPathsTorch(tlas, rays[:0], keys[:0], max_depth, lights_t, sb).shape) == (0, 4)
rays, keys = rd.GenerateRaysTorch(cam, npix, frame, total_samples)
big = torch.zeros((17, 16), dtype=torch.float32, device="cuda")
bad = [lambda: rd.TracePunctualPathsTorch(tlas, rays, keys, max_depth, big, sb), lambda: rd.TracePunctualPathsTorch(tlas, rays, keys, max_depth, lights_t.double(), sb),
       lambda: rd.TracePunctualPathsTorch(tlas, rays, keys, max_depth, lights_t[:, :15], sb), lambda: rd.TracePunctualPathsTorch(tlas, rays, keys, max_depth, lights_t.cpu(), sb),
       lambda: rd.TracePunctualPathsTorch(tlas, rays, keys, max_depth, big[:, ::2], sb), lambda: rd.TracePunctualPathsTorch(tlas, rays, keys, max_depth, table, sb),
       lambda: rd.TracePunctualPathsTorch(tlas, rays[:, :7], keys, max_depth, lights_t, sb), lambda: rd.TracePunctualPathsTorch(tlas, rays, keys[:-1], max_depth, lights_t, sb),
       lambda: rd.TracePunctualPathsTorch(tlas, rays, keys, -1, lights_t, sb), lambda: rd.TracePunctualPathsTorch(tlas, rays, keys, max_depth, lights_t, (1, 2)),
       lambda: rd.PunctualLightHitsTorch(t, mat0, lights_t, 6), lambda: rd.PunctualLightHitsTorch(t, mat0, lights_t, -1),
       lambda: rd.PunctualLightHitsTorch(t, mat0, lights_t.double(), 0), lambda: rd.PunctualLightHitsTorch(t, mat0, lights_t[:, :8], 0),
       lambda: rd.PunctualLightHitsTorch(t, mat0, lights_t.cpu(), 0), lambda: rd.PunctualLightHitsTorch(t.cpu(), mat0, lights_t, 0),
       lambda: rd.PunctualLightHitsTorch(t, mat0[:-1], lights_t, 0), lambda: rd.PunctualLightHitsTorch(t, mat0, lights_t, 1.5)]
for j, fn in enumerate(bad):
    try:
        fn()
    except rd.RadianceError:
        continue
    raise AssertionError("bad argument set %d was accepted" % j)
print("TORCH-PUNCTUAL-OK", npix, shown)
"""


def test_torch_tensors_in_a_fresh_process(gpu):
    """rd.PunctualLightHitsTorch and rd.TracePunctualPathsTorch equal the buffer route bit for bit, and the README's loop over
    rd.PunctualLightHitsTorch equals rd.TracePunctualPathsTorch; a wrong dtype, shape or device is refused in Python.  torch is
    initialised first, in a process of its own (as tests/test_gpu_materials.py)"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _TORCH_CHILD, ROOT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "TORCH-PUNCTUAL-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])

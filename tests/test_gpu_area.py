"""GPU suite (-m gpu): rd.AreaLightHits / rd.TraceAreaPaths and their torch routes (rdx_area_light_hits, rdx_trace_paths_area) -- quad
and triangle area lights from a second caller-owned light table, sampled at one point per (hit, light).

Comparands, in this order of authority:
  1. rd.LightHits (tests/test_gpu_materials.py holds it to the reference's recorded payloads): an area record at a hit is that call
     on the DirLight {direction = -(p - above), color = E}, where p and E are area_cases.emitted_area -- the record's triangle fold,
     sampled point, normal, d2, geometry term and dark rule in numpy float32, one IEEE operation at a time.  normalize3 is built on
     v_rsq_f32, so emitted_area takes the unit vector from the call's own shadow records; it is held to numpy's w / |w| within
     2^-20 (1 ulp of v_rsq_f32, three roundings in d2, one product: the bound of test_gpu_punctual.py, for the same reason);
  2. area_cases.randoms_of, pcg3d in numpy: the keys route is the randoms route on it;
  3. rd.QueryRays for what the shadow interval does;
  4. area_cases.public_loop_area, the README's loop over the two per-hit calls, for the path call; rd.TracePunctualPaths for a call
     without area records.
Every bar but the unit-length one is equality of bits.  The per-hit tests run on the 2048 recorded primary rays of c1 and c2, the
path tests on paths_cases.arbitrary_batch (n = 2048 + 37) with the seeds of test_gpu_paths.py, at depth 4.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import area_cases as ar
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
COUNTS = ((0, 0), (0, 1), (3, 2), (0, 16), (15, 1))        # (punctual, area) records
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
    """per golden scene: the geometry and material records of its 2048 recorded primary rays, resolved once and left unchanged, the
    scene box and the three emitters placed from it"""
    rd, _ = mods
    cache = {}

    def get(name):
        if name not in cache:
            g = golden(name)
            r = sc.records(rd, g.dev, g.mat_rays)
            r["lo"], r["hi"] = scene_box(rd, g.dev)
            r["lights"] = ar.scene_lights(rd, r["lo"], r["hi"])
            r["keys"] = g.keys
            cache[name] = r
        return cache[name]
    return get


def uv_of(keys, stream):
    r = ar.randoms_of(keys["frameID"], keys["pixel"], keys["depth"], stream)["xyz"]
    return r[:, 0].copy(), r[:, 1].copy()


def as_light_hits(rd, plt, scene, bR, bM, i, w, E):
    """the comparand of row i: ONE rd.LightHits call (n = 1) on the DirLight {-w, E}"""
    rd.WriteBuffer(plt, scene, 176, np.array(pu.as_dir_light(rd, -w, E)).reshape(1))
    bL, bSh = rd.LightHits(bR, bM, 1, scene, 0, rays_offset=32 * i, materials_offset=64 * i)
    return sh.read(rd, plt, bL, 1, mc.LIT_DTYPE)[0], sh.read(rd, plt, bSh, 1, rd.RAY_DTYPE)[0]


# ---- 1. one point --------------------------------------------------------------------------------------------------------------------
def test_one_point(mods, golden, recs):
    """c1's material records with `above` of every row overwritten by one point A and constant randoms: p, L and E are uniform, so
    ONE rd.LightHits call on the DirLight {-w, E} is the comparand of every row.  The triangle's pair lies beyond its diagonal, so
    it is folded"""
    rd, _ = mods
    dev, rec = golden("c1").dev, recs("c1")
    plt, n = dev.plt, rec["n"]
    A = np.array([1.8, 1.0, 0.6], F)
    mat = rec["mat"].copy()
    hit = mat["hit"] == 1
    mat["above"][hit] = A
    bM = sh.upload(rd, plt, mat)
    for kind, (u0, v0) in (("ceiling", (0.3, 0.6)), ("inner", (0.7, 0.6))):
        light = rec["lights"][kind]
        randoms = sc.randoms_of(np.tile(np.array([u0, v0, 0.123], F), (n, 1)), 9.0)
        w = ar.area_batch(rd, plt, dev.topAccelStruct, rec["bR"], bM, n, sh.upload(rd, plt, ar.table(rd, [light])), 0, randoms=randoms, query=False)
        L = w["shadow"]["direction"][hit]
        assert hit.sum() >= 1024 and (sh.bits(L) == sh.bits(L[0])).all(), "L is not uniform"
        e = ar.emitted_area(light, A.reshape(1, 3), u0, v0, L[0])
        assert not e["dark"][0] and ar.in_emitter(light, e["u"], e["v"]).all()
        if kind == "inner":
            assert e["u"][0] == F(F(1.0) - F(u0)) and e["v"][0] == F(F(1.0) - F(v0)), "the pair was not folded"
        scene = sh.upload(rd, plt, np.array(pu.as_dir_light(rd, -e["w"][0], e["E"][0])).reshape(1))
        bL, bSh = rd.LightHits(rec["bR"], bM, n, scene, 0)
        want_lit, want_sh = sh.read(rd, plt, bL, n, mc.LIT_DTYPE), sh.read(rd, plt, bSh, n, rd.RAY_DTYPE)
        assert same(w["lit"], want_lit), kind
        assert same(w["shadow"]["direction"], want_sh["direction"]) and same(w["shadow"]["origin"], want_sh["origin"]), kind
        want_tmax = (np.sqrt(e["d2"][0]).astype(F) * F(0.999)).astype(F)
        assert same(w["shadow"]["tmin"], want_sh["tmin"]) and (sh.bits(w["shadow"]["tmax"][hit]) == sh.bits(want_tmax)).all(), kind
        assert sh.bits(e["tmax"][0]) == sh.bits(want_tmax)
        assert not w["shadow"][~hit].view(np.uint8).any() and not w["lit"][~hit].view(np.uint8).any()
        assert (w["lit"]["rgb"][hit] != 0).any(1).sum() >= 256, "%s: the light shows on too few rows" % kind


# ---- 2. the keys route is the randoms route -------------------------------------------------------------------------------------------
def test_the_keys_route_is_the_randoms_route(mods, golden, recs):
    rd, _ = mods
    dev, rec = golden("c1").dev, recs("c1")
    plt, tlas, n, keys = dev.plt, dev.topAccelStruct, rec["n"], rec["keys"]
    lights = rec["lights"]
    bT = sh.upload(rd, plt, ar.table(rd, [lights["ceiling"], lights["inner"], lights["away"]]))
    seen = []
    for index, stream in ((0, 0), (1, 1), (1, 15), (0, 0xfffe)):
        by_keys = ar.area_batch(rd, plt, tlas, rec["bR"], rec["bM"], n, bT, index, keys=keys, stream=stream, query=False)
        by_randoms = ar.area_batch(rd, plt, tlas, rec["bR"], rec["bM"], n, bT, index, randoms=ar.randoms_of(keys["frameID"], keys["pixel"], keys["depth"], stream), query=False)
        assert same(by_keys["lit"], by_randoms["lit"]) and same(by_keys["shadow"], by_randoms["shadow"]), (index, stream)
        assert (~ar.is_dark(by_keys)).sum() >= 256, (index, stream)
        seen.append(by_keys)
    assert not same(seen[1]["shadow"], seen[2]["shadow"]) and not same(seen[0]["shadow"], seen[3]["shadow"])      # another stream, other points
    # `stream` defaults to the index
    for index in (0, 1, 2):
        default = ar.area_batch(rd, plt, tlas, rec["bR"], rec["bM"], n, bT, index, keys=keys, query=False)
        explicit = ar.area_batch(rd, plt, tlas, rec["bR"], rec["bM"], n, bT, index, keys=keys, stream=index, query=False)
        assert same(default["lit"], explicit["lit"]) and same(default["shadow"], explicit["shadow"]), index
    assert same(seen[0]["lit"], ar.area_batch(rd, plt, tlas, rec["bR"], rec["bM"], n, bT, 0, keys=keys, query=False)["lit"])
    # lit alone
    lit_only, none = rd.AreaLightHits(rec["bR"], rec["bM"], n, bT, 1, keys=sh.upload(rd, plt, keys), shadow=None)
    assert none is None and same(sh.read(rd, plt, lit_only, n, mc.LIT_DTYPE), seen[1]["lit"])


# ---- 3. real `above`, sampled rows, exact --------------------------------------------------------------------------------------------
def classify(light, e, hit):
    """the classes of the rows by numpy alone (float64 directions): front (the raw geometry term is positive), back (negative);
    `unsure`: within 1e-4 |n| of the emitter's plane, where the call's own L decides"""
    w64 = e["w"].astype(np.float64)
    nrm = np.cross(np.ascontiguousarray(light["edgeU"], np.float64), np.ascontiguousarray(light["edgeV"], np.float64))
    g = -(w64 / np.linalg.norm(w64, axis=1, keepdims=True)) @ nrm
    margin = 1e-4 * np.linalg.norm(nrm)
    return dict(front=hit & (g > margin), back=hit & (g < -margin), unsure=hit & (np.abs(g) <= margin))


@pytest.mark.parametrize("name", ("c1", "c2"))
def test_real_hit_points_sampled_rows(mods, golden, recs, name):
    rd, _ = mods
    dev, rec = golden(name).dev, recs(name)
    plt, n, mat, keys = dev.plt, rec["n"], rec["mat"], rec["keys"]
    hit = mat["hit"] == 1
    rng = np.random.default_rng(11)
    scene = rd.CreateBuffer(plt, 176)
    kinds = ("ceiling", "inner", "away")
    bT = sh.upload(rd, plt, ar.table(rd, [rec["lights"][k] for k in kinds]))
    for index, kind in enumerate(kinds):
        light = rec["lights"][kind]
        two_sided = bool(int(light["flags"]) & 1)
        w = ar.area_batch(rd, plt, dev.topAccelStruct, rec["bR"], rec["bM"], n, bT, index, keys=keys, query=False)
        u, v = uv_of(keys, index)
        L = w["shadow"]["direction"]
        e = ar.emitted_area(light, mat["above"], u, v, L)
        cls = classify(light, e, hit)
        print("%s %s: %s" % (name, kind, {k: int(m.sum()) for k, m in cls.items()}))
        # every class that must occur has >= 16 rows: lit front; lit back of the two-sided record; dark by back face
        assert cls["front"].sum() >= 16, (name, kind)
        if kind in ("inner", "away"):
            assert cls["back"].sum() >= 16, (name, kind)
        dark = ar.is_dark(w)
        want_lit = cls["front"] | (cls["back"] if two_sided else np.zeros(n, bool))
        want_dark = ~hit | (cls["back"] & (not two_sided))
        assert dark[want_dark].all() and not dark[want_lit].any() and (want_dark | want_lit | cls["unsure"]).all(), (name, kind)
        # dark rows are 16 + 32 zero bytes (is_dark); a row is never half dark
        assert (w["lit"].view(np.uint8).reshape(n, 16).any(1) <= ~dark).all() and (w["shadow"].view(np.uint8).reshape(n, 32).any(1) == ~dark).all()
        lit_rows = ~dark
        # emitted_area on the call's own L agrees row for row
        assert not e["dark"][lit_rows].any() and e["dark"][dark & hit].all(), (name, kind)
        assert (sh.bits(w["shadow"]["tmax"][lit_rows]) == sh.bits(e["tmax"][lit_rows])).all()
        assert (sh.bits(e["tmax"]) == sh.bits((np.sqrt(e["d2"]).astype(F) * F(0.999)).astype(F))).all()
        assert same(w["shadow"]["origin"][lit_rows], mat["above"][lit_rows]) and (sh.bits(w["shadow"]["tmin"][lit_rows]) == sh.bits(F(0.001))).all()
        L64, w64 = L[lit_rows].astype(np.float64), e["w"][lit_rows].astype(np.float64)
        assert np.abs((L64 * L64).sum(1) - 1.0).max() <= EPS
        assert np.abs(L64 - w64 / np.linalg.norm(w64, axis=1, keepdims=True)).max() <= EPS
        # the sampled point, recomputed from (u, v), lies in the emitter, and the shadow ray ends just short of it
        assert ar.in_emitter(light, e["u"], e["v"]).all()
        if int(light["type"]) == ar.TRIANGLE:
            assert ((u + v).astype(F) > 1).sum() >= 256 and (e["u"] != u).sum() >= 256
        end = mat["above"][lit_rows].astype(np.float64) + L64 * (w["shadow"]["tmax"][lit_rows].astype(np.float64) / 0.999)[:, None]
        assert np.abs(end - e["p"][lit_rows].astype(np.float64)).max() <= 1e-4 * float(np.abs(rec["hi"] - rec["lo"]).max())
        # 16 rows of every lit class: the construction of test 1 as an n = 1 rd.LightHits call.  A back row of the two-sided record
        # has the front's E: fabsf
        for k in ("front", "back"):
            if k == "back" and not two_sided:
                continue
            for i in rng.choice(np.flatnonzero(cls[k]), 16, replace=False):
                i = int(i)
                want_l, want_s = as_light_hits(rd, plt, scene, rec["bR"], rec["bM"], i, e["w"][i], e["E"][i])
                assert same(w["lit"][i], want_l), (name, kind, k, i, w["lit"][i], want_l)
                assert same(w["shadow"]["direction"][i], want_s["direction"]) and same(w["shadow"]["origin"][i], want_s["origin"]), (name, kind, k, i)
        if two_sided:
            assert (e["g"][cls["back"]] > 0).all()
        assert (w["lit"]["rgb"][lit_rows] != 0).any(1).sum() >= 16, (name, kind)


# ---- 4. shadows: the interval ends at the light ---------------------------------------------------------------------------------------
def test_the_shadow_ray_stops_short_of_the_emitter(mods, golden, recs):
    """c1: occluded == (closest hit on the shadow ray && t < tmax), row for row and for all three emitters.  The quad lies 0.12 under
    the ceiling: with the stock interval its shadow rays would reach the ceiling behind it"""
    rd, _ = mods
    dev, rec = golden("c1").dev, recs("c1")
    plt, tlas, n, keys = dev.plt, dev.topAccelStruct, rec["n"], rec["keys"]
    kinds = ("ceiling", "inner", "away")
    bT = sh.upload(rd, plt, ar.table(rd, [rec["lights"][k] for k in kinds]))
    total_occluded = total_open = 0
    for index, kind in enumerate(kinds):
        w = ar.area_batch(rd, plt, tlas, rec["bR"], rec["bM"], n, bT, index, keys=keys)
        rows = ~ar.is_dark(w)
        far = w["shadow"][rows].copy()
        far["tmax"] = 1000.0
        q = sh.read(rd, plt, rd.QueryRays(tlas, sh.upload(rd, plt, far), far.shape[0], rd.QUERY_CLOSEST), far.shape[0], rd.RAY_HIT_DTYPE)
        tmax, occluded = w["shadow"]["tmax"][rows], w["occluded"][rows]
        assert np.array_equal(occluded, (q["hit"] == 1) & (q["t"] < tmax)), kind
        assert not w["occluded"][~rows].any(), kind
        behind = (q["hit"] == 1) & (q["t"] >= tmax) & ~occluded
        print("%s: %d lit rows, %d occluded, %d whose first hit lies behind the sampled point" % (kind, int(rows.sum()), int(occluded.sum()), int(behind.sum())))
        total_occluded += int(occluded.sum())
        total_open += int((~occluded).sum())
        if kind == "ceiling":
            # the first hit behind the emitter is the ceiling itself: instance 1 of the scene, at y = hi.y
            end = far["origin"][behind].astype(np.float64) + far["direction"][behind].astype(np.float64) * q["t"][behind].astype(np.float64)[:, None]
            on_ceiling = np.abs(end[:, 1] - rec["hi"][1]) < 1e-3
            assert on_ceiling.sum() >= 64, int(on_ceiling.sum())
            assert occluded.sum() >= 64 and (~occluded).sum() >= 64 and rows.sum() >= 512
    assert total_occluded >= 64 and total_open >= 64, (total_occluded, total_open)


# ---- 5. soft shadows exist --------------------------------------------------------------------------------------------------------------
def test_soft_shadows_exist(mods, golden, recs):
    """the fixed hit points of c1 under the ceiling quad, 64 frames: a hit point in the penumbra is occluded in some frames and not in
    others; under a point light at the quad's centre no answer ever changes.  Structural, not a measurement"""
    rd, _ = mods
    dev, rec = golden("c1").dev, recs("c1")
    plt, tlas, n = dev.plt, dev.topAccelStruct, rec["n"]
    light = rec["lights"]["ceiling"]
    bT = sh.upload(rd, plt, ar.table(rd, [light]))
    pixels = np.arange(n, dtype=np.uint32)
    answers = np.zeros((64, n), bool)
    for frame in range(64):
        w = ar.area_batch(rd, plt, tlas, rec["bR"], rec["bM"], n, bT, 0, keys=sh.keys_of(np.full(n, frame, np.uint32), pixels, np.zeros(n, np.uint32)))
        answers[frame] = w["occluded"]
    differs = answers.any(0) & ~answers.all(0)
    print("soft shadows: %d of %d hit points change their answer over 64 frames; %d always occluded" % (int(differs.sum()), n, int(answers.all(0).sum())))
    assert differs.sum() >= 64
    centre = (np.ascontiguousarray(light["corner"], F) + F(0.5) * np.ascontiguousarray(light["edgeU"], F) + F(0.5) * np.ascontiguousarray(light["edgeV"], F)).astype(F)
    bP = sh.upload(rd, plt, pu.table(rd, [pu.light(rd, pu.POINT, centre, color=(30.0, 28.0, 24.0))]))
    hard = [pu.punctual_batch(rd, plt, tlas, rec["bR"], rec["bM"], n, bP, 0)["occluded"] for _ in range(4)]
    assert all(np.array_equal(h, hard[0]) for h in hard) and hard[0].sum() >= 1


# ---- 6. the path call is the loop ----------------------------------------------------------------------------------------------------
class PathCase:
    """one golden scene: the arbitrary batch of 2048 + 37 paths, the two tables, and per pair of table sizes the answer of the
    README's loop over rd.PunctualLightHits and rd.AreaLightHits, computed once and left unchanged"""

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
        self.area = ar.area_table(rd, lo, hi, SEED[name])
        self._want = {}

    def want(self, counts, depth=DEPTH):
        if (counts, depth) not in self._want:
            self._want[(counts, depth)] = ar.public_loop_area(self.rd, self.plt, self.tlas, self.sb, self.dev.surface_buffers(), self.table[:counts[0]],
                                                              self.area[:counts[1]], self.rays, self.keys["frameID"], self.keys["pixel"], depth)
        return self._want[(counts, depth)]

    def run(self, counts, depth=DEPTH, sb=None, area=None):
        return ar.trace(self.rd, self.plt, self.tlas, sb or self.sb, self.rays, self.keys, depth, self.table[:counts[0]],
                        self.area[:counts[1]] if area is None else area)


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


@pytest.mark.parametrize("counts", COUNTS)
@pytest.mark.parametrize("name", ("c1", "c2"))
def test_the_path_call_is_the_loop(mods, paths, name, counts):
    rd, _ = mods
    c = paths(name)
    color, lives, invalid, _, dark0 = c.want(counts)
    got, got_invalid = c.run(counts)
    bounce = rd.GetBounceCounts(DEPTH + 2).copy()
    st = rd.GetTraceStats()
    check_radiance(got, color, "%s, %d + %d records" % (name, counts[0], counts[1]))
    assert invalid == 0 and got_invalid == 0 and c.n == N_PATHS
    want_counts = np.zeros(DEPTH + 2, np.uint64)
    want_counts[0], want_counts[1:1 + len(lives)] = c.n, lives
    assert np.array_equal(bounce, want_counts), (bounce.tolist(), lives)
    assert len(lives) >= 2 and lives[1] >= 0.25 * c.n
    assert st.rays_shadow == sum(counts) * sum(lives) and st.closest_hits == sum(lives)
    print("%s, %d + %d records: (dark, lit) depth-0 hits per record %s" % (name, counts[0], counts[1], dark0))
    if counts[1]:       # the area table matters, and holds a record that is dark for part of the hits; from 4 records on the type-2 record
        without = c.want((counts[0], 0))[0]
        assert (sh.bits(without) != sh.bits(color)).any(1).sum() >= 20
        area0 = dark0[counts[0]:]
        assert any(d >= 16 and l >= 16 for d, l in area0), area0
    if counts[1] >= 4:
        assert int(c.area["type"][3]) == 2 and dark0[counts[0] + 3][1] == 0 and dark0[counts[0] + 3][0] == lives[0]


@pytest.mark.parametrize("count", (5, 16))
@pytest.mark.parametrize("name", ("c1", "c2"))
def test_without_area_records_it_is_trace_punctual_paths(mods, paths, name, count):
    """the restated punctual_emit and gather of k_area_shade against k_punctual_shade, bit for bit; the area table absent (None)"""
    rd, _ = mods
    c = paths(name)
    want, invalid = pu.trace(rd, c.plt, c.tlas, c.sb, c.rays, c.keys, DEPTH, c.table[:count])
    got, got_invalid = c.run((count, 0))
    assert same(got, want) and invalid == 0 and got_invalid == 0 and want[:, :3].any()
    # ... and with a table given but no record of it counted
    bA = sh.upload(rd, c.plt, c.area)
    bR, inv = rd.TraceAreaPaths(c.tlas, sh.upload(rd, c.plt, c.rays), sh.upload(rd, c.plt, c.keys), c.n, DEPTH, sh.upload(rd, c.plt, c.table), count, bA, 0, c.sb)
    assert same(rd.ReadBuffer(c.plt, bR, 16 * c.n).view(F).reshape(c.n, 4), want) and inv == 0


def test_chunks_do_not_matter(mods, paths):
    rd, _ = mods
    c = paths("c2")
    rad, _ = c.run((0, 16))
    check_radiance(rad, c.want((0, 16))[0], "defaults")
    try:
        rd.SetOption("chunk_paths", 512)
        got, invalid = c.run((0, 16))
        st = rd.GetTraceStats()
        got5, _ = c.run((3, 2))
    finally:
        rd.SetOption("chunk_paths", DEFAULTS["chunk_paths"])
    # 16 records: a chunk is 512 * 592 / (192 + 80 * 16) = 205 paths, eleven chunks; 3 + 2 records: 512 paths, five chunks
    assert same(got, rad) and invalid == 0 and st.rays_primary == c.n and st.launches_extend >= 11
    check_radiance(got5, c.want((3, 2))[0], "3 + 2 records in chunks of 512")
    assert same(c.run((0, 16))[0], rad)


def test_the_tables_are_read_by_every_call(mods, paths):
    rd, _ = mods
    c = paths("c1")
    table, area = c.table[:3].copy(), c.area[:2].copy()
    bT, bA = sh.upload(rd, c.plt, table), sh.upload(rd, c.plt, area)
    bR, bK = sh.upload(rd, c.plt, c.rays), sh.upload(rd, c.plt, c.keys)
    run = lambda: rd.ReadBuffer(c.plt, rd.TraceAreaPaths(c.tlas, bR, bK, c.n, DEPTH, bT, 3, bA, 2, c.sb)[0], 16 * c.n).view(F).reshape(c.n, 4).copy()
    first = run()
    check_radiance(first, c.want((3, 2))[0], "before the rewrite")
    area[0] = c.area[2]
    rd.WriteBuffer(c.plt, bA, area.nbytes, area)
    second = run()
    want = ar.public_loop_area(rd, c.plt, c.tlas, c.sb, c.dev.surface_buffers(), table, area, c.rays, c.keys["frameID"], c.keys["pixel"], DEPTH)[0]
    check_radiance(second, want, "after the rewrite")
    assert not same(first, second)


# ---- 7. shapes -------------------------------------------------------------------------------------------------------------------------
def test_shapes(mods, golden, recs, paths):
    """n in {0, 1, 63, 64, 65, 255, 256, 257} for both calls: the rows of the full run (c2: rows 300 .. hold hits, misses and dark
    rows; a path's radiance does not depend on the other paths of its call).  max_depth 0 gives zeros"""
    rd, _ = mods
    dev, rec = golden("c2").dev, recs("c2")
    plt, keys = dev.plt, recs("c2")["keys"]
    bT = sh.upload(rd, plt, ar.table(rd, [rec["lights"]["away"]]))
    full = ar.area_batch(rd, plt, dev.topAccelStruct, rec["bR"], rec["bM"], rec["n"], bT, 0, keys=keys, query=False)
    c = paths("c2")
    rad, _ = c.run((3, 2))
    first = 300
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        rows = slice(first, first + n)
        w = ar.area_batch(rd, plt, dev.topAccelStruct, rec["bR"], rec["bM"], n, bT, 0, keys=keys[rows] if n else np.zeros(1, keys.dtype), query=False,
                          rays_offset=32 * first, materials_offset=64 * first)
        assert same(w["lit"], full["lit"][rows]) and same(w["shadow"], full["shadow"][rows]), n
        got, invalid = ar.trace(rd, plt, c.tlas, c.sb, c.rays[rows], c.keys[rows], DEPTH, c.table[:3], c.area[:2])
        assert got.shape == (n, 4) and invalid == 0 and same(got, rad[rows]), n
    dark = ar.is_dark(full)[first:first + 257]
    assert 0 < int(dark.sum()) < 257 and (rec["mat"]["hit"][first:first + 257] == 1).sum() > int((~dark).sum()) > 0
    got, invalid = c.run((3, 2), depth=0)
    assert got.shape == (c.n, 4) and not got.view(np.uint8).any() and invalid == 0


# ---- 8. offsets, refusals, fencing -----------------------------------------------------------------------------------------------------
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
    n, tail, lcount, acount, index = 200, 128, 3, 4, 1       # record 1: the two-sided triangle, lit on most hits
    table, area = c.table[:lcount], c.area[:acount]
    hkeys = rec["keys"][:n]
    off = dict(rays=96, mat=192, table=128, area=64, hkeys=48, rnd=80, lit=48, shadow=32, prays=64, keys=80, rad=112)
    size = dict(rays=32 * n, mat=64 * n, table=64 * lcount, area=64 * acount, hkeys=16 * n, rnd=16 * n, lit=16 * n, shadow=32 * n, prays=32 * n, keys=16 * n,
                rad=16 * n)
    B = {k: rd.CreateBuffer(plt, off[k] + size[k] + tail) for k in off}
    fill = lambda buf: rd.WriteBuffer(plt, buf, buf.size, np.full(buf.size, 0xA5, np.uint8))
    for buf in B.values():
        fill(buf)
    rnd = ar.randoms_of(hkeys["frameID"], hkeys["pixel"], hkeys["depth"], index)
    for k, arr in (("rays", golden("c1").mat_rays[:n]), ("mat", rec["mat"][:n]), ("table", table), ("area", area), ("hkeys", hkeys), ("rnd", rnd),
                   ("prays", c.rays[:n]), ("keys", c.keys[:n])):
        rd.WriteBuffer(plt, B[k], size[k], arr, offset=off[k])
    snapshot = lambda: {k: rd.ReadBuffer(plt, B[k], B[k].size).copy() for k in B}

    def hits(**kw):
        a = dict(rays=B["rays"], materials=B["mat"], n=n, lights=B["area"], index=index, keys=B["hkeys"], randoms=None, lit=B["lit"], shadow=B["shadow"],
                 rays_offset=off["rays"], materials_offset=off["mat"], lights_offset=off["area"], keys_offset=off["hkeys"], randoms_offset=off["rnd"],
                 lit_offset=off["lit"], shadow_offset=off["shadow"])
        a.update(kw)
        return rd.AreaLightHits(a.pop("rays"), a.pop("materials"), a.pop("n"), a.pop("lights"), a.pop("index"), **a)

    def trace(**kw):
        a = dict(tlas=tl, rays=B["prays"], keys=B["keys"], n=n, max_depth=DEPTH, lights=B["table"], light_count=lcount, area=B["area"], area_count=acount,
                 scene_buffers=c.sb, radiance=B["rad"], rays_offset=off["prays"], keys_offset=off["keys"], lights_offset=off["table"], area_offset=off["area"],
                 radiance_offset=off["rad"])
        a.update(kw)
        return rd.TraceAreaPaths(a.pop("tlas"), a.pop("rays"), a.pop("keys"), a.pop("n"), a.pop("max_depth"), a.pop("lights"), a.pop("light_count"), a.pop("area"),
                                 a.pop("area_count"), a.pop("scene_buffers"), **a)

    plain = ar.area_batch(rd, plt, tl, rec["bR"], rec["bM"], n, sh.upload(rd, plt, area), index, keys=hkeys, query=False)
    plain_rad, _ = ar.trace(rd, plt, tl, c.sb, c.rays[:n], c.keys[:n], DEPTH, table, area)
    before = snapshot()
    assert hits() == (B["lit"], B["shadow"]) and trace() == (B["rad"], 0)
    after = snapshot()
    for k in ("rays", "mat", "table", "area", "hkeys", "rnd", "prays", "keys"):
        assert np.array_equal(after[k], before[k]), k
    for k, want in (("lit", plain["lit"]), ("shadow", plain["shadow"]), ("rad", plain_rad.reshape(-1))):
        lo, hi = off[k], off[k] + size[k]
        assert same(after[k][lo:hi], want), k
        assert (after[k][:lo] == 0xA5).all() and (after[k][hi:] == 0xA5).all(), k
    assert plain["lit"]["rgb"].any() and plain_rad[:, :3].any()
    # the randoms route at its offset is the keys route
    fill(B["lit"]); fill(B["shadow"])
    hits(keys=None, randoms=B["rnd"])
    now = snapshot()
    assert same(now["lit"][off["lit"]:off["lit"] + size["lit"]], plain["lit"]) and same(now["shadow"][off["shadow"]:off["shadow"] + size["shadow"]], plain["shadow"])
    for k in ("lit", "shadow", "rad"):      # n == 0 touches nothing
        fill(B[k])
    assert hits(n=0) == (B["lit"], B["shadow"]) and trace(n=0) == (B["rad"], 0)
    assert all((rd.ReadBuffer(plt, B[k], B[k].size) == 0xA5).all() for k in ("lit", "shadow", "rad"))
    hits(); trace()
    good = snapshot()

    null, unknown = rd.Buffer(None, 1 << 20), rd.Buffer(12345678, 1 << 20)
    wrapped = lambda buf, shift, nbytes: rd.WrapDeviceMemory(plt, buf.device_ptr + shift, nbytes, keepalive=buf)
    room = rd.CreateBuffer(plt, 64 * acount + 64 * n + 256)      # a table followed by room for an output, for the overlap cases
    rd.WriteBuffer(plt, room, 64 * acount, area)
    room_good = rd.ReadBuffer(plt, room, room.size).copy()
    _refusals(rd, hits, [
        ("a light offset that is no multiple of 16", dict(lights_offset=off["area"] + 8), "16"),
        ("a record past the table's buffer", dict(index=acount + 2), "area-light buffer"),
        ("a record that ends past the buffer", dict(lights=wrapped(B["area"], 0, off["area"] + 64 + 32), index=1), "area-light buffer"),
        ("null lights", dict(lights=null), "area-light buffer handle"), ("unknown lights", dict(lights=unknown), "area-light buffer handle"),
        ("lit over the light", dict(lights=room, lights_offset=0, index=1, lit=room, lit_offset=112), "overlap"),
        ("shadow over the light", dict(lights=room, lights_offset=0, index=0, shadow=room, shadow_offset=32), "overlap"),
        ("a misaligned wrapped table", dict(lights=wrapped(B["area"], 8, 64 * acount + 64), lights_offset=0), "aligned"),
        ("keys_offset 8", dict(keys_offset=8), "16"), ("keys past the end", dict(keys_offset=off["hkeys"] + tail + 16), "key buffer"),
        ("unknown keys", dict(keys=unknown), "key buffer handle"),
        ("lit over the keys", dict(n=4, lit=B["hkeys"], lit_offset=off["hkeys"] + 48), "overlap"),
        ("randoms_offset 8", dict(keys=None, randoms=B["rnd"], randoms_offset=8), "16"),
        ("randoms past the end", dict(keys=None, randoms=B["rnd"], randoms_offset=off["rnd"] + tail + 16), "randoms buffer"),
        ("shadow over the randoms", dict(n=4, keys=None, randoms=B["rnd"], shadow=B["rnd"], shadow_offset=off["rnd"] - 32), "overlap"),
        ("rays_offset 8", dict(rays_offset=8), "16"), ("lit past the end", dict(lit_offset=off["lit"] + tail + 16), "lit buffer"),
        ("null rays", dict(rays=null), "ray buffer handle"), ("unknown shadow", dict(shadow=unknown), "shadow-ray buffer handle"),
    ], snapshot, good, "rdx_area_light_hits")
    _refusals(rd, trace, [
        ("an area offset that is no multiple of 16", dict(area_offset=off["area"] + 4), "16"),
        ("an area table that overruns its buffer", dict(area_offset=off["area"] + tail + 16), "area-light-table buffer"),
        ("an area table one record short", dict(area=wrapped(B["area"], 0, off["area"] + 64 * acount - 64)), "area-light-table buffer"),
        ("null area", dict(area=null), "area-light-table buffer handle"), ("unknown area", dict(area=unknown), "area-light-table buffer handle"),
        ("unknown area, no records", dict(area=unknown, area_count=0), "area-light-table buffer handle"),
        ("null lights", dict(lights=null), "light-table buffer handle"),
        ("a punctual table that overruns its buffer", dict(lights_offset=off["table"] + tail + 16), "light-table buffer"),
        ("radiance over the area table", dict(area=room, area_offset=0, radiance=room, radiance_offset=64 * acount - 16), "overlap"),
        ("radiance = the area table", dict(area=room, area_offset=0, radiance=room, radiance_offset=0), "overlap"),
        ("radiance over the punctual table", dict(radiance=B["table"], radiance_offset=off["table"] + 64 * lcount - 16, n=4), "overlap"),
        ("a misaligned wrapped area table", dict(area=wrapped(B["area"], 4, 64 * acount + 64), area_offset=0), "aligned"),
        ("max_depth 63", dict(max_depth=63), "63"), ("null tlas", dict(tlas=null), "TLAS"), ("keys_offset 4", dict(keys_offset=4), "16"),
        ("radiance past the end", dict(radiance_offset=off["rad"] + tail + 16), "radiance buffer"),
        ("null material", dict(scene_buffers=rd.ShadingBuffers(c.scene, dev.meshInfoData, dev.indexData, dev.uvData, dev.normalData, null)), "material"),
    ], snapshot, good, "rdx_trace_paths_area")
    # what the wrappers refuse before the library sees it, at the C ABI: the sum rule, both / neither of keys and randoms, the stream
    from radiance_ray_tracing_amd import _lib
    L = _lib.lib()
    st = c.sb._struct()
    for lc, acnt in ((16, 1), (9, 8), (0, 17), (17, 0), (0xffffffff, 1), (1, 0xffffffff), (0x80000000, 0x80000000)):
        assert L.rdx_trace_paths_area(tl.handle, B["prays"].handle, off["prays"], B["keys"].handle, off["keys"], n, DEPTH, B["table"].handle, off["table"], lc,
                                      B["area"].handle, off["area"], acnt, C.byref(st), B["rad"].handle, off["rad"], None) != 0
        assert "area_count" in _lib.last_error() and "rdx_trace_paths_area" in _lib.last_error()
    assert L.rdx_trace_paths_area(tl.handle, B["prays"].handle, off["prays"], B["keys"].handle, off["keys"], n, DEPTH, B["table"].handle, off["table"], lcount,
                                  B["area"].handle, off["area"], acount, None, B["rad"].handle, off["rad"], None) != 0
    assert "scene" in _lib.last_error() and "rdx_trace_paths_area" in _lib.last_error()
    raw_hits = lambda keys, stream, randoms: L.rdx_area_light_hits(B["rays"].handle, off["rays"], B["mat"].handle, off["mat"], n, B["area"].handle, off["area"], keys,
                                                                   off["hkeys"], stream, randoms, off["rnd"], B["lit"].handle, off["lit"], B["shadow"].handle, off["shadow"])
    for keys, stream, randoms, word in ((B["hkeys"].handle, 0, B["rnd"].handle, "both"), (None, 0, None, "neither"), (B["hkeys"].handle, 0xffff, None, "stream"),
                                        (B["hkeys"].handle, 0xffffffff, None, "stream")):
        assert raw_hits(keys, stream, randoms) != 0
        assert word in _lib.last_error() and "rdx_area_light_hits" in _lib.last_error(), _lib.last_error()
    assert raw_hits(B["hkeys"].handle, 0xfffe, None) == 0          # the largest stream is accepted
    hits()
    assert all(np.array_equal(v, good[k]) for k, v in snapshot().items()) and np.array_equal(rd.ReadBuffer(plt, room, room.size), room_good)
    # outputs right behind the table are fine, and the calls still work after the refusals
    hits(lights=room, lights_offset=0, lit=room, lit_offset=64 * acount, shadow=None)
    assert same(rd.ReadBuffer(plt, room, 16 * n, offset=64 * acount), plain["lit"])
    trace(area=room, area_offset=0, radiance=room, radiance_offset=64 * acount)
    assert same(rd.ReadBuffer(plt, room, 16 * n, offset=64 * acount), plain_rad.reshape(-1))
    assert np.array_equal(rd.ReadBuffer(plt, room, 64 * acount), room_good[:64 * acount])


def test_scene_buffers_that_do_not_describe_the_scene_are_fenced(mods, paths):
    """the construction of test_gpu_punctual.py: a material buffer that holds fewer Materials than the scene uses.  The hits whose
    Material lies past it are misses, counted as rd.ResolveMaterials counts them over the bounces of the loop on the same buffers"""
    rd, _ = mods
    c = paths("c1")
    dev = c.dev
    nmat = dev.materialData.size // 48
    keep = nmat // 2
    assert keep >= 1
    short = rd.WrapDeviceMemory(c.plt, dev.materialData.device_ptr, 48 * keep, keepalive=dev.materialData)
    sb = lp.buffers_with_scene(rd, dev, c.scene, material=short)
    color, lives, invalid, first_invalid, _ = ar.public_loop_area(rd, c.plt, c.tlas, sb, dev.surface_buffers(), c.table[:3], c.area[:2], c.rays, c.keys["frameID"],
                                                                  c.keys["pixel"], DEPTH)
    print("fencing: %d of %d Materials kept, invalid %d, first hit invalid on %d paths, lives %s" % (keep, nmat, invalid, int(first_invalid.sum()), lives))
    assert invalid >= 20 and first_invalid.sum() >= 20 and lives[0] >= 100
    got, got_invalid = c.run((3, 2), sb=sb)
    check_radiance(got, color, "short material buffer")
    assert got_invalid == invalid
    assert (sh.bits(got[first_invalid, :3]) == sh.bits(sh.ENVIRONMENT)).all()
    assert not same(got[:, :3], c.want((3, 2))[0])


# ---- 9. torch tensors ------------------------------------------------------------------------------------------------------------------
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
import area_cases as ar
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
as_t = lambda a: torch.from_numpy(a.view(np.float32).reshape(-1, 16).copy()).cuda()      # (L, 16) float32; `type` and `flags` keep their bits
lights_t, area_t = as_t(table), as_t(area)
assert np.array_equal(area_t.cpu().numpy().view(np.uint32), area.view(np.uint32).reshape(-1, 16))
bA = sh.upload(rd, plt, area)
# ---- the per-hit call, both routes
n = c.mat_rays.shape[0]
rec = sc.records(rd, dev, c.mat_rays)
t = (torch.from_numpy(c.mat_rays.view(np.float32).reshape(n, 8).copy()).cuda() * torch.ones(8, device="cuda")).contiguous()
mat0, _ = rd.ResolveMaterialsTorch(tlas, t, rd.QueryRaysTorch(tlas, t, rd.QUERY_CLOSEST), sb)
keys_t = torch.from_numpy(c.keys.view(np.int32).reshape(n, 4).copy()).cuda()
shown = 0
for j in range(area.shape[0]):
    want = ar.area_batch(rd, plt, tlas, rec["bR"], rec["bM"], n, bA, j, keys=c.keys, query=False)
    lit, shadow = rd.AreaLightHitsTorch(t, mat0, area_t, j, keys=keys_t)
    assert lit.dtype == torch.float32 and tuple(lit.shape) == (n, 4) and tuple(shadow.shape) == (n, 8) and lit.is_cuda
    assert np.array_equal(lit.cpu().numpy().view(np.uint32), want["lit"].view(np.uint32).reshape(n, 4)), j
    assert np.array_equal(shadow.cpu().numpy().view(np.uint32), want["shadow"].view(np.uint32).reshape(n, 8)), j
    rnd_t = torch.from_numpy(ar.randoms_of(c.keys["frameID"], c.keys["pixel"], c.keys["depth"], j).view(np.float32).reshape(n, 4).copy()).cuda()
    lit2, none = rd.AreaLightHitsTorch(t, mat0, area_t, j, randoms=rnd_t, want_shadow=False)
    assert none is None and torch.equal(lit2.view(torch.int32), lit.view(torch.int32))
    shown += int(want["lit"]["rgb"].any())
assert shown >= 2
e = rd.AreaLightHitsTorch(t[:0], mat0[:0], area_t, 0, keys=keys_t[:0])
assert tuple(e[0].shape) == (0, 4) and tuple(e[1].shape) == (0, 8)
# ---- the path call, and the README's loop with both tables
cam = dev.frame_buffers()[0]
npix = dev.width * dev.height
max_depth, frame, total_samples = 3, 5, 4
rays, keys = rd.GenerateRaysTorch(cam, npix, frame, total_samples)
rn, kn = rays.cpu().numpy().view(rd.RAY_DTYPE).reshape(-1), keys.cpu().numpy().view(rd.SHADE_KEY_DTYPE).reshape(-1)
for L, A in ((0, 0), (0, 3), (2, 2)):
    want, invalid = ar.trace(rd, plt, tlas, sb, rn, kn, max_depth, table[:L], area[:A])
    got = rd.TraceAreaPathsTorch(tlas, rays, keys, max_depth, lights_t[:L] if L else None, area_t[:A] if A else None, sb)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == (npix, 4) and got.is_cuda
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)) and invalid == 0 and want[:, :3].any(), (L, A)
assert torch.equal(rd.TraceAreaPathsTorch(tlas, rays, keys, max_depth, lights_t, area_t[:0], sb).view(torch.int32),
                   rd.TracePunctualPathsTorch(tlas, rays, keys, max_depth, lights_t, sb).view(torch.int32))
call = rd.TraceAreaPathsTorch(tlas, rays, keys, max_depth, lights_t, area_t, sb)
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
    for j in range(area_t.shape[0]):
        lit, shadow = rd.AreaLightHitsTorch(rays, mat, area_t, j, keys=keys)       # stream = j
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
assert torch.equal(color.view(torch.int32), call.view(torch.int32)), "the README's loop differs from rd.TraceAreaPathsTorch"
assert tuple(rd.TraceAreaPathsTorch(tlas, rays[:0], keys[:0], max_depth, lights_t, area_t, sb).shape) == (0, 4)
rays, keys = rd.GenerateRaysTorch(cam, npix, frame, total_samples)
big = torch.zeros((15, 16), dtype=torch.float32, device="cuda")
rnd_t = torch.zeros((t.shape[0], 4), dtype=torch.float32, device="cuda")
bad = [lambda: rd.TraceAreaPathsTorch(tlas, rays, keys, max_depth, lights_t, big, sb), lambda: rd.TraceAreaPathsTorch(tlas, rays, keys, max_depth, lights_t, area_t.double(), sb),
       lambda: rd.TraceAreaPathsTorch(tlas, rays, keys, max_depth, lights_t, area_t[:, :15], sb), lambda: rd.TraceAreaPathsTorch(tlas, rays, keys, max_depth, lights_t, area_t.cpu(), sb),
       lambda: rd.TraceAreaPathsTorch(tlas, rays, keys, max_depth, None, big[:, ::2], sb), lambda: rd.TraceAreaPathsTorch(tlas, rays, keys, max_depth, None, area, sb),
       lambda: rd.TraceAreaPathsTorch(tlas, rays[:, :7], keys, max_depth, lights_t, area_t, sb), lambda: rd.TraceAreaPathsTorch(tlas, rays, keys[:-1], max_depth, lights_t, area_t, sb),
       lambda: rd.TraceAreaPathsTorch(tlas, rays, keys, -1, lights_t, area_t, sb), lambda: rd.TraceAreaPathsTorch(tlas, rays, keys, max_depth, lights_t, area_t, (1, 2)),
       lambda: rd.AreaLightHitsTorch(t, mat0, area_t, 3, keys=keys_t), lambda: rd.AreaLightHitsTorch(t, mat0, area_t, -1, keys=keys_t),
       lambda: rd.AreaLightHitsTorch(t, mat0, area_t.double(), 0, keys=keys_t), lambda: rd.AreaLightHitsTorch(t, mat0, area_t[:, :8], 0, keys=keys_t),
       lambda: rd.AreaLightHitsTorch(t, mat0, area_t.cpu(), 0, keys=keys_t), lambda: rd.AreaLightHitsTorch(t.cpu(), mat0, area_t, 0, keys=keys_t),
       lambda: rd.AreaLightHitsTorch(t, mat0[:-1], area_t, 0, keys=keys_t), lambda: rd.AreaLightHitsTorch(t, mat0, area_t, 1.5, keys=keys_t),
       lambda: rd.AreaLightHitsTorch(t, mat0, area_t, 0), lambda: rd.AreaLightHitsTorch(t, mat0, area_t, 0, keys=keys_t, randoms=rnd_t),
       lambda: rd.AreaLightHitsTorch(t, mat0, area_t, 0, keys=keys_t[:-1]), lambda: rd.AreaLightHitsTorch(t, mat0, area_t, 0, keys=keys_t.float()),
       lambda: rd.AreaLightHitsTorch(t, mat0, area_t, 0, randoms=rnd_t[:, :3]), lambda: rd.AreaLightHitsTorch(t, mat0, area_t, 0, keys=keys_t, stream=0xffff)]
for j, fn in enumerate(bad):
    try:
        fn()
    except rd.RadianceError:
        continue
    raise AssertionError("bad argument set %d was accepted" % j)
print("TORCH-AREA-OK", npix, shown)
"""


def test_torch_tensors_in_a_fresh_process(gpu):
    """rd.AreaLightHitsTorch and rd.TraceAreaPathsTorch equal the buffer route bit for bit, and the README's loop over
    rd.PunctualLightHitsTorch and rd.AreaLightHitsTorch equals rd.TraceAreaPathsTorch; a wrong dtype, shape or device is refused in
    Python.  torch is initialised first, in a process of its own (as tests/test_gpu_materials.py)"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _TORCH_CHILD, ROOT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "TORCH-AREA-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])

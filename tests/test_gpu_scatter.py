"""GPU suite (-m gpu): rd.ScatterHits / rd.ScatterHitsTorch (rdx_scatter_hits) -- the next-direction sample of the stock closest-hit
shader `material`, nextFactor and the choice between the two offset origins, on the records of rd.ResolveMaterials and
rd.ResolveHits, on the device.

Comparands: rd.ShadeHits (rdx_shade_hits), whose bytes 32 .. 47 of a shade record and whose `next` records are what this call
writes; the reference's recorded payloads (shade_cases.Golden.mat_pay) directly; and, at the edges of the inputs, the reference's
recordings of tests/golden/refgpu_shade_edges.npz under shade_edge_cases.compare.  The inputs are the 2048 recorded rays of c0 / c1
/ c2 and the edge batches.  Every bar is equality of bits unless it says otherwise.

The identities with rd.ShadeHits and the recordings are stated for hits whose SBT row is `material`, that is instanceSBTOffset 0
(a material record says nothing about the row); all fixture scenes are such.

That these tests notice a wrong kernel was checked with a local mutation (never committed): the `above` / `below` choice of
k_scatter_hits swapped (`dot3(nd, N) < 0 ? above : below`) -- test_against_shade_hits, test_against_the_recorded_payloads,
test_both_origins_occur, test_edges and test_frames_without_shade_hits fail.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_cases as gc
import material_cases as mc
import oracle_bind as ob
import scatter_cases as sc
import shade_cases as sh
import shade_edge_cases as se

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F = np.float32
same, bits = sc.same, sc.bits


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
    """query + ShadeHits + shadow query of a golden scene's 2048 recorded rays, (not compacting, compacting); computed once"""
    rd, _ = mods
    cache = {}

    def get(name):
        if name not in cache:
            c = golden(name)
            a = (c.dev.plt, c.dev.topAccelStruct, c.dev.shading_buffers(), c.mat_rays, c.keys)
            cache[name] = (sh.shade_batch(rd, *a), sh.shade_batch(rd, *a, compact=True))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def scattered(mods, golden):
    """query + ResolveHits + ResolveMaterials + ScatterHits (keys) of the same rays -> (records, not compacting, compacting)"""
    rd, _ = mods
    cache = {}

    def get(name):
        if name not in cache:
            c = golden(name)
            rec = sc.records(rd, c.dev, c.mat_rays)
            cache[name] = (rec, sc.scatter(rd, c.dev.plt, rec, keys=c.keys), sc.scatter(rd, c.dev.plt, rec, keys=c.keys, compact=True))
        return cache[name]
    return get


# ---- 1. against rdx_shade_hits --------------------------------------------------------------------------------------------------------
# misses among the 2048 recorded rays, counted from the fixtures on the CPU: every ray of c1 (a closed room) hits, so "misses
# included" is exercised on c0 and c2 -- and, at other batch sizes, by test_shapes and test_offsets_and_refusals
RECORDED_MISSES = {"c0": 1501, "c1": 0, "c2": 128}


@pytest.mark.parametrize("name", gc.SCENES)
def test_against_shade_hits(golden, shaded, scattered, name):
    """scatter[i] is bytes 32 .. 47 of shade[i], misses included; `next` and `live` are ShadeHits'; compacting: the same live, src a
    permutation of the hit rows with every block of 64 contiguous and ascending, and the next ray of every hit is ShadeHits'"""
    r, rc = shaded(name)
    rec, s, c = scattered(name)
    hit = rec["mat"]["hit"] == 1
    assert r["invalid"] == 0 and same(rec["q"], r["q"])
    assert int(hit.sum()) >= 100 and int((~hit).sum()) == RECORDED_MISSES[name] and (name == "c1" or RECORDED_MISSES[name] >= 1), name
    assert np.array_equal(hit, golden(name).mat_hits["hit"] == 1), name
    assert mc.all_finite(s["scatter"]["nextFactor"], s["next"]["origin"], s["next"]["direction"], r["shade"]["nextFactor"])
    assert same(s["scatter"], sc.shade_scatter(r["shade"])), "%s: scatter records differ from bytes 32 .. 47 of the shade records" % name
    assert same(s["next"], r["next"]), "%s: next rays" % name
    assert s["live"] == r["live"] == int(hit.sum())
    assert not s["next"][~hit].view(np.uint8).any() and (s["scatter"]["slot"][hit] == np.flatnonzero(hit)).all()
    # compacting
    sc.check_compacted(c, s, hit, name)
    assert c["live"] == rc["live"]
    sc.check_src(rc["src"], hit, name + " (ShadeHits)")
    assert same(c["next"][c["scatter"]["slot"][hit]], rc["next"][rc["shade"]["slot"][hit]]), "%s: compacted next rays" % name
    assert mc.all_finite(c["next"]["origin"], c["next"]["direction"])
    print("%s: %d hits, %d misses" % (name, int(hit.sum()), int((~hit).sum())))


# ---- 2. against the reference's recordings directly -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.SCENES)
def test_against_the_recorded_payloads(golden, scattered, name):
    """on every recorded hit, nextFactor / nextRayOrigin / nextRayDirection equal Golden.mat_pay"""
    c = golden(name)
    rec, s, _ = scattered(name)
    k = c.mat_hits["hit"] == 1
    assert np.array_equal(rec["mat"]["hit"] == 1, k) and int(k.sum()) >= 100
    slot = s["scatter"]["slot"][k]
    for f, got in (("nextFactor", s["scatter"]["nextFactor"][k]), ("nextRayOrigin", s["next"]["origin"][slot]), ("nextRayDirection", s["next"]["direction"][slot])):
        want = c.mat_pay[f][k]
        eq = (bits(got) == bits(want)).all(1)
        assert eq.all(), "%s: %s differs from the recording on %d of %d hits" % (name, f, int((~eq).sum()), eq.shape[0])
    assert (bits(s["next"]["tmin"][slot]) == bits(F(0.001))).all() and (bits(s["next"]["tmax"][slot]) == bits(F(1000.0))).all()


# ---- 3. both origins occur ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.SCENES)
def test_both_origins_occur(scattered, name):
    """a survivor's origin has the bits of surf.below where dot(nd, N) < 0 and of mat.above elsewhere, on every hit, and both occur
    in every c-scene -- as they do on the edge batch "keys" (test_edges), whose keys send the transmissive material's rays
    through the surface by construction"""
    rec, s, _ = scattered(name)
    n_below, n_above = origins(rec, s, name)
    print("%s: %d next rays start below the surface, %d above" % (name, n_below, n_above))
    assert n_below > 0 and n_above > 0


def origins(rec, s, tag):
    """-> (below, above) counts; asserts that every survivor's origin is the one the sign of dot(nd, N) names (the dot in float64:
    rows whose float32 dot could round to the other side of zero are required to carry one of the two)"""
    mat, surf = rec["mat"], rec["surf"]
    hit = mat["hit"] == 1
    nxt = s["next"][s["scatter"]["slot"][hit]]
    is_below = (bits(nxt["origin"]) == bits(surf["below"][hit])).all(1)
    is_above = (bits(nxt["origin"]) == bits(mat["above"][hit])).all(1)
    assert (is_below | is_above).all(), "%s: an origin that is neither `below` nor `above`" % tag
    with np.errstate(invalid="ignore", over="ignore"):
        dot = (nxt["direction"].astype(np.float64) * mat["normal"][hit].astype(np.float64)).sum(1)
        scale = np.abs(nxt["direction"].astype(np.float64) * mat["normal"][hit].astype(np.float64)).sum(1)
    clear = np.isfinite(dot) & (np.abs(dot) > 1e-5 * scale)
    assert is_below[clear & (dot < 0)].all() and is_above[clear & (dot > 0)].all(), "%s: the wrong side" % tag
    distinct = (bits(surf["below"][hit]) != bits(mat["above"][hit])).any(1)
    return int((is_below & distinct).sum()), int((is_above & distinct).sum())


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------------
class Edge:
    def __init__(self, rd, scenes):
        self.G = dict(np.load(os.path.join(GOLD, "refgpu_shade_edges.npz")))
        self.s, self.inst, self.B = se.batches(scenes)
        self.dev = scenes.DeviceScene(self.s)
        blob = rd.ReadBuffer(self.dev.plt, self.dev.topAccelStruct, self.dev.topAccelStruct.size).tobytes()
        assert np.array_equal(gc.sha(blob), self.G["blob_sha256"]), "the TLAS blob of the edge scene changed"
        light0 = sh.upload(rd, self.dev.plt, se.light_buffers(rd)[0:1])
        self.sb = self.dev.shading_buffers()
        self.sb.scene = light0


@pytest.fixture(scope="module")
def edge(mods):
    return Edge(*mods)


LEFT_OUT = {"main": (20, 2376), "s-25": (4, 396), "s+25": (4, 396), "keys": (0, 198)}       # zero_normal_rows of hits, counted from the fixture on the CPU


@pytest.mark.parametrize("name", ("main", "s-25", "s+25", "keys"))
def test_edges(mods, edge, name):
    """the edge batches against the reference's recordings under shade_edge_cases.compare (a NaN of the reference wants a NaN);
    only nextFactor is left out, and only on zero_normal_rows; the next ray is compared on every hit"""
    rd, _ = mods
    e = edge
    b = e.B[name]
    u = se.unpack_batch(e.G, name, b.n, ob.PAYLOAD_DTYPE)
    left = se.zero_normal_rows(e.s, e.inst, u["inst"], u["prim"], u["bary"])
    assert (int(left.sum()), int(u["hit"].sum())) == LEFT_OUT[name]
    plt, tlas = e.dev.plt, e.dev.topAccelStruct
    rays = sh.rays_of(rd, b.o, b.d, b.tmin, b.tmax)
    n = b.n
    bR = sh.upload(rd, plt, rays)
    bH = rd.QueryRays(tlas, bR, n, rd.QUERY_CLOSEST)
    bS, inv_s = rd.ResolveHits(tlas, bR, bH, n, e.dev.surface_buffers())
    bM, inv_m = rd.ResolveMaterials(tlas, bR, bH, n, e.sb)
    assert inv_s == 0 and inv_m == 0
    rec = dict(bR=bR, bM=bM, bS=bS, n=n, mat=sh.read(rd, plt, bM, n, mc.MATERIAL_RECORD_DTYPE), surf=sh.read(rd, plt, bS, n, rd.SURFACE_DTYPE))
    s = sc.scatter(rd, plt, rec, keys=sh.keys_of(b.frames, b.pixels, b.depths.view(np.uint32)))
    k = u["hit"]
    assert np.array_equal(rec["mat"]["hit"] == 1, k) and s["live"] == int(k.sum())
    slot = s["scatter"]["slot"][k]
    assert np.array_equal(slot, np.flatnonzero(k)) and (s["scatter"]["slot"][~k] == sc.NO_SLOT).all()
    want = u["pay"]
    for f, got, out in (("nextFactor", s["scatter"]["nextFactor"][k], left), ("nextRayOrigin", s["next"]["origin"][slot], None),
                        ("nextRayDirection", s["next"]["direction"][slot], None)):
        ok = se.compare(got, want[f])[0]
        if out is not None:
            ok = ok | out
        assert ok.all(), "%s: %s differs on %d of %d hits (first: hit row %d, got %r, want %r)" % (
            name, f, int((~ok).sum()), ok.shape[0], int(np.flatnonzero(~ok)[0]), got[~ok][0].tolist(), want[f][~ok][0].tolist())
    assert not s["next"][~k].view(np.uint8).any() and not bits(s["scatter"]["nextFactor"][~k]).any()
    w = np.concatenate([want[f] for f in ("nextFactor", "nextRayOrigin", "nextRayDirection")], 1)
    print("scatter/%s: %d rows compared, reference NaN share %.4f, inf share %.4f, %d rows left out (nextFactor only); fixture"
          % (name, int(k.sum()), float(np.isnan(w).mean()), float(np.isinf(w).mean()), int(left.sum())))
    if name == "keys":      # item 3: both origins occur here (the transmissive material, from the front and from inside)
        n_below, n_above = origins(rec, s, "keys")
        print("scatter/keys: %d next rays start below the surface, %d above" % (n_below, n_above))
        assert n_below > 0 and n_above > 0


# ---- 5. randoms -----------------------------------------------------------------------------------------------------------------------
def test_randoms(mods, golden, scattered):
    """randoms = pcg3d of the keys, padded to float4 (w arbitrary), gives the bytes of the keys route; other randoms give other rays"""
    rd, _ = mods
    c = golden("c1")
    rec, s, cs = scattered("c1")
    hit = rec["mat"]["hit"] == 1
    u = sc.key_randoms(rd, c.keys, w=123.0)
    got = sc.scatter(rd, c.dev.plt, rec, randoms=u)
    assert same(got["scatter"], s["scatter"]) and same(got["next"], s["next"]) and got["live"] == s["live"]
    sc.check_compacted(sc.scatter(rd, c.dev.plt, rec, randoms=u, compact=True), s, hit, "randoms")
    other = sc.randoms_of(np.random.default_rng(5).random((hit.shape[0], 3), np.float32))
    got2 = sc.scatter(rd, c.dev.plt, rec, randoms=other)
    assert got2["live"] == s["live"] and np.array_equal(got2["scatter"]["slot"], s["scatter"]["slot"])
    differ = (bits(got2["next"]["direction"][hit]) != bits(s["next"]["direction"][hit])).any(1)
    assert differ.all(), "%d of %d next directions did not change with the randoms" % (int((~differ).sum()), differ.shape[0])
    assert mc.all_finite(got2["next"]["direction"], got2["scatter"]["nextFactor"])


# ---- 6. frames ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.SCENES)
def test_frames_without_shade_hits(mods, golden, name, monkeypatch):
    """the raygen loop with each bounce's colour from ResolveMaterials + LightHits(0) + the any-hit query + the ambient term and
    hit / nextFactor / next ray from ScatterHits (compacting), no rd.ShadeHits call anywhere: imageScratch of both progressive
    frames equals the reference's recorded frames"""
    rd, _ = mods
    c = golden(name)
    dev, p = c.dev, c.s.rtprop
    dev.bind()

    def no_shade_hits(*a, **kw):
        raise AssertionError("rd.ShadeHits was called")
    monkeypatch.setattr(rd, "ShadeHits", no_shade_hits)
    calls = []
    generate, bounce = sc.gpu_callables(rd, dev, calls)
    got = sh.compose_frames(dev.width * dev.height, 0, int(p["batchSize"]), int(p["depth"]), 2, generate, bounce)
    assert len(calls) >= 2
    for f in range(2):
        want = np.ascontiguousarray(c.G["scratch%d" % f]).reshape(-1, 4)
        assert mc.all_finite(got[f], want)
        eq = (bits(got[f]) == bits(want)).all(1)
        assert eq.all(), "%s frame %d: %d of %d pixels differ from the recording" % (name, f, int((~eq).sum()), eq.shape[0])


# ---- 7. shapes ------------------------------------------------------------------------------------------------------------------------
def test_shapes(mods, golden, scattered):
    """n in {0, 1, 63, 64, 65, 255, 256, 257} from row 700 of c0 (hits and misses), with and without src: the corresponding rows of
    the 2048-record run; the compacted runs through src"""
    rd, _ = mods
    c = golden("c0")
    rec, full, _ = scattered("c0")
    plt = c.dev.plt
    first = 700
    hit_all = rec["mat"]["hit"] == 1
    assert 0 < int(hit_all[first:first + 257].sum()) < 257
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        rows = slice(first, first + n)
        hit = hit_all[rows]
        keys = c.keys[rows] if n else np.zeros(1, sh.SHADE_KEY_DTYPE)
        want = dict(scatter=full["scatter"][rows].copy(), next=full["next"][rows], live=int(hit.sum()))
        want["scatter"]["slot"][hit] -= first
        got = sc.scatter(rd, plt, rec, keys=keys, n=n, first=first)
        assert got["live"] == want["live"] and same(got["scatter"], want["scatter"]) and same(got["next"], want["next"]), n
        comp = sc.scatter(rd, plt, rec, keys=keys, n=n, first=first, compact=True)
        sc.check_compacted(comp, want, hit, "n = %d" % n)


# ---- 8. offsets and refusals ----------------------------------------------------------------------------------------------------------
def _refusals(rd, run, cases, snapshot, good, symbol):
    for what, kw, word in cases:
        with pytest.raises(rd.RadianceError) as e:
            run(**kw)
        assert word in str(e.value) and symbol in str(e.value), (what, str(e.value))
        now = snapshot()
        for k in now:
            assert np.array_equal(now[k], good[k]), (what, k)


def test_offsets_and_refusals(mods, golden, scattered):
    """n = 200 of c0's records (rows 700 .., hits and misses) at distinct non-zero offsets in buffers filled with 0xA5: the records
    equal the plain call's and no byte outside the written ranges is touched, `next` / `src` from `live` on included when
    compacting; n == 0 touches nothing; one refusal of each kind, after each of which every buffer is unchanged; adjacent ranges
    of one buffer work"""
    rd, _ = mods
    c = golden("c0")
    rec, full, _ = scattered("c0")
    plt = c.dev.plt
    n, tail, first = 200, 128, 700
    rows = slice(first, first + n)
    rays, mats, surfs, keys = c.mat_rays[rows], rec["mat"][rows], rec["surf"][rows], c.keys[rows]
    plain = dict(scatter=full["scatter"][rows].copy(), next=full["next"][rows])
    plain["scatter"]["slot"][mats["hit"] == 1] -= first
    off = dict(rays=96, mat=192, surf=64, keys=48, rnd=80, scatter=32, next=160, src=20)
    rec_size = dict(rays=32, mat=64, surf=64, keys=16, rnd=16, scatter=16, next=32, src=4)
    B = {k: rd.CreateBuffer(plt, off[k] + rec_size[k] * n + tail) for k in off}
    fill = lambda buf: rd.WriteBuffer(plt, buf, buf.size, np.full(buf.size, 0xA5, np.uint8))
    for buf in B.values():
        fill(buf)
    u = sc.key_randoms(rd, keys)
    for k, data in (("rays", rays), ("mat", mats), ("surf", surfs), ("keys", keys), ("rnd", u)):
        rd.WriteBuffer(plt, B[k], rec_size[k] * n, data, offset=off[k])
    snapshot = lambda: {k: rd.ReadBuffer(plt, B[k], B[k].size).copy() for k in B}
    hit = mats["hit"] == 1
    live = int(hit.sum())
    assert 0 < live < n

    def run(**kw):
        a = dict(rays=B["rays"], materials=B["mat"], surfaces=B["surf"], keys=B["keys"], n=n, randoms=None, scatter=B["scatter"], next=B["next"], src=None,
                 rays_offset=off["rays"], materials_offset=off["mat"], surfaces_offset=off["surf"], keys_offset=off["keys"], randoms_offset=off["rnd"],
                 scatter_offset=off["scatter"], next_offset=off["next"], src_offset=off["src"])
        a.update(kw)
        return rd.ScatterHits(a.pop("rays"), a.pop("materials"), a.pop("surfaces"), a.pop("keys"), a.pop("n"), **a)

    def outputs_are(now, src):
        lo, hi = off["scatter"], off["scatter"] + 16 * n
        got = now["scatter"][lo:hi].view(sc.SCATTER_DTYPE)
        assert (now["scatter"][:lo] == 0xA5).all() and (now["scatter"][hi:] == 0xA5).all()
        assert same(got["nextFactor"], plain["scatter"]["nextFactor"][:n])
        m = live if src else n
        lo, hi = off["next"], off["next"] + 32 * m
        assert (now["next"][:lo] == 0xA5).all() and (now["next"][hi:] == 0xA5).all(), "next: a byte outside records 0 .. %d changed" % m
        nxt = now["next"][lo:hi].view(rd.RAY_DTYPE)
        if src:
            lo, hi = off["src"], off["src"] + 4 * live
            assert (now["src"][:lo] == 0xA5).all() and (now["src"][hi:] == 0xA5).all(), "src: a byte outside records 0 .. live changed"
            s = now["src"][lo:hi].view("<u4")
            sc.check_compacted(dict(scatter=got, next=nxt, src=s, live=live), dict(scatter=plain["scatter"][:n], next=plain["next"][:n], live=live), hit, "offsets")
        else:
            assert (now["src"] == 0xA5).all()
            assert same(got, plain["scatter"][:n]) and same(nxt, plain["next"][:n])

    before = snapshot()
    assert run() == (B["scatter"], B["next"], None, live)
    after = snapshot()
    for k in ("rays", "mat", "surf", "keys", "rnd"):
        assert np.array_equal(after[k], before[k]), k
    outputs_are(after, False)
    for k in ("scatter", "next"):
        fill(B[k])
    assert run(keys=None, randoms=B["rnd"]) == (B["scatter"], B["next"], None, live)        # the randoms route at its own offset
    outputs_are(snapshot(), False)
    for k in ("scatter", "next"):
        fill(B[k])
    assert run(src=B["src"]) == (B["scatter"], B["next"], B["src"], live)
    outputs_are(snapshot(), True)
    # n == 0 touches nothing
    for k in ("scatter", "next", "src"):
        fill(B[k])
    assert run(n=0, src=B["src"]) == (B["scatter"], B["next"], B["src"], 0)
    assert all((rd.ReadBuffer(plt, B[k], B[k].size) == 0xA5).all() for k in ("scatter", "next", "src"))
    run()
    good = snapshot()

    # rays | materials | surfaces | keys | room for outputs, for the overlap cases
    one = rd.CreateBuffer(plt, 32 * n * 12)
    at = dict(rays=0, mat=32 * n, surf=96 * n, keys=160 * n, scatter=176 * n, next=192 * n, src=224 * n)
    for k, data in (("rays", rays), ("mat", mats), ("surf", surfs), ("keys", keys)):
        rd.WriteBuffer(plt, one, rec_size[k] * n, data, offset=at[k])
    in_one = dict(rays=one, materials=one, surfaces=one, keys=one, rays_offset=at["rays"], materials_offset=at["mat"], surfaces_offset=at["surf"],
                  keys_offset=at["keys"])
    null, unknown = rd.Buffer(None, 1 << 20), rd.Buffer(12345678, 1 << 20)
    wrapped = lambda k, shift, size: rd.WrapDeviceMemory(plt, B[k].device_ptr + shift, size, keepalive=B[k])
    _refusals(rd, run, [
        ("rays_offset 8", dict(rays_offset=8), "16"), ("materials_offset 8", dict(materials_offset=8), "16"), ("surfaces_offset 24", dict(surfaces_offset=24), "16"),
        ("keys_offset 4", dict(keys_offset=4), "16"), ("randoms_offset 8", dict(keys=None, randoms=B["rnd"], randoms_offset=8), "16"),
        ("scatter_offset 8", dict(scatter_offset=8), "16"), ("next_offset 16 + 8", dict(next_offset=24), "16"), ("src_offset 2", dict(src=B["src"], src_offset=2), "4 for src"),
        ("rays past the end", dict(rays_offset=off["rays"] + tail + 16), "ray buffer"),
        ("material records past the end", dict(materials_offset=off["mat"] + tail + 16), "material-record buffer"),
        ("surface records past the end", dict(surfaces_offset=off["surf"] + tail + 16), "surface-record buffer"),
        ("keys past the end", dict(keys_offset=off["keys"] + tail + 16), "key buffer"),
        ("randoms past the end", dict(keys=None, randoms=B["rnd"], randoms_offset=off["rnd"] + tail + 16), "randoms buffer"),
        ("scatter past the end", dict(scatter_offset=off["scatter"] + tail + 16), "scatter buffer"),
        ("next one record short", dict(next=rd.CreateBuffer(plt, 32 * n - 16), next_offset=0), "next-ray buffer"),
        ("src past the end", dict(src=B["src"], src_offset=off["src"] + tail + 4), "src buffer"),
        ("scatter over the rays", dict(in_one, scatter=one, scatter_offset=32 * n - 16), "overlap"),
        ("scatter over the material records", dict(in_one, scatter=one, scatter_offset=96 * n - 16), "overlap"),
        ("next over the surface records", dict(in_one, next=one, next_offset=160 * n - 32), "overlap"),
        ("next over the keys", dict(in_one, next=one, next_offset=176 * n - 16), "overlap"),
        ("next over scatter", dict(scatter=one, scatter_offset=at["scatter"], next=one, next_offset=at["next"] - 16), "overlap"),
        ("src over next", dict(next=one, next_offset=at["next"], src=one, src_offset=at["src"] - 4), "overlap"),
        ("null rays", dict(rays=null), "ray buffer handle"), ("unknown materials", dict(materials=unknown), "material-record buffer handle"),
        ("null surfaces", dict(surfaces=null), "surface-record buffer handle"), ("null scatter", dict(scatter=null), "scatter buffer handle"),
        ("unknown next", dict(next=unknown), "next-ray buffer handle"), ("unknown keys", dict(keys=unknown), "key buffer handle"),
        ("unknown randoms", dict(keys=None, randoms=unknown), "randoms buffer handle"), ("unknown src", dict(src=unknown), "src buffer handle"),
        ("misaligned wrapped rays", dict(rays=wrapped("rays", 8, 32 * n + 64), rays_offset=16), "aligned"),
        ("misaligned wrapped scatter", dict(scatter=wrapped("scatter", 4, 16 * n + 32), scatter_offset=0), "aligned"),
        ("misaligned wrapped src", dict(src=wrapped("src", 2, 4 * n + 32), src_offset=0), "aligned"),
    ], snapshot, good, "rdx_scatter_hits")
    # both / neither of keys and randoms at the C ABI (rd.ScatterHits refuses them before the library sees them)
    from radiance_ray_tracing_amd import _lib
    L = _lib.lib()
    h = lambda k: B[k].handle
    for hk, hu, word in ((None, None, "neither"), (h("keys"), h("rnd"), "both")):
        assert L.rdx_scatter_hits(h("rays"), off["rays"], h("mat"), off["mat"], h("surf"), off["surf"], hk, off["keys"], hu, off["rnd"], n, h("scatter"),
                                  off["scatter"], h("next"), off["next"], None, 0, None) != 0
        assert word in _lib.last_error() and "rdx_scatter_hits" in _lib.last_error()
    assert all(np.array_equal(v, good[k]) for k, v in snapshot().items())
    for fn in (lambda: run(keys=None), lambda: run(randoms=B["rnd"]), lambda: run(scatter=7), lambda: run(next=7), lambda: run(src=7), lambda: run(rays=None)):
        with pytest.raises(rd.RadianceError):
            fn()
    # adjacent ranges of one buffer are fine, and the call still works after the refusals
    got = rd.ScatterHits(one, one, one, one, n, scatter=one, next=one, src=one, rays_offset=at["rays"], materials_offset=at["mat"], surfaces_offset=at["surf"],
                         keys_offset=at["keys"], scatter_offset=at["scatter"], next_offset=at["next"], src_offset=at["src"])
    assert got == (one, one, one, live)
    sc.check_compacted(dict(scatter=rd.ReadBuffer(plt, one, 16 * n, offset=at["scatter"]).view(sc.SCATTER_DTYPE),
                            next=rd.ReadBuffer(plt, one, 32 * live, offset=at["next"]).view(rd.RAY_DTYPE),
                            src=rd.ReadBuffer(plt, one, 4 * live, offset=at["src"]).view("<u4"), live=live),
                       dict(scatter=plain["scatter"][:n], next=plain["next"][:n], live=live), hit, "adjacent ranges")
    for k, data in (("rays", rays), ("mat", mats), ("surf", surfs), ("keys", keys)):
        assert same(rd.ReadBuffer(plt, one, rec_size[k] * n, offset=at[k]), data), k
    st = rd.GetTraceStats()
    assert st.ms_shade > 0.0


# ---- 9. caller-filled records ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compact", (False, True))
def test_caller_filled_records(mods, golden, scattered, compact):
    """hit = 2 gives (0, 0, 0, 0xffffffff) and no survivor; hit = 1 with NaN / inf / zero / 3e38 normals writes only its own ranges
    (the kernel gathers nothing, so there is nothing a record could make it read); untouched rows keep their bits"""
    rd, _ = mods
    c = golden("c1")
    rec, plain, _ = scattered("c1")
    plt = c.dev.plt
    n, lead, tail = 200, 64, 128
    own = rec["mat"][:n].copy()
    own["hit"][0::4] = 2
    garbage = np.arange(n) % 4 == 1
    own["hit"][garbage] = 1
    own["normal"][garbage] = np.resize(np.array([[np.nan, 0, 0], [np.inf, -np.inf, 0], [0, 0, 0], [3e38, 3e38, 3e38], [1e-42, 0, 0]], F), (int(garbage.sum()), 3))
    alive = own["hit"] == 1
    live = int(alive.sum())
    untouched = (np.arange(n) % 4 >= 2) & alive
    assert untouched.any() and (own["hit"][np.arange(n) % 4 >= 2] == rec["mat"]["hit"][:n][np.arange(n) % 4 >= 2]).all()
    size = dict(scatter=16, next=32, src=4)
    B = {k: rd.CreateBuffer(plt, lead + size[k] * n + tail) for k in size}
    for buf in B.values():
        rd.WriteBuffer(plt, buf, buf.size, np.full(buf.size, 0xA5, np.uint8))
    _, _, _, got_live = rd.ScatterHits(sh.upload(rd, plt, c.mat_rays[:n]), sh.upload(rd, plt, own), sh.upload(rd, plt, rec["surf"][:n]),
                                       sh.upload(rd, plt, c.keys[:n]), n, scatter=B["scatter"], next=B["next"], src=B["src"] if compact else None,
                                       scatter_offset=lead, next_offset=lead, src_offset=lead)
    assert got_live == live
    now = {k: rd.ReadBuffer(plt, B[k], B[k].size).copy() for k in B}
    written = dict(scatter=n, next=live if compact else n, src=live if compact else 0)
    for k in B:
        lo, hi = lead, lead + size[k] * written[k]
        assert (now[k][:lo] == 0xA5).all() and (now[k][hi:] == 0xA5).all(), k
    s = now["scatter"][lead:lead + 16 * n].view(sc.SCATTER_DTYPE)
    nxt = now["next"][lead:lead + 32 * written["next"]].view(rd.RAY_DTYPE)
    dead = ~alive
    assert not bits(s["nextFactor"][dead]).any() and (s["slot"][dead] == sc.NO_SLOT).all()
    slot = s["slot"][alive]
    if compact:
        src = now["src"][lead:lead + 4 * live].view("<u4")
        sc.check_src(src, alive, "caller-filled")
        assert np.array_equal(src[slot], np.flatnonzero(alive))
    else:
        assert np.array_equal(slot, np.flatnonzero(alive)) and not np.ascontiguousarray(nxt[dead]).view(np.uint8).any()
    assert same(s["nextFactor"][untouched], plain["scatter"]["nextFactor"][:n][untouched])
    assert same(nxt[s["slot"][untouched]], plain["next"][:n][untouched])
    g = nxt[s["slot"][garbage]]
    assert (bits(g["tmin"]) == bits(F(0.001))).all() and (bits(g["tmax"]) == bits(F(1000.0))).all()
    is_below = (bits(g["origin"]) == bits(rec["surf"]["below"][:n][garbage])).all(1)
    is_above = (bits(g["origin"]) == bits(own["above"][garbage])).all(1)
    assert (is_below | is_above).all()


# ---- 10. torch variant ----------------------------------------------------------------------------------------------------------------
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
import material_cases as mc
import scatter_cases as sc
import shade_cases as sh
c = sh.Golden(rd, scenes, "c1")
dev, n = c.dev, c.mat_rays.shape[0]
tlas, sb, sf = dev.topAccelStruct, dev.shading_buffers(), dev.surface_buffers()
rec = sc.records(rd, dev, c.mat_rays)
want = sc.scatter(rd, dev.plt, rec, keys=c.keys)
hit = rec["mat"]["hit"] == 1
assert 0 < int(hit.sum())
# the tensor route, on tensors a torch op produced
t = (torch.from_numpy(c.mat_rays.view(np.float32).reshape(n, 8).copy()).cuda() * torch.ones(8, device="cuda")).contiguous()
keys = torch.from_numpy(c.keys.view(np.uint32).reshape(n, 4).astype(np.int64)).cuda().to(torch.int32).contiguous()
h = rd.QueryRaysTorch(tlas, t, rd.QUERY_CLOSEST)
mat, _ = rd.ResolveMaterialsTorch(tlas, t, h, sb)
surf, _ = rd.ResolveHitsTorch(tlas, t, h, sf)
scatter, nxt, src, live = rd.ScatterHitsTorch(t, mat, surf, keys, compact=False)
assert src is None and live == want["live"] and scatter.dtype == torch.float32 and tuple(scatter.shape) == (n, 4) and tuple(nxt.shape) == (n, 8)
assert np.array_equal(scatter.cpu().numpy().view(np.uint32), want["scatter"].view(np.uint32).reshape(n, 4))
assert np.array_equal(nxt.cpu().numpy().view(np.uint32), want["next"].view(np.uint32).reshape(n, 8))
scatter, nxt, src, live = rd.ScatterHitsTorch(t, mat, surf, keys)
assert live == want["live"] and tuple(nxt.shape) == (live, 8) and tuple(src.shape) == (live,) and src.dtype == torch.int32
sc.check_compacted(dict(scatter=scatter.cpu().numpy().view(sc.SCATTER_DTYPE).reshape(-1), next=nxt.cpu().numpy().view(rd.RAY_DTYPE).reshape(-1),
                        src=src.cpu().numpy().view(np.uint32), live=live), want, hit, "torch")
u = torch.from_numpy(sc.key_randoms(rd, c.keys).view(np.float32).reshape(n, 4).copy()).cuda()
s2, n2, none, live2 = rd.ScatterHitsTorch(t, mat, surf, randoms_t=u, compact=False)
assert none is None and live2 == live and torch.equal(n2.view(torch.int32), torch.from_numpy(want["next"].view(np.int32).reshape(n, 8)).cuda())
assert np.array_equal(s2.cpu().numpy().view(np.uint32), want["scatter"].view(np.uint32).reshape(n, 4))
e = rd.ScatterHitsTorch(t[:0], mat[:0], surf[:0], keys[:0])
assert tuple(e[0].shape) == (0, 4) and tuple(e[1].shape) == (0, 8) and tuple(e[2].shape) == (0,) and e[3] == 0

# the README's path tracer over the three lights, 3 bounces, against the same loop on buffers folded in numpy float32
light_count, max_depth = 3, 3
scene3 = sh.upload(rd, dev.plt, np.array(mc.three_lights(rd)).reshape(1))
sb3 = dev.shading_buffers()
sb3.scene = scene3
rays = t.clone()
frame_of, pixel = keys[:, 0].contiguous(), keys[:, 1].contiguous()
color = torch.zeros((n, 4), device="cuda")
weight = torch.ones((n, 3), device="cuda")
path = torch.arange(n, device="cuda")
miss_colour = torch.tensor([0.2, 0.2, 0.5], device="cuda")
lives = []
for depth in range(max_depth):
    k = torch.stack([frame_of, pixel, torch.full_like(pixel, depth), torch.zeros_like(pixel)], 1).contiguous()
    hits = rd.QueryRaysTorch(tlas, rays, rd.QUERY_CLOSEST)
    surf, _ = rd.ResolveHitsTorch(tlas, rays, hits, sf)
    mat, _ = rd.ResolveMaterialsTorch(tlas, rays, hits, sb3)
    if depth == 0:
        color[path[mat.view(torch.int32)[:, 3] != 1], :3] = miss_colour
    direct = torch.zeros((rays.shape[0], 3), device="cuda")
    for j in range(light_count):
        lit, shadow = rd.LightHitsTorch(rays, mat, sb3.scene, j)
        occluded = rd.QueryRaysTorch(tlas, shadow, rd.QUERY_ANY)[:, 3:4] == 1
        direct += torch.where(occluded, torch.zeros_like(lit[:, :3]), lit[:, :3])
    radiance = direct + mat[:, 4:7] * 0.1
    scatter, rays, src, live = rd.ScatterHitsTorch(rays, mat, surf, k)
    src = src.long()
    color[path[src], :3] += weight[path[src]] * radiance[src]
    weight[path[src]] *= scatter[src, 0:3]
    path, pixel, frame_of = path[src], pixel[src].contiguous(), frame_of[src].contiguous()
    lives.append(live)
    if live == 0:
        break
ref_color, ref_weight, ref_lives = sc.path_tracer_numpy(rd, dev, scene3, light_count, c.mat_rays, c.keys["frameID"], c.keys["pixel"], max_depth)
assert lives == ref_lives and len(lives) == max_depth and lives[-1] > 0, (lives, ref_lives)
assert np.isfinite(ref_color).all() and np.isfinite(ref_weight).all()
assert np.array_equal(color[:, :3].cpu().numpy().view(np.uint32), ref_color.view(np.uint32))
assert np.array_equal(weight.cpu().numpy().view(np.uint32), ref_weight.view(np.uint32))
assert not color[:, 3].any()

bad = [lambda: rd.ScatterHitsTorch(t[:, :7], mat, surf, keys), lambda: rd.ScatterHitsTorch(t.double(), mat, surf, keys),
       lambda: rd.ScatterHitsTorch(t.cpu(), mat, surf, keys), lambda: rd.ScatterHitsTorch(c.mat_rays, mat, surf, keys)]
t2, h2 = t, rd.QueryRaysTorch(tlas, t, rd.QUERY_CLOSEST)
mat, _ = rd.ResolveMaterialsTorch(tlas, t2, h2, sb)
surf, _ = rd.ResolveHitsTorch(tlas, t2, h2, sf)
bad += [lambda: rd.ScatterHitsTorch(t, mat[:, :8], surf, keys), lambda: rd.ScatterHitsTorch(t, mat.double(), surf, keys),
        lambda: rd.ScatterHitsTorch(t, mat.cpu(), surf, keys), lambda: rd.ScatterHitsTorch(t, mat[:-1], surf, keys),
        lambda: rd.ScatterHitsTorch(t, mat, surf[:, :8], keys), lambda: rd.ScatterHitsTorch(t, mat, surf.cpu(), keys),
        lambda: rd.ScatterHitsTorch(t, mat, surf[:-1], keys), lambda: rd.ScatterHitsTorch(t, mat, surf, keys.float()),
        lambda: rd.ScatterHitsTorch(t, mat, surf, keys[:, :3]), lambda: rd.ScatterHitsTorch(t, mat, surf, keys.cpu()),
        lambda: rd.ScatterHitsTorch(t, mat, surf, keys[:-1]), lambda: rd.ScatterHitsTorch(t, mat, surf),
        lambda: rd.ScatterHitsTorch(t, mat, surf, keys, u), lambda: rd.ScatterHitsTorch(t, mat, surf, randoms_t=u.double()),
        lambda: rd.ScatterHitsTorch(t, mat, surf, randoms_t=u[:, :3]), lambda: rd.ScatterHitsTorch(t, mat, surf, randoms_t=u.cpu()),
        lambda: rd.ScatterHitsTorch(t, mat, surf, randoms_t=keys)]
for j, fn in enumerate(bad):
    try:
        fn()
    except rd.RadianceError:
        continue
    raise AssertionError("bad argument set %d was accepted" % j)
print("TORCH-SCATTER-OK", n, int(hit.sum()), lives)
"""


def test_torch_tensors_in_a_fresh_process(gpu):
    """rd.ScatterHitsTorch equals the buffer route bit for bit; the README's three-light path tracer, 3 bounces on c1, equals the same
    loop on buffers folded in numpy float32; wrong dtype, shape or device is refused in Python.  torch is initialised first, in a
    process of its own (as tests/test_gpu_shade.py)"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _TORCH_CHILD, ROOT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "TORCH-SCATTER-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
    print(out.stdout.strip().splitlines()[-1])

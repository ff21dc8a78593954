"""Shared pieces of the shading tests (test_shade_cpu.py, test_gpu_shade.py): rd.ShadeHits / rdx_shade_hits.

compose_frames is a numpy float32 restatement of the reference's raygen loop (samples/shader.cl:197-281) around two callables --
`generate` (generateRay for a batch of pixels) and `bounce` (one traceRay of the loop for a batch of rays: closest walk, closest-hit
or miss shader, the shader's shadow walk) -- one operation at a time under the contract of DESIGN.md section 2 (no contraction):

    color += contribution * payload.color; contribution *= payload.nextFactor         on a hit
    color = payload.color                                                             on a miss at depth 0
    break                                                                             on a later miss
    imageScratch = color                                                              frameID == 0
    imageScratch = (float(frameID) * imageScratch + color) / float(frameID + 1)       otherwise

(a depth-0 miss traces the unchanged ray once more, misses again and breaks: the colour is the miss colour either way.)
test_shade_cpu.py pins it to the CPU oracle's own frames before test_gpu_shade.py drives it with the public GPU calls.
"""
import os

import numpy as np

import golden_cases as gc
import oracle_bind as ob

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SHADE_KEY_DTYPE = np.dtype([("frameID", "<u4"), ("pixel", "<u4"), ("depth", "<u4"), ("_0", "<u4")])           # rdx_shade_key
SHADE_DTYPE = np.dtype([("color", "<f4", 3), ("hit", "<u4"), ("colorOccluded", "<f4", 3), ("materialIndex", "<u4"),
                        ("nextFactor", "<f4", 3), ("slot", "<u4")])                                                 # rdx_shade
NO_SLOT = 0xffffffff
ENVIRONMENT = np.array([0.2, 0.2, 0.5], F)          # the miss shader `environment` (shader.cl:543-549)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def keys_of(frames, pixels, depths):
    k = np.zeros(np.asarray(pixels).shape[0], SHADE_KEY_DTYPE)
    k["frameID"], k["pixel"], k["depth"] = frames, pixels, depths
    return k


# ---- the raygen loop ------------------------------------------------------------------------------------------------------------------
def compose_frames(npix, total_samples, batch_size, max_depth, nframes, generate, bounce):
    """-> [imageScratch (npix, 4) float32 after each of `nframes` TraceRays calls], starting from a cleared imageScratch and
    RTProp.totalSamples = total_samples, the host adding batch_size after every call (samples/sample1.cpp:447-498).
    generate(pixels uint32 (n,), randInput uint32 (n, 3)) -> (origins, directions) float32 (n, 3)
    bounce(origins, directions, frameID, pixels, depth) -> (hit bool (n,), color, nextFactor, nextOrigin, nextDirection float32
    (n, 3)): payload.color is the shader's colour AFTER its shadow test, the miss colour where hit is False"""
    px = np.arange(npix, dtype=np.uint32)
    scratch = np.zeros((npix, 4), F)
    out = []
    total = int(total_samples)
    for _ in range(nframes):
        for it in range(int(batch_size)):
            frame = total + it
            rnd = np.stack([np.full(npix, frame, np.uint32), np.full(npix, total, np.uint32), px], 1)       # shader.cl:205
            o, d = generate(px, rnd)
            o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
            color = np.zeros((npix, 3), F)
            contribution = np.ones((npix, 3), F)
            alive = px.astype(np.int64)             # pixels whose path is still being traced; o, d are theirs
            for depth in range(int(max_depth)):
                if not alive.size:
                    break
                hit, pc, nf, no, nd = bounce(o, d, frame, alive.astype(np.uint32), depth)
                hit = np.asarray(hit, bool)
                pc, nf = np.ascontiguousarray(pc, F), np.ascontiguousarray(nf, F)
                h = alive[hit]
                color[h] = color[h] + contribution[h] * pc[hit]
                contribution[h] = contribution[h] * nf[hit]
                if depth == 0:
                    color[alive[~hit]] = pc[~hit]
                alive = h
                o, d = np.ascontiguousarray(no, F)[hit], np.ascontiguousarray(nd, F)[hit]
            if frame == 0:
                scratch[:, :3] = color
            else:
                scratch[:, :3] = (F(frame) * scratch[:, :3] + color) / F(frame + 1)
            assert scratch.dtype == F
        total += int(batch_size)
        out.append(scratch.copy())
    return out


def oracle_callables(osc, blob):
    """(generate, bounce) of compose_frames over the CPU oracle's seams: ob.trace_batch for the closest walk, OracleScene.material_batch
    for the closest-hit shader -- which runs its shadow walk itself, as the reference's does (oracle/rt_oracle.c material) -- and
    OracleScene.generate_rays"""
    def bounce(o, d, frame, pixels, depth):
        n = o.shape[0]
        h = ob.trace_batch(blob, o, d)
        hit = h["hit"] == 1
        pay = osc.material_batch(h[hit], d[hit], pixels[hit], np.full(int(hit.sum()), frame, np.uint32), np.full(int(hit.sum()), depth, np.int32))
        pc = np.tile(ENVIRONMENT, (n, 1))
        nf, no, nd = np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros((n, 3), F)
        pc[hit], nf[hit], no[hit], nd[hit] = pay["color"], pay["nextFactor"], pay["nextRayOrigin"], pay["nextRayDirection"]
        return hit, pc, nf, no, nd
    return osc.generate_rays, bounce


def upload(rd, plt, arr, slack=0):
    arr = np.ascontiguousarray(arr)
    buf = rd.CreateBuffer(plt, max(arr.nbytes + slack, 16))
    rd.WriteBuffer(plt, buf, arr.nbytes, arr)
    return buf


def read(rd, plt, buf, n, dtype):
    if buf is None or n == 0:
        return np.zeros(0, dtype)
    return rd.ReadBuffer(plt, buf, n * dtype.itemsize).view(dtype).reshape(-1).copy()


def rays_of(rd, o, d, tmin=0.001, tmax=1000.0):
    rays = np.zeros(np.asarray(o).shape[0], rd.RAY_DTYPE)
    rays["origin"], rays["direction"], rays["tmin"], rays["tmax"] = o, d, tmin, tmax
    return rays


def chosen_color(shade, occluded):
    """payload.color of every shade record: colorOccluded where the ray's shadow ray hit something, else color"""
    return np.where(np.asarray(occluded, bool)[:, None], shade["colorOccluded"], shade["color"]).astype(F)


def shade_batch(rd, plt, tlas, sb, rays, keys, compact=False, hits=None, want_next=True):
    """QueryRays (closest) -> ShadeHits -> QueryRays (any) on the shadow rays, all on device buffers -> dict: q (query records),
    shade, next, shadow (records 0 .. live - 1 when compacting, else n), src, live, invalid, occluded (per INPUT ray: its shadow
    ray hit).  hits: records to shade instead of the query's"""
    n = rays.shape[0]
    bR, bK = upload(rd, plt, rays), upload(rd, plt, keys)
    bH = rd.QueryRays(tlas, bR, n, rd.QUERY_CLOSEST) if hits is None else upload(rd, plt, hits)
    bS, bN, bSh, bSrc, live, invalid = rd.ShadeHits(tlas, bR, bH, bK, n, sb, next=True if want_next else None, compact=compact)
    m = live if compact else n
    shade = read(rd, plt, bS, n, rd.SHADE_DTYPE)
    shadow = read(rd, plt, bSh, m, rd.RAY_DTYPE)
    occluded = np.zeros(n, bool)
    if m:
        sh = read(rd, plt, rd.QueryRays(tlas, bSh, m, rd.QUERY_ANY), m, rd.RAY_HIT_DTYPE)["hit"] == 1
        ok = shade["slot"] != NO_SLOT
        occluded[ok] = sh[shade["slot"][ok]]
    return dict(q=read(rd, plt, bH, n, rd.RAY_HIT_DTYPE), shade=shade, next=read(rd, plt, bN, m, rd.RAY_DTYPE) if want_next else None,
                shadow=shadow, src=read(rd, plt, bSrc, live, np.dtype("<u4")) if compact else None, live=live, invalid=invalid, occluded=occluded)


def gpu_callables(rd, dev, sb=None):
    """(generate, bounce) of compose_frames over the public calls: rd.GenerateBatch, rd.QueryRays, rd.ShadeHits with compaction on"""
    plt, tlas = dev.plt, dev.topAccelStruct
    sb = sb or dev.shading_buffers()

    def bounce(o, d, frame, pixels, depth):
        n = o.shape[0]
        r = shade_batch(rd, plt, tlas, sb, rays_of(rd, o, d), keys_of(frame, pixels, depth), compact=True)
        assert r["invalid"] == 0
        s = r["shade"]
        hit = s["hit"] == 1
        assert int(hit.sum()) == r["live"]
        no, nd = np.zeros((n, 3), F), np.zeros((n, 3), F)
        no[hit], nd[hit] = r["next"]["origin"][s["slot"][hit]], r["next"]["direction"][s["slot"][hit]]
        return hit, chosen_color(s, r["occluded"]), s["nextFactor"], no, nd
    return rd.GenerateBatch, bounce


class Golden:
    """one golden scene (tests/golden/refgpu_<name>.npz) on the device: the 2048 primary rays the reference's `material` was recorded on"""

    def __init__(self, rd, scenes, name):
        self.name = name
        self.G = np.load(os.path.join(GOLD, "refgpu_%s.npz" % name))
        self.s = gc.small_scene(scenes, name)
        self.b = self.s.buffers()
        self.dev = scenes.DeviceScene(self.s)
        blob = rd.ReadBuffer(self.dev.plt, self.dev.topAccelStruct, self.dev.topAccelStruct.size).tobytes()
        assert np.array_equal(gc.sha(blob), self.G["blob_sha256"]), "the TLAS blob of %s changed" % name
        sel = gc.spread(self.s.width * self.s.height, gc.N_MATERIAL)
        self.mat_rays = rays_of(rd, self.G["gen_o"][sel], self.G["gen_d"][sel])
        self.mat_hits = np.ascontiguousarray(self.G["mat_hits"]).view(ob.HIT_DTYPE).reshape(-1)
        self.mat_pay = np.ascontiguousarray(self.G["mat_payload"]).view(ob.PAYLOAD_DTYPE).reshape(-1)
        n = self.mat_rays.shape[0]
        frames, depths = gc.material_inputs(n)
        self.keys = keys_of(frames, np.arange(n, dtype=np.uint32), depths)


def recorded_branches(scene, hits, pay):
    """(lit, occluded) counts of recorded `material` payloads whose branch shows in the colour: occluded = payload.color has the
    bits of the ambient term alone, 0 + albedo * 0.1f (shader.cl:510-521; materialIndex is the instance's customInstanceID in these
    scenes), on a surface that faces the light -- where N.L <= 0 the direct term is 0 and both branches give the ambient term, so
    such hits count for neither.  N is the face normal of surface_cases.restate (these scenes have no normal maps)."""
    import surface_cases as sc
    k = hits["hit"] == 1
    albedo = np.array(scene.materials)["albedo"][hits["instanceCustomIndex"][k], :3]
    ambient = (np.zeros(3, F) + (albedo * F(0.1)).astype(F)).astype(F)
    ld = -np.array(scene.sceneProps).reshape(1)["lights"][0, 0]["direction"][:3].astype(np.float64)
    facing = sc.restate(hits[k], scene.buffers())["n64"] @ (ld / np.linalg.norm(ld)) > 1e-3
    is_ambient = (bits(pay["color"][k]) == bits(ambient)).all(1)
    return int((facing & ~is_ambient).sum()), int((facing & is_ambient).sum())


def check_against_payloads(r, hits, pay, tag="", compare=None, leave_out=None):
    """test 1 of the issue: on every recorded hit, `hit`, the chosen colour, nextFactor and the next ray equal the recorded payload
    bit for bit; misses carry the environment record.  -> (lit, occluded) counts among the hits whose two colours differ (where the
    direct term is 0 the branch does not show).  compare(got, want) -> (equal per row, ...): another rule than equal bits
    (shade_edge_cases.compare: a NaN of the recording wants a NaN); leave_out: bool per ray, rows whose colour and nextFactor are
    not compared (shade_edge_cases.zero_normal_rows)"""
    s, k = r["shade"], hits["hit"] == 1
    assert np.array_equal(s["hit"], hits["hit"].astype(np.uint32)), tag
    assert np.array_equal(s["hit"][k], pay["hit"][k]), tag
    slot = s["slot"][k]
    assert (slot != NO_SLOT).all() and (s["slot"][~k] == NO_SLOT).all(), tag
    col = chosen_color(s, r["occluded"])
    for name, got, want in (("color", col[k], pay["color"][k]), ("nextFactor", s["nextFactor"][k], pay["nextFactor"][k]),
                            ("nextRayOrigin", r["next"]["origin"][slot], pay["nextRayOrigin"][k]),
                            ("nextRayDirection", r["next"]["direction"][slot], pay["nextRayDirection"][k])):
        same = (bits(got) == bits(want)).all(1) if compare is None else compare(got, want)[0]
        if leave_out is not None and name in ("color", "nextFactor"):
            same = same | np.asarray(leave_out, bool)[k]
        assert same.all(), "%s: %s differs on %d of %d hits (first: hit row %d, got %r, want %r)" % (
            tag, name, int((~same).sum()), same.shape[0], int(np.flatnonzero(~same)[0]), got[~same][0].tolist(), want[~same][0].tolist())
    assert (bits(r["next"]["tmin"][slot]) == bits(F(0.001))).all() and (bits(r["next"]["tmax"][slot]) == bits(F(1000.0))).all(), tag
    check_misses(s, ~k, tag)
    shows = (bits(s["color"]) != bits(s["colorOccluded"])).any(1) & k
    return int((shows & ~r["occluded"]).sum()), int((shows & r["occluded"]).sum())


def check_misses(shade, miss, tag=""):
    m = shade[miss]
    assert (bits(m["color"]) == bits(ENVIRONMENT)).all() and (bits(m["colorOccluded"]) == bits(ENVIRONMENT)).all(), "%s: miss colour" % tag
    assert not m["hit"].any() and not m["materialIndex"].any() and not bits(m["nextFactor"]).any() and (m["slot"] == NO_SLOT).all(), tag


# ---- the bounds rule (rdx_debug_shade_in_bounds) ---------------------------------------------------------------------------------
MESH_INFO_DTYPE = np.dtype([("vertexOffset", "<i4"), ("indexOffset", "<i4"), ("uvOffset", "<i4"), ("normalOffset", "<i4"),
                            ("materialIndex", "<i4"), ("_0", "<i4"), ("_1", "<i4"), ("_2", "<i4")])
MATERIAL_DTYPE = np.dtype([("albedo", "<f4", 4), ("metallic", "<f4"), ("roughness", "<f4"), ("transmission", "<f4"), ("ior", "<f4"),
                           ("albedoTexIdx", "<i4"), ("metallicTexIdx", "<i4"), ("roughnessTexIdx", "<i4"), ("normalTexIdx", "<i4")])
LAYERS = 3


def bounds_scene():
    """surface_cases.bounds_scene (two meshes over 30 indices, 24 normal floats, 24 uv floats) with materialIndex 0 / 1 and two
    Material records without textures"""
    mi = np.zeros(2, MESH_INFO_DTYPE)
    mi[1]["indexOffset"], mi[1]["normalOffset"], mi[1]["uvOffset"], mi[1]["vertexOffset"], mi[1]["materialIndex"] = 18, 12, 12, 12, 1
    mt = np.zeros(2, MATERIAL_DTYPE)
    for f in ("albedoTexIdx", "metallicTexIdx", "roughnessTexIdx", "normalTexIdx"):
        mt[f] = -1
    return mi, mt, 30, 24, 24


def _mesh(field, value, k=1):
    mi = bounds_scene()[0]
    mi[k][field] = value
    return mi


def _mat(field, value, k=1):
    mt = bounds_scene()[1]
    mt[k][field] = value
    return mt


def bounds_table():
    """[(what, kwargs of bounds_answer, wanted answer)]"""
    T = [
        ("a valid triangle, textures off", dict(inst=1, prim=3, idx3=(1, 2, 3)), True),
        ("a valid triangle, textures on", dict(inst=1, prim=3, idx3=(1, 2, 3), textures=True), True),
        ("negative indexOffset", dict(inst=1, prim=0, idx3=(0, 0, 0), mi=_mesh("indexOffset", -1)), False),
        ("negative indexOffset, before the indices are read", dict(inst=1, prim=0, idx3=None, mi=_mesh("indexOffset", -1)), False),
        ("negative normalOffset", dict(inst=1, prim=0, idx3=(0, 1, 2), mi=_mesh("normalOffset", -1)), False),
        ("negative uvOffset, textures on", dict(inst=1, prim=0, idx3=(0, 1, 2), mi=_mesh("uvOffset", -1), textures=True), False),
        ("negative uvOffset, textures off: the uv stream is not read", dict(inst=1, prim=0, idx3=(0, 1, 2), mi=_mesh("uvOffset", -1)), True),
        ("primitiveIndex 0x55555556 (3 * it wraps to 2)", dict(inst=0, prim=0x55555556, idx3=(0, 1, 2)), False),
        ("primitiveIndex 0x55555556, before the indices are read", dict(inst=0, prim=0x55555556, idx3=None), False),
        ("primitiveIndex 0xffffffff (3 * it wraps to 0xfffffffd)", dict(inst=0, prim=0xffffffff, idx3=(0, 1, 2)), False),
        ("primitiveIndex 0x55555555 in a stream large enough for 64-bit positions: 3 * it + 2 wraps", dict(inst=0, prim=0x55555555, idx3=None, nindex=2 ** 33), False),
        ("primitiveIndex 0x55555554 in that stream: the last whose positions fit 32 bits", dict(inst=0, prim=0x55555554, idx3=None, nindex=2 ** 33), True),
        ("vertex 0x55555556 (3 * it wraps to 2)", dict(inst=0, prim=0, idx3=(0, 1, 0x55555556)), False),
        ("vertex 0x55555555 in a stream large enough", dict(inst=0, prim=0, idx3=(0, 1, 0x55555555), nnormal=2 ** 33), False),
        ("materialIndex == nmaterials", dict(inst=1, prim=0, idx3=(0, 1, 2), mi=_mesh("materialIndex", 2)), False),
        ("materialIndex == nmaterials - 1", dict(inst=1, prim=0, idx3=(0, 1, 2), mi=_mesh("materialIndex", 1)), True),
        ("materialIndex -1", dict(inst=1, prim=0, idx3=(0, 1, 2), mi=_mesh("materialIndex", -1)), False),
        ("materialIndex past the table, before the indices are read: the rule ends earlier", dict(inst=1, prim=0, idx3=None, mi=_mesh("materialIndex", 2)), True),
        ("materialIndex below a shorter table's end", dict(inst=1, prim=0, idx3=(0, 1, 2), nmaterials=1), False),
        ("no Material records at all", dict(inst=0, prim=0, idx3=(0, 1, 2), nmaterials=0), False),
    ]
    for f in ("albedoTexIdx", "metallicTexIdx", "roughnessTexIdx", "normalTexIdx"):
        T += [
            ("%s -1, textures on" % f, dict(inst=1, prim=0, idx3=(0, 1, 2), mt=_mat(f, -1), textures=True), True),
            ("%s layers - 1, textures on" % f, dict(inst=1, prim=0, idx3=(0, 1, 2), mt=_mat(f, LAYERS - 1), textures=True), True),
            ("%s == layers, textures on" % f, dict(inst=1, prim=0, idx3=(0, 1, 2), mt=_mat(f, LAYERS), textures=True), False),
            ("%s == layers, textures off: no texel is read" % f, dict(inst=1, prim=0, idx3=(0, 1, 2), mt=_mat(f, LAYERS)), True),
            ("%s -2, textures on" % f, dict(inst=1, prim=0, idx3=(0, 1, 2), mt=_mat(f, -2), textures=True), False),
            ("%s == layers in ANOTHER instance's material" % f, dict(inst=0, prim=0, idx3=(0, 1, 2), mt=_mat(f, LAYERS), textures=True), True),
        ]
    return T


def bounds_answer(rd, kw):
    mi, mt, nidx, nn, nuv = bounds_scene()
    return rd.DebugShadeInBounds(kw.get("mi", mi), kw.get("ninst", 2), kw["inst"], kw["prim"], kw["idx3"], kw.get("nindex", nidx),
                                 kw.get("nnormal", nn), kw.get("nuv", nuv), kw.get("mt", mt), textures=kw.get("textures", False),
                                 layers=LAYERS, nmaterials=kw.get("nmaterials"))

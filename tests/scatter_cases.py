"""Shared pieces of the scatter tests (test_scatter_cpu.py, test_gpu_scatter.py): rd.ScatterHits / rd.ScatterHitsTorch
(rdx_scatter_hits) -- the next-direction sample of the stock closest-hit shader `material` on the records of rd.ResolveMaterials
and rd.ResolveHits.

The comparands are rd.ShadeHits (rdx_shade_hits; tests/test_gpu_shade.py holds it to the reference's recorded payloads) and the
recordings themselves: bytes 32 .. 47 of a shade record are (nextFactor | slot), which is a scatter record, and ShadeHits' `next`
records are ScatterHits'.  Every bar is equality of bits.

The identities are stated for hits whose SBT row is `material`, that is instanceSBTOffset 0: a material record says nothing about
the row.  All fixture scenes are such.
"""
import numpy as np

import material_cases as mc
import shade_cases as sh

F = np.float32
SCATTER_DTYPE = np.dtype([("nextFactor", "<f4", 3), ("slot", "<u4")])          # rdx_scatter
RANDOMS_DTYPE = np.dtype([("xyz", "<f4", 3), ("w", "<f4")])
NO_SLOT = sh.NO_SLOT
bits, same = sh.bits, mc.same


def randoms_of(xyz, w=0.0):
    r = np.zeros(np.asarray(xyz).shape[0], RANDOMS_DTYPE)
    r["xyz"], r["w"] = xyz, w
    return r


def key_randoms(rd, keys, w=0.0):
    """pcg3d(frameID, pixel, depth) of SHADE_KEY_DTYPE records, padded to float4: the randoms route's equivalent of the keys"""
    return randoms_of(rd.Pcg3dBatch(np.stack([keys["frameID"], keys["pixel"], keys["depth"]], 1)), w)


def records(rd, dev, rays, hits=None):
    """QueryRays (closest) -> ResolveHits + ResolveMaterials, on device buffers -> dict: q, surf, mat, and the buffers bR, bH, bS, bM"""
    plt, tlas = dev.plt, dev.topAccelStruct
    n = rays.shape[0]
    bR = sh.upload(rd, plt, rays)
    bH = rd.QueryRays(tlas, bR, n, rd.QUERY_CLOSEST) if hits is None else sh.upload(rd, plt, hits)
    bS, inv_s = rd.ResolveHits(tlas, bR, bH, n, dev.surface_buffers())
    bM, inv_m = rd.ResolveMaterials(tlas, bR, bH, n, dev.shading_buffers())
    assert inv_s == 0 and inv_m == 0
    return dict(q=sh.read(rd, plt, bH, n, rd.RAY_HIT_DTYPE), surf=sh.read(rd, plt, bS, n, rd.SURFACE_DTYPE),
                mat=sh.read(rd, plt, bM, n, mc.MATERIAL_RECORD_DTYPE), bR=bR, bH=bH, bS=bS, bM=bM, n=n)


def scatter(rd, plt, rec, keys=None, randoms=None, compact=False, n=None, first=0):
    """rd.ScatterHits on the records of `records` (rows first .. first + n through the offsets) -> dict: scatter (n), next (live
    records when compacting, else n), src (live; None when not compacting), live"""
    n = rec["n"] - first if n is None else n
    bK = sh.upload(rd, plt, keys) if keys is not None else None
    bU = sh.upload(rd, plt, randoms) if randoms is not None else None
    bO, bN, bSrc, live = rd.ScatterHits(rec["bR"], rec["bM"], rec["bS"], bK, n, randoms=bU, compact=compact, rays_offset=32 * first,
                                        materials_offset=64 * first, surfaces_offset=64 * first)
    assert (bSrc is not None) == compact
    m = live if compact else n
    return dict(scatter=sh.read(rd, plt, bO, n, SCATTER_DTYPE), next=sh.read(rd, plt, bN, m, rd.RAY_DTYPE),
                src=sh.read(rd, plt, bSrc, live, np.dtype("<u4")) if compact else None, live=live)


def shade_scatter(shade):
    """bytes 32 .. 47 of every SHADE_DTYPE record, as SCATTER_DTYPE"""
    return np.ascontiguousarray(np.ascontiguousarray(shade).view(np.uint8).reshape(-1, 48)[:, 32:48]).view(SCATTER_DTYPE).reshape(-1)


def check_src(src, hit, tag=""):
    """the compaction rule: src is a permutation of the rows with hit, in which the survivors of every block of 64 consecutive
    inputs are contiguous and ascending"""
    rows = np.flatnonzero(hit)
    assert src.shape[0] == rows.shape[0] and np.array_equal(np.sort(src), rows), tag
    block = src // 64
    change = np.flatnonzero(np.diff(block) != 0)
    assert np.unique(block[np.r_[0, change + 1]]).shape[0] == change.shape[0] + 1 if src.size else True, "%s: a block of 64 is split" % tag
    inside = np.diff(block) == 0
    assert (np.diff(src.astype(np.int64))[inside] > 0).all(), "%s: a block's survivors are out of input order" % tag


def check_compacted(got, full, hit, tag=""):
    """a compacting run `got` against the not compacting run `full` of the same records (dicts of `scatter`)"""
    assert got["live"] == int(hit.sum()) == full["live"], tag
    check_src(got["src"], hit, tag)
    slot = got["scatter"]["slot"]
    assert (slot[~hit] == NO_SLOT).all() and np.array_equal(got["src"][slot[hit]], np.flatnonzero(hit)), tag
    assert same(got["scatter"]["nextFactor"], full["scatter"]["nextFactor"]), tag
    assert same(got["next"][slot[hit]], full["next"][hit]), "%s: next rays" % tag


# ---- frames: compose_frames without a ShadeHits call ---------------------------------------------------------------------------------
def gpu_callables(rd, dev, calls=None):
    """(generate, bounce) of sh.compose_frames: the colour of a hit from ResolveMaterials + LightHits(0) + an any-hit query of the
    shadow records + the ambient term (material_cases.material_batch), hit / nextFactor / next ray from ScatterHits, compacting;
    a miss has the miss colour.  rd.ShadeHits is not called"""
    plt, tlas, sb = dev.plt, dev.topAccelStruct, dev.shading_buffers()

    def bounce(o, d, frame, pixels, depth):
        n = o.shape[0]
        m = mc.material_batch(rd, plt, tlas, sb, sh.rays_of(rd, o, d))
        bS, invalid = rd.ResolveHits(tlas, m["bR"], m["bH"], n, dev.surface_buffers())
        assert invalid == 0 and m["invalid"] == 0
        r = scatter(rd, plt, dict(bR=m["bR"], bM=m["bM"], bS=bS, n=n), keys=sh.keys_of(frame, pixels, depth), compact=True)
        hit = m["mat"]["hit"] == 1
        assert r["live"] == int(hit.sum()) and np.array_equal(r["src"][r["scatter"]["slot"][hit]], np.flatnonzero(hit))
        albedo = m["mat"]["albedo"]
        pc = np.where(m["occluded"][:, None], mc.color_occluded(albedo), mc.color_lit(m["lit"]["rgb"], albedo)).astype(F)
        pc[~hit] = sh.ENVIRONMENT
        no, nd = np.zeros((n, 3), F), np.zeros((n, 3), F)
        no[hit], nd[hit] = r["next"]["origin"][r["scatter"]["slot"][hit]], r["next"]["direction"][r["scatter"]["slot"][hit]]
        if calls is not None:
            calls.append(n)
        return hit, pc, r["scatter"]["nextFactor"], no, nd
    return rd.GenerateBatch, bounce


# ---- the README's path tracer over several lights, on buffers, folded in numpy float32 ------------------------------------------------
def path_tracer_numpy(rd, dev, scene, light_count, rays, frames, pixels, max_depth):
    """the second Quick-start loop of the README with every call on device buffers and the folding in numpy, one float32 operation
    at a time -> (color (n, 3), weight (n, 3), live rays per bounce)"""
    plt, tlas = dev.plt, dev.topAccelStruct
    n = rays.shape[0]
    color, weight = np.zeros((n, 3), F), np.ones((n, 3), F)
    path = np.arange(n)
    frames, pixels = np.asarray(frames, np.uint32), np.asarray(pixels, np.uint32)
    lives = []
    for depth in range(max_depth):
        m = rays.shape[0]
        rec = records(rd, dev, rays)
        hit = rec["mat"]["hit"] == 1
        if depth == 0:
            color[path[~hit]] = sh.ENVIRONMENT
        direct = np.zeros((m, 3), F)
        for j in range(light_count):
            w = mc.light_batch(rd, plt, tlas, rec["bR"], rec["bM"], m, scene, j)
            direct = (direct + np.where(w["occluded"][:, None], F(0), w["lit"]["rgb"])).astype(F)
        radiance = (direct + mc.ambient(rec["mat"]["albedo"])).astype(F)
        r = scatter(rd, plt, rec, keys=sh.keys_of(frames, pixels, depth), compact=True)
        src = r["src"].astype(np.int64)
        color[path[src]] = (color[path[src]] + (weight[path[src]] * radiance[src]).astype(F)).astype(F)
        weight[path[src]] = (weight[path[src]] * r["scatter"]["nextFactor"][src]).astype(F)
        path, frames, pixels, rays = path[src], frames[src], pixels[src], r["next"]
        lives.append(r["live"])
        if r["live"] == 0:
            break
    return color, weight, lives

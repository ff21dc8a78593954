"""Shared pieces of the tests of rd.TracePaths / rdx_trace_paths (test_paths_cpu.py, test_gpu_paths.py): radiance along the
caller's own rays.

fold is the numpy float32 restatement of what the call does with the closest-hit shader's answers, one operation at a time under
the contract of DESIGN.md section 2 (samples/shader.cl:231-260; the loop of the README with a frameID per path):

    color += contribution * payload.color; contribution *= payload.nextFactor         on a hit
    color = payload.color                                                             on a miss at depth 0
    the path ends                                                                     on a later miss, or after max_depth segments

around one callable, `bounce`, which answers for the live rays of one depth with rd.ShadeHits' records.  test_paths_cpu.py checks it
on hand-made records; public_loop drives it with rd.QueryRays / rd.ShadeHits, and that is what rd.TracePaths is held to.
"""
import numpy as np

import shade_cases as sh

F = np.float32
U4 = np.dtype("<u4")


def fold(n, max_depth, bounce):
    """-> (radiance (n, 4) float32: rgb, 0; counts: live rays entering each depth traced, then the survivors of the last one).
    bounce(depth, path) answers for the live rays, ray k being the current segment of path number path[k]:
    -> (shade: SHADE_DTYPE records, one per live ray; occluded: bool per live ray, its shadow ray hit something; src: for next ray j
    the number k of the live ray it continues, the survivors in any order)"""
    color = np.zeros((n, 3), F)
    contribution = np.ones((n, 3), F)
    path = np.arange(n, dtype=np.int64)
    counts = []
    for depth in range(int(max_depth)):
        if not path.size:
            break
        counts.append(int(path.size))
        shade, occluded, src = bounce(depth, path)
        hit = shade["hit"] == 1
        src = np.asarray(src, np.int64)
        assert shade.shape[0] == path.size and src.shape[0] == int(hit.sum()) and hit[src].all() and np.unique(src).size == src.size
        pc = sh.chosen_color(shade, occluded)
        h = path[hit]
        color[h] = color[h] + contribution[h] * pc[hit]
        contribution[h] = contribution[h] * np.ascontiguousarray(shade["nextFactor"], F)[hit]
        if depth == 0:
            color[path[~hit]] = pc[~hit]
        path = path[src]
    if max_depth:
        counts.append(int(path.size))
    out = np.zeros((n, 4), F)
    out[:, :3] = color
    assert color.dtype == F and contribution.dtype == F
    return out, counts


def public_loop(rd, plt, tlas, sb, rays, keys, max_depth):
    """the loop over the public calls for rays (RAY_DTYPE) and keys (SHADE_KEY_DTYPE: frameID and pixel are used) of the caller's
    own: per depth QueryRays (closest) -> ShadeHits, compacting, the next direction not sampled at the last depth (next = None) ->
    QueryRays (any) on the shadow rays -> fold.  The first segment is traced with each ray's own interval, every later one with
    the 0.001 / 1000 ShadeHits writes.  -> (radiance (n, 4), counts, first-segment records RAY_HIT_DTYPE)"""
    n = rays.shape[0]
    state = dict(rays=sh.upload(rd, plt, rays), first=None)

    def bounce(depth, path):
        m = path.size
        k = sh.upload(rd, plt, sh.keys_of(keys["frameID"][path], keys["pixel"][path], depth))
        hits = rd.QueryRays(tlas, state["rays"], m, rd.QUERY_CLOSEST)
        if depth == 0:
            state["first"] = sh.read(rd, plt, hits, m, rd.RAY_HIT_DTYPE)
        last = depth + 1 == max_depth
        bS, bN, bSh, bSrc, live, invalid = rd.ShadeHits(tlas, state["rays"], hits, k, m, sb, next=None if last else True, compact=True)
        assert invalid == 0
        s = sh.read(rd, plt, bS, m, rd.SHADE_DTYPE)
        hit = s["hit"] == 1
        assert int(hit.sum()) == live
        occluded = np.zeros(m, bool)
        if live:
            shadowed = sh.read(rd, plt, rd.QueryRays(tlas, bSh, live, rd.QUERY_ANY), live, rd.RAY_HIT_DTYPE)["hit"] == 1
            occluded[hit] = shadowed[s["slot"][hit]]
        state["rays"] = bN
        return s, occluded, sh.read(rd, plt, bSrc, live, U4)
    radiance, counts = fold(n, max_depth, bounce)
    if state["first"] is None:
        state["first"] = sh.read(rd, plt, rd.QueryRays(tlas, state["rays"], n, rd.QUERY_CLOSEST), n, rd.RAY_HIT_DTYPE)
    return radiance, counts, state["first"]


def trace_paths(rd, plt, tlas, sb, rays, keys, max_depth, want_hits=True):
    """rd.TracePaths on uploaded copies of rays / keys -> (radiance (n, 4) float32, first-segment records or None)"""
    n = rays.shape[0]
    out = rd.TracePaths(tlas, sh.upload(rd, plt, rays), sh.upload(rd, plt, keys), n, max_depth, sb, hits=True if want_hits else None)
    bR, bH = out if want_hits else (out, None)
    rad = rd.ReadBuffer(plt, bR, 16 * n).view(F).reshape(n, 4).copy() if n else np.zeros((0, 4), F)
    return rad, (sh.read(rd, plt, bH, n, rd.RAY_HIT_DTYPE) if want_hits else None)


# ---- the batch of the issue's test 2 --------------------------------------------------------------------------------------------
N_BATCH = 1000 + 37         # four blocks, the last one partial and ending in a partial wave
KINDS = ("stock", "tmax before the first hit", "tmin beyond the first hit", "NaN bound", "tmax 0")


def arbitrary_batch(rd, lo, hi, first_t, seed, n=N_BATCH):
    """n rays against a scene whose box is lo .. hi: origins inside and outside it, directions of any length (towards a point of the
    box; every eighth axis-aligned with two zero components), keys with a frameID per ray (0 and 0xffffffff among them), arbitrary
    and repeated pixels, junk in depth / _0.  first_t(rays) -> (hit, t) of the stock interval, from which the interval kinds are
    cut: -> (rays, keys, kind (n,) index into KINDS)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    o = (lo + ext * rng.uniform(0.05, 0.95, (n, 3)))
    outside = rng.uniform(size=n) < 0.35
    o[outside] = (lo + ext * rng.uniform(-0.6, 1.6, (n, 3)))[outside]
    target = lo + ext * rng.uniform(0.1, 0.9, (n, 3))
    d = (target - o) * rng.uniform(0.05, 4.0, (n, 1))
    axis = np.arange(n) % 8 == 3
    da = np.zeros((n, 3))
    da[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-2.5, 0.5, 1.0, 3.0], n)
    d[axis] = da[axis]
    rays = sh.rays_of(rd, o.astype(F), d.astype(F))
    hit, t = first_t(rays)
    kind = rng.choice(len(KINDS), n, p=[0.6, 0.1, 0.1, 0.1, 0.1])
    kind[~hit & ((kind == 1) | (kind == 2))] = 0            # these two need a first hit to be cut against
    t = t.astype(np.float64)
    rays["tmax"][kind == 1] = (t * 0.5).astype(F)[kind == 1]
    rays["tmin"][kind == 2] = (t * 1.5 + 0.01).astype(F)[kind == 2]
    nan = np.flatnonzero(kind == 3)
    rays["tmin"][nan[::2]] = np.nan
    rays["tmax"][nan[1::2]] = np.nan
    rays["tmax"][kind == 4] = 0.0
    keys = np.zeros(n, rd.SHADE_KEY_DTYPE)
    keys["frameID"] = rng.permutation(np.arange(1, 5 * n, dtype=np.uint64))[:n].astype(np.uint32) * np.uint32(2654435761)
    keys["frameID"][0], keys["frameID"][1] = 0, 0xffffffff
    assert np.unique(keys["frameID"]).size == n
    keys["pixel"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    keys["pixel"][n // 2:] = keys["pixel"][:n - n // 2]     # every pixel number twice
    keys["depth"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    keys["_0"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    return rays, keys, kind

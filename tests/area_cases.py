"""Shared pieces of the tests of rd.AreaLightHits / rd.TraceAreaPaths (rdx_area_light_hits, rdx_trace_paths_area): quad and triangle
area lights from a second caller-owned light table, sampled at one point per (hit, light) (test_area_cpu.py, test_gpu_area.py).

  pcg3d             device_math.h's pcg3d in numpy: uint32 arithmetic that wraps, then three float32 divisions by (float)0xffffffff;
                    test_area_cpu.py holds it to oracle_bind.pcg3d, the oracle's, bit for bit.
  randoms_of        the random records of the keys route, pcg3d(frame, pixel, depth + ((stream + 1) << 16)), as the float4 records
                    the randoms route takes: the two routes must agree bit for bit.
  emitted_area      what an area record emits at a point `above` for the random pair (u, v), restated from include/rdx.h in numpy
                    float32 one IEEE operation at a time (no contraction): the triangle fold, p, n, w, d2, g, E,
                    tmax and the dark rule.  Like punctual_cases.emitted it takes the unit vector L (towards p) as an INPUT:
                    normalize3 is built on v_rsq_f32, which the CPU does not reproduce.  The GPU tests pass in L as read from the
                    call's shadow records, so everything else of the record's arithmetic is held to numpy bit for bit, and the BRDF
                    to rd.LightHits (which tests/test_gpu_materials.py holds to the reference's recordings).
  public_loop_area  punctual_cases.public_loop_punctual with the area loop added: the comparand of rd.TraceAreaPaths.
"""
import numpy as np

import light_paths_cases as lp
import material_cases as mc
import punctual_cases as pu
import scatter_cases as sc
import shade_cases as sh

F = np.float32
U = np.uint32
QUAD, TRIANGLE = 0, 1


def pcg3d(x, y, z):
    """(n, 3) float32: csrc/device_math.h pcg3d of three uint32 arrays"""
    with np.errstate(over="ignore"):
        v = [np.atleast_1d(np.asarray(a)).astype(U) * U(1664525) + U(1013904223) for a in np.broadcast_arrays(x, y, z)]
        for _ in range(2):
            v[0] = v[0] + v[1] * v[2]
            v[1] = v[1] + v[2] * v[0]
            v[2] = v[2] + v[0] * v[1]
            if _ == 0:
                v = [a ^ (a >> U(16)) for a in v]
    return np.stack([(a.astype(F) / F(0xffffffff)).astype(F) for a in v], 1)


def stream_word(depth, stream):
    """the third input of pcg3d for (depth, stream), in uint32 arithmetic"""
    return (np.asarray(depth).astype(U) + ((np.asarray(stream).astype(U) + U(1)) << U(16))).astype(U)


def randoms_of(frames, pixels, depth, stream):
    """sc.RANDOMS_DTYPE records (n,): pcg3d(frame, pixel, depth + ((stream + 1) << 16)); the call reads x and y"""
    return sc.randoms_of(pcg3d(frames, pixels, stream_word(depth, stream)))


def table(rd, records):
    return np.array([np.array(r) for r in records], rd.AREA_LIGHT_DTYPE).reshape(-1)


def emitted_area(light, above, u, v, L):
    """light: one AREA_LIGHT_DTYPE record; above (n, 3); u, v (n,) or scalars: the random pair as the call reads it (before the
    triangle fold); L (n, 3) or (3,): the call's unit vector towards the sampled point
    -> dict: dark (n,) bool, E (n, 3), tmax (n,), d2 (n,), g (n,), p (n, 3), w (n, 3) = p - above, u, v (after the fold) -- every
    float32 operation rounded on its own, in the order of include/rdx.h.  E and tmax of dark rows are not meaningful."""
    above = np.ascontiguousarray(above, F).reshape(-1, 3)
    n = above.shape[0]
    u, v = np.broadcast_to(np.asarray(u, F), (n,)).copy(), np.broadcast_to(np.asarray(v, F), (n,)).copy()
    L = np.broadcast_to(np.ascontiguousarray(L, F).reshape(-1, 3), (n, 3))
    t, two_sided = int(light["type"]), bool(int(light["flags"]) & 1)
    c, eu, ev, rad = (np.ascontiguousarray(light[k], F) for k in ("corner", "edgeU", "edgeV", "radiance"))
    zero = np.zeros(n, F)
    if t > TRIANGLE:
        return dict(dark=np.ones(n, bool), E=np.zeros((n, 3), F), tmax=zero, d2=zero, g=zero, p=np.zeros((n, 3), F), w=np.zeros((n, 3), F), u=u, v=v)
    with np.errstate(all="ignore"):
        if t == TRIANGLE:
            fold = (u + v).astype(F) > F(1.0)
            u, v = np.where(fold, (F(1.0) - u).astype(F), u), np.where(fold, (F(1.0) - v).astype(F), v)
        p = np.stack([((c[k] + (eu[k] * u).astype(F)).astype(F) + (ev[k] * v).astype(F)).astype(F) for k in range(3)], 1)
        nrm = [F(F(eu[1] * ev[2]) - F(eu[2] * ev[1])), F(F(eu[2] * ev[0]) - F(eu[0] * ev[2])), F(F(eu[0] * ev[1]) - F(eu[1] * ev[0]))]
        w = (p - above).astype(F)
        xx, yy, zz = (w[:, 0] * w[:, 0]).astype(F), (w[:, 1] * w[:, 1]).astype(F), (w[:, 2] * w[:, 2]).astype(F)
        d2 = ((xx + yy).astype(F) + zz).astype(F)
        dark = ~(d2 > F(0.0))
        dark |= ~(d2 < F(np.inf))
        g = -((((nrm[0] * L[:, 0]).astype(F) + (nrm[1] * L[:, 1]).astype(F)).astype(F) + (nrm[2] * L[:, 2]).astype(F)).astype(F))
        if t == TRIANGLE:
            g = (g * F(0.5)).astype(F)
        if two_sided:
            g = np.abs(g)
        dark |= ~(g > F(0.0))
        s = (g / d2).astype(F)
        E = (rad[None, :] * s[:, None]).astype(F)
        tmax = (np.sqrt(d2).astype(F) * F(0.999)).astype(F)
    return dict(dark=dark, E=E, tmax=tmax, d2=d2, g=g.astype(F), p=p, w=w, u=u, v=v)


# ---- the calls, on device buffers --------------------------------------------------------------------------------------------------
def area_batch(rd, plt, tlas, bR, bM, n, bT, index, keys=None, randoms=None, stream=None, want_shadow=True, query=True, **offsets):
    """rd.AreaLightHits(record `index` of the table buffer bT; keys / randoms: numpy records, uploaded) -> QueryRays (any) on its
    shadow rays -> dict as punctual_cases.punctual_batch"""
    bK = sh.upload(rd, plt, keys) if keys is not None else None
    bU = sh.upload(rd, plt, randoms) if randoms is not None else None
    bL, bSh = rd.AreaLightHits(bR, bM, n, bT, index, keys=bK, randoms=bU, stream=stream, shadow=True if want_shadow else None, **offsets)
    occluded = np.zeros(n, bool)
    shadow = None
    if want_shadow:
        shadow = sh.read(rd, plt, bSh, n, rd.RAY_DTYPE)
        if n and query:
            occluded = sh.read(rd, plt, rd.QueryRays(tlas, bSh, n, rd.QUERY_ANY), n, rd.RAY_HIT_DTYPE)["hit"] == 1
    return dict(lit=sh.read(rd, plt, bL, n, mc.LIT_DTYPE), shadow=shadow, occluded=occluded, bL=bL, bSh=bSh)


is_dark = pu.is_dark


def trace(rd, plt, tlas, sb, rays, keys, max_depth, lights, area):
    """rd.TraceAreaPaths on uploaded copies of rays / keys / the two tables (an empty table is passed as None)
    -> (radiance (n, 4) float32, invalid)"""
    n, L, A = rays.shape[0], lights.shape[0], area.shape[0]
    bT = sh.upload(rd, plt, lights) if L else None
    bA = sh.upload(rd, plt, area) if A else None
    bR, invalid = rd.TraceAreaPaths(tlas, sh.upload(rd, plt, rays), sh.upload(rd, plt, keys), n, max_depth, bT, L, bA, A, sb)
    return (rd.ReadBuffer(plt, bR, 16 * n).view(F).reshape(n, 4).copy() if n else np.zeros((0, 4), F)), invalid


def public_loop_area(rd, plt, tlas, sb, surface_buffers, lights, area, rays, frames, pixels, max_depth):
    """punctual_cases.public_loop_punctual with, after record j of the punctual table `lights` through rd.PunctualLightHits, record j
    of the area table `area` through rd.AreaLightHits on the keys route (stream = j, the default) with the path's own (frame,
    pixel, depth); the shadow rays carry each call's tmax; the fold runs over the punctual records first
    -> (color (n, 3), live rays per bounce, invalid summed over the bounces, first-hit-invalid mask (n,), (dark, lit) rows among the
    depth-0 hits per record)"""
    n, L, A = rays.shape[0], lights.shape[0], area.shape[0]
    bT = sh.upload(rd, plt, lights if L else np.zeros(1, rd.PUNCTUAL_LIGHT_DTYPE))
    bA = sh.upload(rd, plt, area if A else np.zeros(1, rd.AREA_LIGHT_DTYPE))
    color, weight = np.zeros((n, 3), F), np.ones((n, 3), F)
    path = np.arange(n)
    frames, pixels = np.asarray(frames, np.uint32), np.asarray(pixels, np.uint32)
    lives, invalid, first_invalid, dark0 = [], 0, np.zeros(n, bool), []
    for depth in range(max_depth):
        m = rays.shape[0]
        bR = sh.upload(rd, plt, rays)
        bH = rd.QueryRays(tlas, bR, m, rd.QUERY_CLOSEST)
        bS, _ = rd.ResolveHits(tlas, bR, bH, m, surface_buffers)
        bM, inv = rd.ResolveMaterials(tlas, bR, bH, m, sb)
        invalid += inv
        mat = sh.read(rd, plt, bM, m, mc.MATERIAL_RECORD_DTYPE)
        hit = mat["hit"] == 1
        if depth == 0:
            color[path[~hit]] = sh.ENVIRONMENT
            first_invalid = (sh.read(rd, plt, bH, m, rd.RAY_HIT_DTYPE)["hit"] == 1) & ~hit
        keys = sh.keys_of(frames, pixels, depth)
        lit, occluded = np.zeros((m, L + A, 3), F), np.zeros((m, L + A), bool)
        for j in range(L + A):
            w = pu.punctual_batch(rd, plt, tlas, bR, bM, m, bT, j) if j < L else area_batch(rd, plt, tlas, bR, bM, m, bA, j - L, keys=keys)
            lit[:, j], occluded[:, j] = w["lit"]["rgb"], w["occluded"]
            if depth == 0:
                dark0.append((int((is_dark(w) & hit).sum()), int((~is_dark(w) & hit).sum())))
        r = sc.scatter(rd, plt, dict(bR=bR, bM=bM, bS=bS, n=m), keys=keys, compact=True)
        src = r["src"].astype(np.int64)
        p = path[src]
        color[p], weight[p] = lp.fold_lights(lit[src], occluded[src], mc.ambient(mat["albedo"][src]), r["scatter"]["nextFactor"][src], color[p], weight[p])
        path, frames, pixels, rays = p, frames[src], pixels[src], r["next"]
        lives.append(r["live"])
        if r["live"] == 0:
            break
    return color, lives, invalid, first_invalid, dark0


def scene_lights(rd, lo, hi):
    """the three emitters of the per-hit tests, placed from the scene box lo .. hi:
      ceiling  a one-sided quad, 0.3 of the box wide, 0.02 of its height under its top, facing down;
      inner    a two-sided, tilted triangle in the middle of the box: hit points see it from both sides;
      away     a one-sided upright quad three quarters of the way to the box's far end (+z) that faces that end: dark for the
               larger part of the scene, which lies behind it."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    at = lambda fx, fy, fz: lo + ext * np.array([fx, fy, fz])
    return dict(ceiling=rd.QuadLight(at(0.35, 0.98, 0.35), (0.3 * ext[0], 0, 0), (0, 0, 0.3 * ext[2]), (30.0, 28.0, 24.0)),
                inner=rd.TriangleLight(at(0.35, 0.45, 0.4), (0.3 * ext[0], 0.1 * ext[1], 0), (0, 0.1 * ext[1], 0.3 * ext[2]), (24.0, 30.0, 36.0), two_sided=True),
                away=rd.QuadLight(at(0.3, 0.3, 0.75), (0.4 * ext[0], 0, 0), (0, 0.4 * ext[1], 0), (40.0, 20.0, 30.0)))


def area_table(rd, lo, hi, seed):
    """MAX_PATH_LIGHTS area records inside the scene box lo .. hi: the quad that faces away first, the two-sided triangle second, the
    ceiling quad third, a record of an unknown type (2: dark everywhere) fourth, then quads and triangles, one- and two-sided, of
    random place and orientation: every prefix the tests take (1, 2, 16) holds a record that is dark for part of the scene"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    named = scene_lights(rd, lo, hi)
    out = [named["away"], named["inner"], named["ceiling"]]
    unknown = np.array(named["ceiling"]).copy()
    unknown["type"] = 2
    out.append(unknown)
    for k in range(rd.MAX_PATH_LIGHTS - len(out)):
        corner = lo + ext * rng.uniform(0.2, 0.8, 3)
        eu, ev = rng.normal(size=3), rng.normal(size=3)
        eu, ev = eu / np.linalg.norm(eu) * 0.15 * ext.min(), ev / np.linalg.norm(ev) * 0.15 * ext.min()
        make = rd.TriangleLight if k % 2 else rd.QuadLight
        out.append(make(corner, eu, ev, rng.uniform(10.0, 40.0, 3), two_sided=k % 3 == 0))
    return table(rd, out)


def in_emitter(light, u, v):
    """(u, v) after the fold lie in the record's parameter domain: the unit square, or its lower-left triangle (one ulp of slack on
    the sum, which the fold's own rounding can leave)"""
    ok = (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1)
    if int(light["type"]) == TRIANGLE:
        ok &= u.astype(np.float64) + v.astype(np.float64) <= 1.0 + 2.0 ** -23
    return ok

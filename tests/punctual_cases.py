"""Shared pieces of the tests of rd.PunctualLightHits / rd.TracePunctualPaths (rdx_punctual_light_hits, rdx_trace_paths_punctual):
point and spot lights from a caller-owned light table (test_punctual_cpu.py, test_gpu_punctual.py).

  emitted               what a table record emits at a point `above`, restated from include/rdx.h in numpy float32 one IEEE operation
                        at a time (no contraction): d2, att, E, f, tmax and the dark rule.  It takes the unit
                        vectors L (towards the light) and S (the spot's axis) as INPUTS: normalize3 is built on v_rsq_f32, which the
                        CPU does not reproduce.  The GPU tests pass in L as read from the call's shadow records and S from one
                        rd.LightHits call, so everything else of the record's arithmetic is held to numpy bit for bit, and the BRDF
                        to rd.LightHits (which tests/test_gpu_materials.py holds to the reference's recordings).
  public_loop_punctual  light_paths_cases.public_loop with the per-light call replaced by rd.PunctualLightHits: the comparand of
                        rd.TracePunctualPaths.
"""
import numpy as np

import light_paths_cases as lp
import material_cases as mc
import scatter_cases as sc
import shade_cases as sh

F = np.float32
DIRECTIONAL, POINT, SPOT = 0, 1, 2


def light(rd, type=POINT, position=(0, 0, 0), direction=(0, -1, 0), range=0.0, color=(1, 1, 1), cone=(0.0, 0.0)):
    """one rd.PUNCTUAL_LIGHT_DTYPE record; cone = (coneScale, coneOffset), e.g. rd.SpotCone(inner, outer)"""
    r = np.zeros((), rd.PUNCTUAL_LIGHT_DTYPE)
    r["type"], r["position"], r["direction"], r["range"], r["color"] = type, position, direction, range, color
    r["coneScale"], r["coneOffset"] = cone
    return r


def table(rd, records):
    return np.array([np.array(r) for r in records], rd.PUNCTUAL_LIGHT_DTYPE).reshape(-1)


def directional_table(rd, sp, count=lp.N_LIGHTS):
    """the first `count` DirLights of a SceneProperties as type-0 records"""
    sp = np.array(sp).reshape(1)[0]
    return table(rd, [light(rd, DIRECTIONAL, direction=sp["lights"][j]["direction"][:3], color=sp["lights"][j]["color"][:3]) for j in range(count)])


def emitted(light, above, L, S=None):
    """light: one PUNCTUAL_LIGHT_DTYPE record; above (n, 3); L (n, 3) or (3,): the call's unit vector towards the light; S (3,):
    normalize3(direction), spots only -> dict: dark (n,) bool, E (n, 3), tmax (n,), d2 (n,), f (n,) -- every float32 operation
    rounded on its own, in the order of include/rdx.h.  E and tmax of dark rows are not meaningful."""
    above = np.ascontiguousarray(above, F).reshape(-1, 3)
    n = above.shape[0]
    t = int(light["type"])
    color = np.ascontiguousarray(light["color"], F)
    one = np.ones(n, F)
    if t > SPOT:
        return dict(dark=np.ones(n, bool), E=np.zeros((n, 3), F), tmax=np.zeros(n, F), d2=np.zeros(n, F), f=one)
    if t == DIRECTIONAL:
        return dict(dark=np.zeros(n, bool), E=np.tile(color, (n, 1)), tmax=np.full(n, 1000.0, F), d2=np.zeros(n, F), f=one)
    with np.errstate(all="ignore"):
        v = (np.ascontiguousarray(light["position"], F)[None, :] - above).astype(F)
        xx, yy, zz = (v[:, 0] * v[:, 0]).astype(F), (v[:, 1] * v[:, 1]).astype(F), (v[:, 2] * v[:, 2]).astype(F)
        d2 = ((xx + yy).astype(F) + zz).astype(F)
        dark = ~(d2 > F(0.0))
        dark |= ~(d2 < F(np.inf))
        rng = F(light["range"])
        if rng > F(0.0):
            dark |= ~(d2 < F(rng * rng))
        att = (F(1.0) / d2).astype(F)
        E = (color[None, :] * att[:, None]).astype(F)
        tmax = np.sqrt(d2).astype(F)
        f = one
        if t == SPOT:
            L = np.broadcast_to(np.ascontiguousarray(L, F).reshape(-1, 3), (n, 3))
            S = np.ascontiguousarray(S, F).reshape(3)
            c = -((((S[0] * L[:, 0]).astype(F) + (S[1] * L[:, 1]).astype(F)).astype(F) + (S[2] * L[:, 2]).astype(F)).astype(F))
            f = mc.clamp(((c * F(light["coneScale"])).astype(F) + F(light["coneOffset"])).astype(F), 0.0, 1.0)
            dark |= ~(f > F(0.0))
            E = (E * (f * f).astype(F)[:, None]).astype(F)
    return dict(dark=dark, E=E, tmax=tmax, d2=d2, f=f)


def as_dir_light(rd, direction, color):
    """a SceneProperties whose lights[0] is DirLight{direction, color}"""
    sp = np.zeros((), rd.SceneProperties)
    sp["lightCount"][0] = 1
    sp["lights"][0]["direction"][:3] = np.ascontiguousarray(direction, F)
    sp["lights"][0]["color"][:3] = np.ascontiguousarray(color, F)
    sp["lights"][0]["color"][3] = 1.0
    return sp


# ---- the calls, on device buffers --------------------------------------------------------------------------------------------------
def punctual_batch(rd, plt, tlas, bR, bM, n, bT, index, want_shadow=True, query=True):
    """rd.PunctualLightHits(record `index` of the table buffer bT) -> QueryRays (any) on its shadow rays -> dict as
    material_cases.light_batch: lit (LIT_DTYPE), shadow (rd.RAY_DTYPE), occluded, and the buffers bL, bSh"""
    bL, bSh = rd.PunctualLightHits(bR, bM, n, bT, index, shadow=True if want_shadow else None)
    occluded = np.zeros(n, bool)
    shadow = None
    if want_shadow:
        shadow = sh.read(rd, plt, bSh, n, rd.RAY_DTYPE)
        if n and query:
            occluded = sh.read(rd, plt, rd.QueryRays(tlas, bSh, n, rd.QUERY_ANY), n, rd.RAY_HIT_DTYPE)["hit"] == 1
    return dict(lit=sh.read(rd, plt, bL, n, mc.LIT_DTYPE), shadow=shadow, occluded=occluded, bL=bL, bSh=bSh)


def is_dark(w):
    """rows of a punctual_batch whose lit and shadow records are zero bytes"""
    return ~w["lit"].view(np.uint8).reshape(-1, 16).any(1) & ~w["shadow"].view(np.uint8).reshape(-1, 32).any(1)


def trace(rd, plt, tlas, sb, rays, keys, max_depth, lights):
    """rd.TracePunctualPaths on uploaded copies of rays / keys / the table `lights` -> (radiance (n, 4) float32, invalid)"""
    n, L = rays.shape[0], lights.shape[0]
    bT = sh.upload(rd, plt, lights if L else np.zeros(1, rd.PUNCTUAL_LIGHT_DTYPE))
    bR, invalid = rd.TracePunctualPaths(tlas, sh.upload(rd, plt, rays), sh.upload(rd, plt, keys), n, max_depth, bT, L, sb)
    return (rd.ReadBuffer(plt, bR, 16 * n).view(F).reshape(n, 4).copy() if n else np.zeros((0, 4), F)), invalid


def public_loop_punctual(rd, plt, tlas, sb, surface_buffers, lights, rays, frames, pixels, max_depth):
    """light_paths_cases.public_loop with record j of the table `lights` through rd.PunctualLightHits in the place of light j of
    sb.scene through rd.LightHits; the shadow rays carry that call's tmax
    -> (color (n, 3), live rays per bounce, invalid summed over the bounces, first-hit-invalid mask (n,), (dark, lit) rows among the
    depth-0 hits per record)"""
    n, L = rays.shape[0], lights.shape[0]
    bT = sh.upload(rd, plt, lights if L else np.zeros(1, rd.PUNCTUAL_LIGHT_DTYPE))
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
        lit, occluded = np.zeros((m, L, 3), F), np.zeros((m, L), bool)
        for j in range(L):
            w = punctual_batch(rd, plt, tlas, bR, bM, m, bT, j)
            lit[:, j], occluded[:, j] = w["lit"]["rgb"], w["occluded"]
            if depth == 0:
                dark0.append((int((is_dark(w) & hit).sum()), int((~is_dark(w) & hit).sum())))
        r = sc.scatter(rd, plt, dict(bR=bR, bM=bM, bS=bS, n=m), keys=sh.keys_of(frames, pixels, depth), compact=True)
        src = r["src"].astype(np.int64)
        p = path[src]
        color[p], weight[p] = lp.fold_lights(lit[src], occluded[src], mc.ambient(mat["albedo"][src]), r["scatter"]["nextFactor"][src], color[p], weight[p])
        path, frames, pixels, rays = p, frames[src], pixels[src], r["next"]
        lives.append(r["live"])
        if r["live"] == 0:
            break
    return color, lives, invalid, first_invalid, dark0


def mixed_table(rd, lo, hi, sp, seed):
    """MAX_PATH_LIGHTS records of every kind inside the scene box lo .. hi, in an order that puts a ranged point light first, a
    spot second, a directional light third, a record of an unknown type (3: dark everywhere) fourth and an unranged point light
    fifth: every prefix the tests take (1, 5, 6, 16) holds a record that is dark for part of the scene, and those from 5 on hold the
    type-3 record.  Colours grow with the box so that a light matters at the box's scale"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    size = float(ext.max())
    power = size * size / 8.0
    dirs = directional_table(rd, sp)
    kinds = [(POINT, True), (SPOT, False), (DIRECTIONAL, False), (3, False), (POINT, False)]
    kinds += [((POINT, SPOT, DIRECTIONAL)[k % 3], k % 2 == 0) for k in range(rd.MAX_PATH_LIGHTS - len(kinds))]
    out, nd = [], 0
    for kind, ranged in kinds:
        pos = lo + ext * rng.uniform(0.2, 0.8, 3)
        col = rng.uniform(0.3, 1.0, 3) * power
        if kind == DIRECTIONAL:
            out.append(dirs[nd % dirs.shape[0]])
            nd += 1
            continue
        axis = np.array([rng.uniform(-0.5, 0.5), -1.0, rng.uniform(-0.5, 0.5)])
        inner = rng.uniform(10.0, 25.0)
        out.append(light(rd, kind, pos, axis, 0.45 * size if ranged else 0.0, col, rd.SpotCone(np.radians(inner), np.radians(inner + rng.uniform(10.0, 30.0)))))
    return table(rd, out)

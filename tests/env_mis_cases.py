"""Shared pieces of the tests of multiple-importance sampling of the environment (rdx_env_mis_weights, rdx_trace_paths_env_mis;
env.EnvMisWeights, env.TraceEnvMisPaths; test_env_mis_cpu.py, test_gpu_env_mis.py).  The numpy restatements here ARE the
specification of include/rdx.h, one IEEE operation at a time, under the contract of csrc/device_math.h: dot3 is an fma chain,
normalize3 is v * rsqrt(dot3(v, v)) -- numpy's 1 / sqrt is within an ulp of v_rsq_f32, so whatever stands behind a normalize3
carries a tolerance against the device.

  lobe_of            the lobe of a scatter sample from its random triple, the branches of sample_brdf_transm.
  scatter_pdf        NoL and the density of the two reflective lobes for L, float32.
  env_pdf            the density of the environment's table for d, float32, from env_cases.parts; the texel is
                     env_cases.lookup_texel's (float64: the tests keep away from the texel edges, border_distance says how far).
  mis_weight         the weight rule.
  weights_of         all of it for rows of (ray direction, material record, direction): what rdx_env_mis_weights writes.
  public_loop_env_mis  env_cases.public_loop_env with the three lines of MIS: the comparand of env.TraceEnvMisPaths.
  sample64, brdf64   the stock sampler's direction, nextFactor and lobe, and microfacet_brdf, in float64, for the statistical tests.
"""
import numpy as np

import area_cases as ar
import denoise_cases as dn
import env_cases as ec
import light_paths_cases as lp
import material_cases as mc
import punctual_cases as pu
import scatter_cases as sc
import shade_cases as sh

F = np.float32
U = np.uint32
PI_F = F(3.14159265359)
LOBE_DIFFUSE, LOBE_SPECULAR, LOBE_TRANSMISSION, LOBE_NONE = 0, 1, 2, 3
MIS_WEIGHT_DTYPE = np.dtype([("w_scatter", "<f4"), ("pdf_scatter", "<f4"), ("pdf_env", "<f4"), ("lobe", "<u4")])
dot3 = dn.dot3


def normalize3(v):
    """device_math.h normalize3 for vectors of ordinary size: zeros unchanged, else v * rsqrt(dot3(v, v))"""
    v = np.ascontiguousarray(v, F)
    with np.errstate(all="ignore"):
        l2 = dot3(v, v).astype(F)
        r = (F(1.0) / np.sqrt(l2)).astype(F)
        return np.where((v == 0).all(-1, keepdims=True), v, (v * r[..., None]).astype(F)).astype(F)


def clamp01(x):
    return np.minimum(np.maximum(np.asarray(x, F), F(0.0)), F(1.0)).astype(F)


def lobe_of(rnd, transmission):
    """rnd (n, 3) float32, transmission (n,) float32 -> (n,) uint32"""
    z = np.asarray(rnd, F)[..., 2]
    lower = z < F(0.5)
    trans = lower & ((F(2.0) * z).astype(F) < np.asarray(transmission, F))
    return np.where(trans, LOBE_TRANSMISSION, np.where(lower, LOBE_DIFFUSE, LOBE_SPECULAR)).astype(U)


def d_ggx(NoH, r):
    """stages.h d_ggx, float32"""
    with np.errstate(all="ignore"):
        alpha = (r * r).astype(F)
        a2 = (alpha * alpha).astype(F)
        den = (((NoH * NoH).astype(F) * (a2 - F(1.0)).astype(F)).astype(F) + F(1.0)).astype(F)
        return (a2 / ((PI_F * den).astype(F) * den).astype(F)).astype(F)


def scatter_pdf(N, V, L, r, transmission):
    """N, V, L (n, 3), r, transmission (n,), float32 -> (NoL, p_s) float32; p_s is 0 where NoL is not positive"""
    N, V, L = (np.ascontiguousarray(a, F) for a in (N, V, L))
    r, t = np.asarray(r, F), np.asarray(transmission, F)
    with np.errstate(all="ignore"):
        NoL = dot3(N, L).astype(F)
        H = normalize3((V + L).astype(F))
        NoH, VoH = clamp01(dot3(N, H)), clamp01(dot3(V, H))
        pSpec = ((d_ggx(NoH, r) * NoH).astype(F) / (F(4.0) * VoH).astype(F)).astype(F)
        pDiff = (np.minimum(NoL, F(1.0)) / PI_F).astype(F)
        that = clamp01(t)
        p = ((F(0.5) * pSpec).astype(F) + ((F(0.5) * (F(1.0) - that).astype(F)).astype(F) * pDiff).astype(F)).astype(F)
        return NoL, np.where(NoL > 0, p, F(0.0)).astype(F)


def shows_nothing(d):
    d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        return (d == 0).all(-1) | ~(np.abs(d) < np.inf).all(-1)


def env_pdf(p, W, H, d):
    """p = env_cases.parts(table); d (n, 3) float32 -> (n,) float32: ((float)q / (float)total) / (twoPiOverW * (rowCos[y] -
    rowCos[y + 1])) for the texel the environment shows along d; 0 where it shows nothing, for a header that is not W x H's and
    for total == 0"""
    d = np.ascontiguousarray(d, F).reshape(-1, 3)
    hd = p["header"]
    out = np.zeros(d.shape[0], F)
    total = int(hd["total"])
    if hd["magic"] != ec.MAGIC or hd["width"] != W or hd["height"] != H or total == 0:
        return out
    ok = ~shows_nothing(d)
    y, x = ec.lookup_texel(p, W, H, np.where(ok[:, None], d, F(1.0)))
    C, rc = p["C"], p["rowCos"]
    with np.errstate(all="ignore"):
        q = (C[y, x] - np.where(x > 0, C[y, np.maximum(x, 1) - 1], U(0))).astype(U)
        share = (q.astype(F) / F(total)).astype(F)
        omega = (F(hd["twoPiOverW"]) * (rc[y] - rc[y + 1]).astype(F)).astype(F)
        return np.where(ok, (share / omega).astype(F), F(0.0)).astype(F)


def border_distance(p, W, H, d):
    """d (n, 3) -> (distance of the column coordinate from the nearest column border in texels, distance of cos(theta) from the
    nearest rowCos edge), float64: how far a direction is from the places where OCML's atan2f and v_rsq_f32 may choose another texel
    than numpy"""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        c = d[:, 1] / np.linalg.norm(d, axis=1)
        phi = np.arctan2(d[:, 2], d[:, 0])
        phi = np.where(phi < 0, phi + 2.0 * np.pi, phi)
        col = phi * float(p["header"]["wOverTwoPi"])
        dcol = np.abs(col - np.round(col))
        drow = np.abs(c[:, None] - p["rowCos"].astype(np.float64)[None, 1:-1]).min(1) if H > 1 else np.full(d.shape[0], np.inf)
    return dcol, drow


def mis_weight(lobe, r, NoL, p_s, p_e):
    """the rule of include/rdx.h -> w_scatter (n,) float32"""
    lobe, r, NoL, p_s, p_e = np.asarray(lobe), np.asarray(r, F), np.asarray(NoL, F), np.asarray(p_s, F), np.asarray(p_e, F)
    with np.errstate(all="ignore"):
        a2 = ((r * r).astype(F) * (r * r).astype(F)).astype(F)
        s = (p_s + p_e).astype(F)
        one = (lobe == LOBE_TRANSMISSION) | ((lobe == LOBE_SPECULAR) & (a2 == 0)) | ~(NoL > 0) | ~(np.abs(p_s) < np.inf) | ~(np.abs(p_e) < np.inf) | ~(s > 0)
        return np.where(one, F(1.0), (p_s / s).astype(F)).astype(F)


def weights_of(p, W, H, ray_dir, mat, dirs, lobe):
    """what rdx_env_mis_weights writes for direction rows `dirs` (rd.RAY_DTYPE) seen from ray directions `ray_dir` (n, 3) and
    material records `mat` (n,), with lobes `lobe` (n,) -> MIS_WEIGHT_DTYPE (n,)"""
    n = dirs.shape[0]
    out = np.zeros(n, MIS_WEIGHT_DTYPE)
    d = np.ascontiguousarray(dirs["direction"], F)
    live = (mat["hit"] == 1) & (dirs["tmax"] != 0) & ~(d == 0).all(1)
    V = normalize3((-np.ascontiguousarray(ray_dir, F)).astype(F))
    NoL, ps = scatter_pdf(mat["normal"], V, d, mat["roughness"], mat["transmission"])
    pe = env_pdf(p, W, H, d)
    w = mis_weight(lobe, mat["roughness"], NoL, ps, pe)
    out["w_scatter"], out["pdf_scatter"], out["pdf_env"], out["lobe"] = w, ps, pe, lobe
    out[~live] = np.zeros((), MIS_WEIGHT_DTYPE)
    return out


# ---- the calls, on device buffers --------------------------------------------------------------------------------------------------
def mis_weights(rd, env, plt, bR, bM, dirs, e, keys=None, randoms=None, src=None, nrecords=None, **offsets):
    """env.EnvMisWeights on the uploaded direction rows `dirs` (numpy rd.RAY_DTYPE; keys / randoms / src numpy too) -> MIS_WEIGHT_DTYPE (n,)"""
    n = dirs.shape[0]
    if not n:
        return np.zeros(0, MIS_WEIGHT_DTYPE)
    up = lambda a: sh.upload(rd, plt, a) if a is not None else None
    out = env.EnvMisWeights(bR, bM, up(dirs), n, e, keys=up(keys), randoms=up(randoms), src=up(src), nrecords=nrecords, **offsets)
    return sh.read(rd, plt, out, n, MIS_WEIGHT_DTYPE)


def trace(rd, env, plt, tlas, sb, rays, keys, max_depth, lights, area, e):
    """env_cases.trace for env.TraceEnvMisPaths"""
    n, L, A = rays.shape[0], lights.shape[0], area.shape[0]
    bT = sh.upload(rd, plt, lights) if L else None
    bA = sh.upload(rd, plt, area) if A else None
    bR, invalid = env.TraceEnvMisPaths(tlas, sh.upload(rd, plt, rays), sh.upload(rd, plt, keys), n, max_depth, bT, L, bA, A, e, sb)
    return (rd.ReadBuffer(plt, bR, 16 * n).view(F).reshape(n, 4).copy() if n else np.zeros((0, 4), F)), invalid


def public_loop_env_mis(rd, env, plt, tlas, sb, surface_buffers, lights, area, e, rays, frames, pixels, max_depth, record=None):
    """env_cases.public_loop_env with the three lines of include/rdx.h: the environment's lit of a hit is scaled by 1 - w_scatter of
    its shadow direction (lobe NONE) at every depth but the last; w_scatter of the next direction is kept with the path; a live ray of depth >= 1 without a valid
    hit adds weight * (EnvLookup(ray).rgb * w).  record: a list that receives, per depth, a dict of what the loop saw
    -> (color (n, 3), live rays per bounce, invalid summed over the bounces, first-miss mask (n,))"""
    n, L, A = rays.shape[0], lights.shape[0], area.shape[0]
    bT = sh.upload(rd, plt, lights if L else np.zeros(1, rd.PUNCTUAL_LIGHT_DTYPE))
    bA = sh.upload(rd, plt, area if A else np.zeros(1, rd.AREA_LIGHT_DTYPE))
    color, weight = np.zeros((n, 3), F), np.ones((n, 3), F)
    path = np.arange(n)
    kept = np.zeros(n, F)             # per live ray: w_scatter of the sample that drew it
    frames, pixels = np.asarray(frames, np.uint32), np.asarray(pixels, np.uint32)
    lives, invalid, first_miss = [], 0, np.zeros(n, bool)
    for depth in range(max_depth):
        m = rays.shape[0]
        if not m:
            break
        bR = sh.upload(rd, plt, rays)
        bH = rd.QueryRays(tlas, bR, m, rd.QUERY_CLOSEST)
        bS, _ = rd.ResolveHits(tlas, bR, bH, m, surface_buffers)
        bM, inv = rd.ResolveMaterials(tlas, bR, bH, m, sb)
        invalid += inv
        mat = sh.read(rd, plt, bM, m, mc.MATERIAL_RECORD_DTYPE)
        hit = mat["hit"] == 1
        sky = ec.lookup(rd, env, plt, e, rays)[:, :3] if (~hit).any() else np.zeros((m, 3), F)
        if depth == 0:
            first_miss = ~hit
            color[path[~hit]] = sky[~hit]
        else:
            gone = path[~hit]
            color[gone] = (color[gone] + (weight[gone] * (sky[~hit] * kept[~hit, None]).astype(F)).astype(F)).astype(F)
        keys = sh.keys_of(frames, pixels, depth)
        lit, occluded = np.zeros((m, L + A + 1, 3), F), np.zeros((m, L + A + 1), bool)
        for j in range(L + A + 1):
            if j < L:
                w = pu.punctual_batch(rd, plt, tlas, bR, bM, m, bT, j)
                lit[:, j] = w["lit"]["rgb"]
            elif j < L + A:
                w = ar.area_batch(rd, plt, tlas, bR, bM, m, bA, j - L, keys=keys)
                lit[:, j] = w["lit"]["rgb"]
            else:
                w = ec.env_batch(rd, env, plt, tlas, bR, bM, m, e, keys=keys, stream=A)
                lit[:, j] = w["lit"]["rgb"]
                if depth + 1 < max_depth:         # a next ray is sampled and carries the other share
                    ws = mis_weights(rd, env, plt, bR, bM, w["shadow"], e)["w_scatter"]
                    lit[:, j] = (w["lit"]["rgb"] * (F(1.0) - ws).astype(F)[:, None]).astype(F)
            occluded[:, j] = w["occluded"]
        r = sc.scatter(rd, plt, dict(bR=bR, bM=bM, bS=bS, n=m), keys=keys, compact=True)
        src = r["src"].astype(np.int64)
        nxt = mis_weights(rd, env, plt, bR, bM, r["next"], e, keys=keys, src=r["src"], nrecords=m)
        if record is not None:
            record.append(dict(rays=rays, path=path, mat=mat, hit=hit, sky=sky, kept=kept, src=src, next=r["next"], mis=nxt,
                               nextFactor=r["scatter"]["nextFactor"], weight=weight.copy(), color=color.copy()))
        p = path[src]
        color[p], weight[p] = lp.fold_lights(lit[src], occluded[src], mc.ambient(mat["albedo"][src]), r["scatter"]["nextFactor"][src], color[p], weight[p])
        path, frames, pixels, rays, kept = p, frames[src], pixels[src], r["next"], nxt["w_scatter"]
        lives.append(r["live"])
    return color, lives, invalid, first_miss


# ---- float64: the stock sampler and BRDF, for the statistical tests ---------------------------------------------------------------------
def frame64(N):
    """the tangent frame of stages.h make_frame: (t, b, n) with t = normalize(cross((1, 0, 0), n)), or (0, 1, 0) where n is +-x"""
    N = np.asarray(N, np.float64)
    t = np.cross([1.0, 0.0, 0.0], N)
    t = np.array([0.0, 1.0, 0.0]) if 1.0 - abs(N[0]) <= 1e-6 else t / np.linalg.norm(t)
    return t, np.cross(N, t), N


def _schlick64(cos_theta, metallic, albedo):
    F0 = 0.04 + (np.asarray(albedo, np.float64) - 0.04) * metallic
    return F0 + (1.0 - F0) * ((1.0 - cos_theta) ** 5)[:, None]


def _lambda64(z, a):
    with np.errstate(all="ignore"):
        cos2 = z * z
        tan2 = np.maximum(0.0, 1.0 - cos2) / cos2
        return np.where(np.isinf(tan2), 0.0, (np.sqrt(1.0 + a * a * tan2) - 1.0) / 2.0)


def _g64(N, wo, wi, r):
    zo, zi = wo @ N, wi @ N
    return np.where((zi < 0) | (zo < 0), 0.0, 1.0 / (1.0 + _lambda64(zi, r) + _lambda64(zo, r)))


def brdf64(N, V, L, albedo, metallic, r, transmission=0.0):
    """stages.h microfacet_brdf x NoL, float64: V (3,), L (n, 3) -> (n, 3)"""
    N, V, L = np.asarray(N, np.float64), np.asarray(V, np.float64), np.asarray(L, np.float64)
    H = V + L
    H = H / np.linalg.norm(H, axis=1, keepdims=True)
    NoV, NoL = np.clip(N @ V, 0, 1), np.clip(L @ N, 0, 1)
    NoH, VoH = np.clip(H @ N, 0, 1), np.clip(H @ V, 0, 1)
    Fr = _schlick64(VoH, metallic, albedo)
    a2 = r ** 4
    D = a2 / (np.pi * (NoH * NoH * (a2 - 1.0) + 1.0) ** 2)
    G = _g64(N, np.broadcast_to(V, L.shape), L, r)
    spec = Fr * (D * G)[:, None] / np.maximum(4.0 * NoV * NoL, 0.001)[:, None]
    diff = (1.0 - Fr) * (1.0 - metallic) * (1.0 - transmission) * (np.asarray(albedo, np.float64) / np.pi)
    return (diff + spec) * NoL[:, None]


def sample64(N, V, albedo, metallic, r, transmission, rnd):
    """stages.h sample_brdf_transm for the two reflective lobes, float64: rnd (n, 3) -> (L (n, 3), nextFactor (n, 3), lobe (n,)).
    L and nextFactor of a transmission sample are zeros: the tests that use this count that lobe by its label alone"""
    N, V, rnd = np.asarray(N, np.float64), np.asarray(V, np.float64), np.asarray(rnd, np.float64)
    t, b, n = frame64(N)
    lobe = lobe_of(rnd.astype(F), np.full(rnd.shape[0], transmission, F))
    diffuse = lobe == LOBE_DIFFUSE
    a2 = r ** 4
    with np.errstate(all="ignore"):
        theta = np.where(diffuse, np.arccos(np.sqrt(rnd[:, 1])), np.arccos(np.sqrt((1.0 - rnd[:, 1]) / (1.0 + (a2 - 1.0) * rnd[:, 1]))))
    phi = 2.0 * np.pi * rnd[:, 0]
    st, ct = np.sin(theta), np.cos(theta)
    dirv = (st * np.cos(phi))[:, None] * t + (st * np.sin(phi))[:, None] * b + ct[:, None] * n
    refl = -V + dirv * (2.0 * (dirv @ V))[:, None]
    L = np.where(diffuse[:, None], dirv, refl)
    H = V + L
    H = np.where(diffuse[:, None], H / np.linalg.norm(H, axis=1, keepdims=True), dirv)
    VoH = np.clip(H @ V, 0, 1)
    Fr = _schlick64(VoH, metallic, albedo)
    NoV, NoH = np.clip(N @ V, 0, 1), np.clip(H @ N, 0, 1)
    G = _g64(N, np.broadcast_to(V, L.shape), L, r)
    nf_spec = Fr * (G * VoH / np.maximum(NoH * NoV, 0.001))[:, None] * 2.0
    nf_diff = (1.0 - Fr) * (1.0 - metallic) * np.asarray(albedo, np.float64) * 2.0
    nf = np.where(diffuse[:, None], nf_diff, nf_spec)
    trans = lobe == LOBE_TRANSMISSION
    return np.where(trans[:, None], 0.0, L), np.where(trans[:, None], 0.0, nf), lobe

"""Shared pieces of the tests of rd.TraceLightPaths / rdx_trace_paths_lights (test_light_paths_cpu.py, test_gpu_light_paths.py):
radiance along the caller's own rays with every light of the scene sampled at every hit.

The specification is the README's second Quick-start loop, which the tests already own as scatter_cases.path_tracer_numpy; the GPU
tests hold the call to it bit for bit.  Restated here:

  fold_lights   the per-hit fold of that loop in numpy float32, one IEEE operation at a time:
                    direct = (0, 0, 0);  for j = 0 .. L - 1:  direct = direct + (occluded_j ? 0 : lit_j)
                    radiance = direct + ambient;  color = color + weight * radiance;  weight = weight * nextFactor
                test_light_paths_cpu.py checks it on hand-made rows;
  public_loop   the same loop over the public calls on scene buffers of the caller's choice, which tolerates -- and counts -- hits
                the buffers do not describe (path_tracer_numpy asserts there are none).  test_gpu_light_paths.py holds it to
                path_tracer_numpy before using it as the comparand of the fencing test.
"""
import numpy as np

import material_cases as mc
import scatter_cases as sc
import shade_cases as sh

F = np.float32
N_LIGHTS = 5


def fold_lights(lit, occluded, ambient, next_factor, color, weight):
    """lit (n, L, 3), occluded (n, L) bool, ambient / next_factor / color / weight (n, 3) -> (color, weight) after the hit"""
    lit, occluded = np.ascontiguousarray(lit, F), np.asarray(occluded, bool)
    n, L = occluded.shape
    assert lit.shape == (n, L, 3)
    direct = np.zeros((n, 3), F)
    for j in range(L):
        direct = (direct + np.where(occluded[:, j, None], F(0), lit[:, j])).astype(F)
    radiance = (direct + np.ascontiguousarray(ambient, F)).astype(F)
    weight = np.ascontiguousarray(weight, F)
    color = (np.ascontiguousarray(color, F) + (weight * radiance).astype(F)).astype(F)
    return color, (weight * np.ascontiguousarray(next_factor, F)).astype(F)


def five_lights(rd):
    """material_cases.three_lights extended to the five lights a SceneProperties holds, of distinct directions and colours; light 1
    still shines upwards"""
    sp = np.array(mc.three_lights(rd)).copy()
    sp["lightCount"][0] = N_LIGHTS
    for j, (d, c) in ((3, ((0.6, -0.5, -0.62), (1.5, 3.0, 0.8))), (4, ((-0.1, -0.95, 0.3), (2.0, 2.0, 2.5)))):
        sp["lights"][j]["direction"] = (d[0], d[1], d[2], 0.0)
        sp["lights"][j]["color"] = (c[0], c[1], c[2], 1.0)
    dirs = np.array([sp["lights"][j]["direction"][:3] for j in range(N_LIGHTS)])
    cols = np.array([sp["lights"][j]["color"][:3] for j in range(N_LIGHTS)])
    assert np.unique(dirs, axis=0).shape[0] == N_LIGHTS and np.unique(cols, axis=0).shape[0] == N_LIGHTS
    return sp


def scene_buffer(rd, plt, sp):
    return sh.upload(rd, plt, np.array(sp).reshape(1))


def buffers_with_scene(rd, dev, scene, material=None):
    """dev.shading_buffers() with another SceneProperties buffer (and, optionally, another Material buffer)"""
    return rd.ShadingBuffers(scene, dev.meshInfoData, dev.indexData, dev.uvData, dev.normalData, material if material is not None else dev.materialData)


def trace(rd, plt, tlas, sb, rays, keys, max_depth, light_count):
    """rd.TraceLightPaths on uploaded copies of rays / keys -> (radiance (n, 4) float32, invalid)"""
    n = rays.shape[0]
    bR, invalid = rd.TraceLightPaths(tlas, sh.upload(rd, plt, rays), sh.upload(rd, plt, keys), n, max_depth, light_count, sb)
    return (rd.ReadBuffer(plt, bR, 16 * n).view(F).reshape(n, 4).copy() if n else np.zeros((0, 4), F)), invalid


def occlusion_at_depth0(rd, dev, scene, rays, lights=N_LIGHTS):
    """per light j: (depth-0 hits whose shadow ray towards j is occluded, hits whose shadow ray is not), by the public calls"""
    rec = sc.records(rd, dev, rays)
    hit = rec["mat"]["hit"] == 1
    out = []
    for j in range(lights):
        w = mc.light_batch(rd, dev.plt, dev.topAccelStruct, rec["bR"], rec["bM"], rays.shape[0], scene, j)
        out.append((int((w["occluded"] & hit).sum()), int((~w["occluded"] & hit).sum())))
    return out


def public_loop(rd, plt, tlas, sb, surface_buffers, light_count, rays, frames, pixels, max_depth):
    """scatter_cases.path_tracer_numpy on scene buffers of the caller's choice, the lights those of sb.scene, folded by fold_lights;
    a hit the buffers do not describe is a miss and is counted, as rd.ResolveMaterials counts it
    -> (color (n, 3), live rays per bounce, invalid summed over the bounces, first-hit-invalid mask (n,))"""
    n = rays.shape[0]
    color, weight = np.zeros((n, 3), F), np.ones((n, 3), F)
    path = np.arange(n)
    frames, pixels = np.asarray(frames, np.uint32), np.asarray(pixels, np.uint32)
    lives, invalid, first_invalid = [], 0, np.zeros(n, bool)
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
        lit, occluded = np.zeros((m, light_count, 3), F), np.zeros((m, light_count), bool)
        for j in range(light_count):
            w = mc.light_batch(rd, plt, tlas, bR, bM, m, sb.scene, j)
            lit[:, j], occluded[:, j] = w["lit"]["rgb"], w["occluded"]
        r = sc.scatter(rd, plt, dict(bR=bR, bM=bM, bS=bS, n=m), keys=sh.keys_of(frames, pixels, depth), compact=True)
        src = r["src"].astype(np.int64)
        p = path[src]
        color[p], weight[p] = fold_lights(lit[src], occluded[src], mc.ambient(mat["albedo"][src]), r["scatter"]["nextFactor"][src], color[p], weight[p])
        path, frames, pixels, rays = p, frames[src], pixels[src], r["next"]
        lives.append(r["live"])
        if r["live"] == 0:
            break
    return color, lives, invalid, first_invalid

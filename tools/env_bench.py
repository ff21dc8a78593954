#!/usr/bin/env python3
"""env_bench.py -- env.TraceEnvPaths (rdx_trace_paths_env) beside rd.TraceAreaPaths and beside the loop over
env.EnvLightHitsTorch it replaces, on the Sponza-class scene: the 2^21 camera rays of a 2048 x 1024 frame (rays and keys from
rd.GenerateRays, sample 1), depth 8, under the 1024 x 512 procedural sky.  After 3 warm-up rounds these legs ALTERNATE in this one
process, 20 rounds:
  a   rd.TraceAreaPaths with ONE directional record (the sun of the sky): ms_total and its ms_*
  b   env.TraceEnvPaths with the sky alone: one shadow ray per hit, as a
  c0  rd.TraceAreaPaths, three point lights inside the atrium
  c   env.TraceEnvPaths, the three point lights and the sky
  d   the README's fifth loop over env.EnvLightHitsTorch with the sky alone, from the same rays: wall time
  h0  rd.AreaLightHits, one quad, on the 2^21 material records of the camera rays: ms_shade
  h   env.EnvLightHits on the same records: ms_shade
Medians, min / max and max - min per leg.  b is compared once with the loop of d, bit for bit on all rays.  Then rdx_env_build
alone, 20 calls each for 1024 x 512 and 4096 x 2048: the time between the events around the upload of the header, the three
kernels and the padding (ms_shade), the bytes the kernels move (the image read twice, C written, M written and read) and that rate
as a share of the 8 TB/s an MI355X's HBM delivers at most.  No test gates on a time.  GPU only.
    python tools/env_bench.py [out.json]          (default: profiles/env_bench.json)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
torch.zeros(1, device="cuda").cpu()          # torch initialises the GPU first
import rrt_amd  # noqa: F401
from radiance_ray_tracing_amd import env, rd, scenes
from ray_query_bench import stat
import area_cases as ar
import material_cases as mc
import punctual_cases as pu

W, H, DEPTH, REPS, WARM, LIGHTS = 2048, 1024, 8, 20, 3, 3
N = W * H
FRAME = TOTAL = 1
STAGES = ("ms_extend", "ms_shade", "ms_shadow")
POINTS = ((0.0, 6.0, -8.0), (-4.0, 3.0, 2.0), (5.0, 7.0, 10.0))        # inside scenes.c2_atrium (x -12 .. 12, y 0 .. 9, z -20 .. 20)
COLORS = ((300.0, 280.0, 240.0), (120.0, 160.0, 220.0), (260.0, 200.0, 120.0))
SKY, SUN = (1024, 512), (0.3, 0.8, 0.52)
HBM_PEAK = 8.0e12


def readme_loop(tlas, sb, sf, rays, keys, frame, max_depth, sky):
    """the README's fifth loop with the sky alone, from given rays and keys -> colour (n, 4)"""
    n = rays.shape[0]
    pixel = keys[:, 1].contiguous()
    color = torch.zeros((n, 4), device="cuda")
    weight = torch.ones((n, 3), device="cuda")
    path = torch.arange(n, device="cuda")
    for depth in range(max_depth):
        if depth:
            keys = torch.stack([torch.full_like(pixel, frame), pixel, torch.full_like(pixel, depth), torch.zeros_like(pixel)], 1).contiguous()
        hits = rd.QueryRaysTorch(tlas, rays, rd.QUERY_CLOSEST)
        surf, _ = rd.ResolveHitsTorch(tlas, rays, hits, sf)
        mat, _ = rd.ResolveMaterialsTorch(tlas, rays, hits, sb)
        if depth == 0:
            missed = mat.view(torch.int32)[:, 3] != 1
            color[path[missed], :3] = env.EnvLookupTorch(rays, sky)[missed, :3]
        lit, shadow = env.EnvLightHitsTorch(rays, mat, sky, keys=keys, stream=0)
        occluded = rd.QueryRaysTorch(tlas, shadow, rd.QUERY_ANY)[:, 3:4] == 1
        radiance = torch.where(occluded, torch.zeros_like(lit[:, :3]), lit[:, :3]) + mat[:, 4:7] * 0.1
        scatter, rays, src, live = rd.ScatterHitsTorch(rays, mat, surf, keys)
        src = src.long()
        color[path[src], :3] += weight[path[src]] * radiance[src]
        weight[path[src]] *= scatter[src, 0:3]
        path, pixel = path[src], pixel[src].contiguous()
        if live == 0:
            break
    torch.cuda.synchronize()
    return color


def build_times(plt, width, height):
    image = env.ProceduralSky(width, height, SUN)
    e = env.CreateEnvironment(plt, image)
    ms = []
    for r in range(WARM + REPS):
        env.BuildEnvironment(e.image, width, height, e.table)
        if r >= WARM:
            ms.append(rd.GetTraceStats().ms_shade)
    texels = width * height
    moved = 2 * 16 * texels + 4 * texels + 3 * 8 * height + 4 * (height + 1)
    k = stat(ms)
    k.update(bytes_moved=moved, table_bytes=env.TableSize(width, height), GB_per_s=round(moved / (k["median"] * 1e-3) / 1e9, 1),
             share_of_hbm_peak=round(moved / (k["median"] * 1e-3) / HBM_PEAK, 4))
    return k


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "env_bench.json")
    plt = rd.Platform.GetPlatform()
    dev = scenes.DeviceScene(scenes.CONFIGS["c2_atrium"](W, H, 1, DEPTH))
    assert dev.width * dev.height == N == 1 << 21
    cam = dev.frame_buffers()[0]
    tlas, sf = dev.topAccelStruct, dev.surface_buffers()
    sp3 = np.array(mc.three_lights(rd)).reshape(1)
    scene3 = rd.CreateBuffer(plt, sp3.nbytes)
    rd.WriteBuffer(plt, scene3, sp3.nbytes, sp3)
    sb3 = rd.ShadingBuffers(scene3, dev.meshInfoData, dev.indexData, dev.uvData, dev.normalData, dev.materialData)
    points = pu.table(rd, [pu.light(rd, pu.POINT, p, color=c) for p, c in zip(POINTS, COLORS)])
    sun = pu.table(rd, [pu.light(rd, pu.DIRECTIONAL, direction=tuple(-x for x in SUN), color=(3.0, 2.7, 2.2))])
    quad = ar.table(rd, [rd.QuadLight((-1.0, 6.0, -9.0), (2.0, 0, 0), (0, 0, 2.0), (75.0, 70.0, 60.0))])
    bP, bS, bQ = (rd.CreateBuffer(plt, t.nbytes) for t in (points, sun, quad))
    for b, t in ((bP, points), (bS, sun), (bQ, quad)):
        rd.WriteBuffer(plt, b, t.nbytes, t)
    sky = env.CreateEnvironment(plt, env.ProceduralSky(SKY[0], SKY[1], SUN))
    bR, bK = rd.GenerateRays(cam, N, FRAME, TOTAL)
    out = {leg: rd.CreateBuffer(plt, N * 16) for leg in ("a", "b", "c0", "c")}
    tR = torch.from_numpy(rd.ReadBuffer(plt, bR, N * 32).view(np.float32).reshape(N, 8).copy()).cuda()
    tK = torch.from_numpy(rd.ReadBuffer(plt, bK, N * 16).view(np.int32).reshape(N, 4).copy()).cuda()
    bH = rd.QueryRays(tlas, bR, N, rd.QUERY_CLOSEST)
    bM, _ = rd.ResolveMaterials(tlas, bR, bH, N, sb3)
    bLit, bSh = rd.CreateBuffer(plt, N * 16), rd.CreateBuffer(plt, N * 32)
    rd.SetProfiling(True)
    path_legs = {"a": ("a_area_paths_1_directional", lambda o: rd.TraceAreaPaths(tlas, bR, bK, N, DEPTH, bS, 1, None, 0, sb3, radiance=o)),
                 "b": ("b_env_paths_sky_alone", lambda o: env.TraceEnvPaths(tlas, bR, bK, N, DEPTH, None, 0, None, 0, sky, sb3, radiance=o)),
                 "c0": ("c0_area_paths_3_point", lambda o: rd.TraceAreaPaths(tlas, bR, bK, N, DEPTH, bP, LIGHTS, None, 0, sb3, radiance=o)),
                 "c": ("c_env_paths_3_point_and_sky", lambda o: env.TraceEnvPaths(tlas, bR, bK, N, DEPTH, bP, LIGHTS, None, 0, sky, sb3, radiance=o))}
    names = [v[0] for v in path_legs.values()] + ["d_readme_loop_sky_alone_wall", "h0_area_light_hits_ms_shade", "h_env_light_hits_ms_shade"]
    total = {name: [] for name in names}
    stages = {leg: {s: [] for s in STAGES} for leg in path_legs}
    counts = {}
    for r in range(WARM + REPS):
        st = {}
        for leg, (_, call) in path_legs.items():
            call(out[leg])
            st[leg] = rd.GetTraceStats()
        t0 = time.perf_counter()
        readme_loop(tlas, sb3, sf, tR, tK, FRAME, DEPTH, sky)
        wall = (time.perf_counter() - t0) * 1e3
        rd.AreaLightHits(bR, bM, N, bQ, 0, keys=bK, lit=bLit, shadow=bSh)
        h0 = rd.GetTraceStats().ms_shade
        env.EnvLightHits(bR, bM, N, sky, keys=bK, stream=0, lit=bLit, shadow=bSh)
        h = rd.GetTraceStats().ms_shade
        if r < WARM:
            continue
        for name, v in zip(names, [st[leg].ms_total for leg in path_legs] + [wall, h0, h]):
            total[name].append(v)
        for leg in path_legs:
            for s in STAGES:
                stages[leg][s].append(getattr(st[leg], s))
        counts = {leg: [int(st[leg].rays_primary), int(st[leg].rays_bounce), int(st[leg].rays_shadow), int(st[leg].launches_extend), int(st[leg].launches_shadow)]
                  for leg in path_legs}
    rd.SetProfiling(False)
    got_b = rd.ReadBuffer(plt, out["b"], N * 16).view(np.uint32).reshape(N, 4).copy()
    loop_b = readme_loop(tlas, sb3, sf, tR, tK, FRAME, DEPTH, sky)
    b_is_loop = bool(np.array_equal(got_b[:, :3], loop_b.cpu().numpy().view(np.uint32)[:, :3]))
    assert b_is_loop and counts["a"][:2] == counts["b"][:2] and counts["a"][2] == counts["b"][2], (b_is_loop, counts)
    k = {name: stat(v) for name, v in total.items()}
    for name, v in total.items():
        k[name]["spread"] = round(float(np.max(v) - np.min(v)), 4)
    a, b, c0, c, d, h0, h = (k[n]["median"] for n in names)
    med = {leg: {s: round(float(np.median(v)), 4) for s, v in st.items()} for leg, st in stages.items()}
    res = {"device": rd.Platform.device_name(), "scene": "c2_atrium (Sponza-class)", "rays": N, "frame": "%d x %d, sample %d, depth %d" % (W, H, FRAME, DEPTH),
           "sky": "%d x %d procedural" % SKY, "reps": REPS, "warmup_rounds": WARM, "unit": "ms", "ms": k, "b_over_a": round(b / a, 4), "b_minus_a": round(b - a, 4),
           "c_over_c0": round(c / c0, 4), "c_minus_c0": round(c - c0, 4), "d_over_b": round(d / b, 2), "h_over_h0": round(h / h0, 3),
           "stage_ms_median": med, "rays_primary_bounce_shadow_launches_extend_shadow": counts,
           "bytes_per_path_of_a_chunk": {"1 record": 192 + 80, "4 records": 192 + 80 * 4}, "b_equals_readme_loop_on_all_rays": b_is_loop,
           "env_build": {"%d x %d" % s: build_times(plt, *s) for s in ((1024, 512), (4096, 2048))}}
    print("ms: a TraceAreaPaths(1 directional) %.3f | b TraceEnvPaths(sky) %.3f | b / a %.4f | c0 3 point %.3f | c 3 point + sky %.3f | d README loop %.1f | "
          "AreaLightHits %.3f, EnvLightHits %.3f | stages %s | build %s" % (a, b, b / a, c0, c, d, h0, h, med, res["env_build"]), flush=True)
    print(json.dumps(res))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""area_bench.py -- rd.TraceAreaPaths (rdx_trace_paths_area) beside rd.TracePunctualPaths and beside the loop over
rd.AreaLightHitsTorch it replaces, on the Sponza-class scene: the 2^21 camera rays of a 2048 x 1024 frame (rays and keys from
rd.GenerateRays, sample 1), depth 8.  After 3 warm-up rounds these legs ALTERNATE in this one process, 20 rounds:
  a   rd.TracePunctualPaths, three point lights inside the atrium, profiling on: rdx_get_trace_stats().ms_total (the HIP events
      around the whole call) and its ms_*
  b   rd.TraceAreaPaths on the same three records and NO area records: ms_total and its ms_*
  c   rd.TraceAreaPaths, no punctual records, three down-facing 2 x 2 quads centred on those points: ms_total and its ms_*
  d   rd.TraceAreaPaths, the three point lights and the three quads: ms_total and its ms_*
  e   the README's loop over rd.AreaLightHitsTorch with the three quads of c, from the same rays: wall time
Medians, min / max and max - min per leg; b / a, c / a, e / c.  The legs' results are compared once, outside the rounds: b against
a and c against e, bit for bit on all rays, and d against the same loop over both tables; the loops also count the shadow rays of c
and d whose record is dark at the hit (they are traced, and accept nothing).  No test gates on a time.  GPU only.
    python tools/area_bench.py [out.json]          (default: profiles/area_bench.json)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
torch.zeros(1, device="cuda").cpu()          # torch initialises the GPU first
import rrt_amd  # noqa: F401
from radiance_ray_tracing_amd import rd, scenes
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
SIDE = 2.0


def readme_loop(tlas, sb, sf, rays, keys, frame, max_depth, lights_t, area_t):
    """the README's loop over the punctual table `lights_t` and the area table `area_t` (either may be None) from given rays and
    keys -> (colour (n, 4), shadow rays, those of them whose record is dark at the hit)"""
    n = rays.shape[0]
    pixel = keys[:, 1].contiguous()
    color = torch.zeros((n, 4), device="cuda")
    weight = torch.ones((n, 3), device="cuda")
    path = torch.arange(n, device="cuda")
    miss_colour = torch.tensor([0.2, 0.2, 0.5], device="cuda")
    shadow_rays = dark = 0
    for depth in range(max_depth):
        if depth:
            keys = torch.stack([torch.full_like(pixel, frame), pixel, torch.full_like(pixel, depth), torch.zeros_like(pixel)], 1).contiguous()
        hits = rd.QueryRaysTorch(tlas, rays, rd.QUERY_CLOSEST)
        surf, _ = rd.ResolveHitsTorch(tlas, rays, hits, sf)
        mat, _ = rd.ResolveMaterialsTorch(tlas, rays, hits, sb)
        hit = mat.view(torch.int32)[:, 3] == 1
        if depth == 0:
            color[path[~hit], :3] = miss_colour
        direct = torch.zeros((rays.shape[0], 3), device="cuda")
        calls = [lambda j=j: rd.PunctualLightHitsTorch(rays, mat, lights_t, j) for j in range(0 if lights_t is None else lights_t.shape[0])]
        calls += [lambda j=j: rd.AreaLightHitsTorch(rays, mat, area_t, j, keys=keys) for j in range(0 if area_t is None else area_t.shape[0])]
        for call in calls:
            lit, shadow = call()
            occluded = rd.QueryRaysTorch(tlas, shadow, rd.QUERY_ANY)[:, 3:4] == 1
            direct += torch.where(occluded, torch.zeros_like(lit[:, :3]), lit[:, :3])
            shadow_rays += int(hit.sum())
            dark += int((hit & (shadow[:, 7] == 0)).sum())
        radiance = direct + mat[:, 4:7] * 0.1
        scatter, rays, src, live = rd.ScatterHitsTorch(rays, mat, surf, keys)
        src = src.long()
        color[path[src], :3] += weight[path[src]] * radiance[src]
        weight[path[src]] *= scatter[src, 0:3]
        path, pixel = path[src], pixel[src].contiguous()
        if live == 0:
            break
    torch.cuda.synchronize()
    return color, shadow_rays, dark


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "area_bench.json")
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
    # a point light's `color` is its intensity; a quad of area A and radiance R seen head-on from afar has intensity R * A
    quads = ar.table(rd, [rd.QuadLight((p[0] - SIDE / 2, p[1], p[2] - SIDE / 2), (SIDE, 0, 0), (0, 0, SIDE), tuple(x / (SIDE * SIDE) for x in c))
                          for p, c in zip(POINTS, COLORS)])
    assert points.shape[0] == quads.shape[0] == LIGHTS
    bP, bQ = rd.CreateBuffer(plt, points.nbytes), rd.CreateBuffer(plt, quads.nbytes)
    rd.WriteBuffer(plt, bP, points.nbytes, points)
    rd.WriteBuffer(plt, bQ, quads.nbytes, quads)
    tP, tQ = (torch.from_numpy(t.view(np.float32).reshape(-1, 16).copy()).cuda() for t in (points, quads))
    bR, bK = rd.GenerateRays(cam, N, FRAME, TOTAL)
    out = {leg: rd.CreateBuffer(plt, N * 16) for leg in "abcd"}
    tR = torch.from_numpy(rd.ReadBuffer(plt, bR, N * 32).view(np.float32).reshape(N, 8).copy()).cuda()
    tK = torch.from_numpy(rd.ReadBuffer(plt, bK, N * 16).view(np.int32).reshape(N, 4).copy()).cuda()
    rd.SetProfiling(True)
    legs = ("a_punctual_paths_3_point", "b_area_paths_3_point_0_quads", "c_area_paths_0_point_3_quads", "d_area_paths_3_point_3_quads", "e_readme_loop_3_quads_wall")
    total = {name: [] for name in legs}
    stages = {leg: {s: [] for s in STAGES} for leg in "abcd"}
    counts = {}
    area_legs = dict(b=(bP, LIGHTS, None, 0), c=(None, 0, bQ, LIGHTS), d=(bP, LIGHTS, bQ, LIGHTS))
    for r in range(WARM + REPS):
        st = {}
        rd.TracePunctualPaths(tlas, bR, bK, N, DEPTH, bP, LIGHTS, sb3, radiance=out["a"])
        st["a"] = rd.GetTraceStats()
        for leg, (lt, lc, at, ac) in area_legs.items():
            rd.TraceAreaPaths(tlas, bR, bK, N, DEPTH, lt, lc, at, ac, sb3, radiance=out[leg])
            st[leg] = rd.GetTraceStats()
        t0 = time.perf_counter()
        readme_loop(tlas, sb3, sf, tR, tK, FRAME, DEPTH, None, tQ)
        wall = (time.perf_counter() - t0) * 1e3
        if r < WARM:
            continue
        for name, v in zip(legs, [st[leg].ms_total for leg in "abcd"] + [wall]):
            total[name].append(v)
        for leg in "abcd":
            for s in STAGES:
                stages[leg][s].append(getattr(st[leg], s))
        counts = {leg: [int(st[leg].rays_primary), int(st[leg].rays_bounce), int(st[leg].rays_shadow), int(st[leg].launches_extend), int(st[leg].launches_shadow)]
                  for leg in "abcd"}
    rd.SetProfiling(False)
    # the legs computed the same thing
    got = {leg: rd.ReadBuffer(plt, out[leg], N * 16).view(np.uint32).reshape(N, 4).copy() for leg in "abcd"}
    loop_c, shadow_c, dark_c = readme_loop(tlas, sb3, sf, tR, tK, FRAME, DEPTH, None, tQ)
    loop_d, shadow_d, dark_d = readme_loop(tlas, sb3, sf, tR, tK, FRAME, DEPTH, tP, tQ)
    b_is_a = bool(np.array_equal(got["b"], got["a"]))
    c_is_e = bool(np.array_equal(got["c"][:, :3], loop_c.cpu().numpy().view(np.uint32)[:, :3]))
    d_is_loop = bool(np.array_equal(got["d"][:, :3], loop_d.cpu().numpy().view(np.uint32)[:, :3]))
    assert b_is_a and c_is_e and d_is_loop and counts["a"] == counts["b"] and shadow_c == counts["c"][2] and shadow_d == counts["d"][2], \
        (b_is_a, c_is_e, d_is_loop, counts, shadow_c, shadow_d)
    k = {name: stat(v) for name, v in total.items()}
    for name, v in total.items():
        k[name]["spread"] = round(float(np.max(v) - np.min(v)), 4)
    a, b, c, d, e = (k[n]["median"] for n in legs)
    med = {leg: {s: round(float(np.median(v)), 4) for s, v in st.items()} for leg, st in stages.items()}
    spread_ab = max(k[legs[0]]["spread"], k[legs[1]]["spread"])
    res = {"device": rd.Platform.device_name(), "scene": "c2_atrium (Sponza-class)", "rays": N, "frame": "%d x %d, sample %d, depth %d" % (W, H, FRAME, DEPTH),
           "reps": REPS, "warmup_rounds": WARM, "unit": "ms", "ms": k, "b_over_a": round(b / a, 4), "b_minus_a": round(b - a, 4),
           "b_within_the_larger_spread_of_a_and_b": bool(abs(b - a) <= spread_ab), "c_over_a": round(c / a, 4), "d_over_a": round(d / a, 4), "e_over_c": round(e / c, 2),
           "stage_ms_median": med, "rays_primary_bounce_shadow_launches_extend_shadow": counts,
           "c_shadow_rays": shadow_c, "c_shadow_rays_of_dark_records": dark_c, "c_dark_share": round(dark_c / max(shadow_c, 1), 4),
           "d_shadow_rays": shadow_d, "d_shadow_rays_of_dark_records": dark_d, "d_dark_share": round(dark_d / max(shadow_d, 1), 4),
           "bytes_per_path_of_a_chunk": {"3 records": 192 + 80 * LIGHTS, "6 records": 192 + 80 * 2 * LIGHTS},
           "b_equals_trace_punctual_paths": b_is_a, "c_equals_readme_loop_on_all_rays": c_is_e, "d_equals_readme_loop": d_is_loop}
    print("ms: a TracePunctualPaths(3 point) %.3f (spread %.3f) | b TraceAreaPaths(3 point, 0 quads) %.3f (spread %.3f) | b / a %.4f | c 3 quads %.3f (spread %.3f), "
          "%d of %d shadow rays dark | d 3 point + 3 quads %.3f (spread %.3f), %d of %d shadow rays dark | e README loop, 3 quads %.1f (spread %.1f) | e / c %.2f | stages %s"
          % (a, k[legs[0]]["spread"], b, k[legs[1]]["spread"], b / a, c, k[legs[2]]["spread"], dark_c, shadow_c, d, k[legs[3]]["spread"], dark_d, shadow_d, e,
             k[legs[4]]["spread"], e / c, med), flush=True)
    print(json.dumps(res))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

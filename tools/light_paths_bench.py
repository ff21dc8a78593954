#!/usr/bin/env python3
"""light_paths_bench.py -- rd.TraceLightPaths (rdx_trace_paths_lights) beside rd.TracePaths and beside the loop over the public
calls it replaces, on the Sponza-class scene: the 2^21 camera rays of a 2048 x 1024 frame (rays and keys from rd.GenerateRays,
sample 1), depth 8.  After 3 warm-up rounds these legs ALTERNATE in this one process, 20 rounds:
  a   rd.TraceLightPaths, light_count 1, the scene's own SceneProperties, profiling on: rdx_get_trace_stats().ms_total and its ms_*
  b   rd.TracePaths on the same rays, profiling on: ms_total and its ms_*          -- yardstick: the frame path's stages
  c   rd.TraceLightPaths, light_count 3, under material_cases.three_lights: ms_total and its ms_*
  d   the README's second loop in torch with 3 lights, from the same rays: wall time
Medians, min / max and max - min per leg; a / b and d / c; a's and b's stage times side by side (a: ms_extend = the closest-hit
queries, ms_shade = k_lights_shade + k_lights_fold, ms_shadow = the any-hit queries; b: ms_extend = the first segment, ms_generate =
k_paths_ingest, ms_shade, ms_fused = shadow(d) + extend(d + 1) in one launch, ms_shadow = the last depth's).  The legs' results are
compared once, outside the rounds: a against b and c against d, bit for bit.  No test gates on a time.  GPU only.
    python tools/light_paths_bench.py [out.json]          (default: profiles/light_paths_bench.json)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
torch.zeros(1, device="cuda").cpu()          # torch initialises the GPU first
import rrt_amd  # noqa: F401
from radiance_ray_tracing_amd import rd, scenes
from ray_query_bench import stat
import material_cases as mc

W, H, DEPTH, REPS, WARM, LIGHTS = 2048, 1024, 8, 20, 3, 3
N = W * H
FRAME = TOTAL = 1
STAGES = ("ms_generate", "ms_extend", "ms_shade", "ms_sort", "ms_fused", "ms_shadow")


def readme_loop(tlas, sb, sf, rays, keys, frame, max_depth, light_count):
    """the second loop of the README from given rays and keys -> colour (n, 4)"""
    n = rays.shape[0]
    pixel = keys[:, 1].contiguous()
    color = torch.zeros((n, 4), device="cuda")
    weight = torch.ones((n, 3), device="cuda")
    path = torch.arange(n, device="cuda")
    miss_colour = torch.tensor([0.2, 0.2, 0.5], device="cuda")
    for depth in range(max_depth):
        if depth:
            keys = torch.stack([torch.full_like(pixel, frame), pixel, torch.full_like(pixel, depth), torch.zeros_like(pixel)], 1).contiguous()
        hits = rd.QueryRaysTorch(tlas, rays, rd.QUERY_CLOSEST)
        surf, _ = rd.ResolveHitsTorch(tlas, rays, hits, sf)
        mat, _ = rd.ResolveMaterialsTorch(tlas, rays, hits, sb)
        if depth == 0:
            color[path[mat.view(torch.int32)[:, 3] != 1], :3] = miss_colour
        direct = torch.zeros((rays.shape[0], 3), device="cuda")
        for j in range(light_count):
            lit, shadow = rd.LightHitsTorch(rays, mat, sb.scene, j)
            occluded = rd.QueryRaysTorch(tlas, shadow, rd.QUERY_ANY)[:, 3:4] == 1
            direct += torch.where(occluded, torch.zeros_like(lit[:, :3]), lit[:, :3])
        radiance = direct + mat[:, 4:7] * 0.1
        scatter, rays, src, live = rd.ScatterHitsTorch(rays, mat, surf, keys)
        src = src.long()
        color[path[src], :3] += weight[path[src]] * radiance[src]
        weight[path[src]] *= scatter[src, 0:3]
        path, pixel = path[src], pixel[src].contiguous()
        if live == 0:
            break
    torch.cuda.synchronize()
    return color


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "light_paths_bench.json")
    plt = rd.Platform.GetPlatform()
    dev = scenes.DeviceScene(scenes.CONFIGS["c2_atrium"](W, H, 1, DEPTH))
    assert dev.width * dev.height == N == 1 << 21
    cam = dev.frame_buffers()[0]
    tlas, sb1, sf = dev.topAccelStruct, dev.shading_buffers(), dev.surface_buffers()
    sp3 = np.array(mc.three_lights(rd)).reshape(1)
    scene3 = rd.CreateBuffer(plt, sp3.nbytes)
    rd.WriteBuffer(plt, scene3, sp3.nbytes, sp3)
    sb3 = rd.ShadingBuffers(scene3, dev.meshInfoData, dev.indexData, dev.uvData, dev.normalData, dev.materialData)
    bR, bK = rd.GenerateRays(cam, N, FRAME, TOTAL)
    bA, bB, bC = (rd.CreateBuffer(plt, N * 16) for _ in range(3))
    tR = torch.from_numpy(rd.ReadBuffer(plt, bR, N * 32).view(np.float32).reshape(N, 8).copy()).cuda()
    tK = torch.from_numpy(rd.ReadBuffer(plt, bK, N * 16).view(np.int32).reshape(N, 4).copy()).cuda()
    rd.SetProfiling(True)
    legs = ("a_light_paths_1", "b_trace_paths", "c_light_paths_3", "d_readme_loop_3_wall")
    total = {name: [] for name in legs}
    stages = {leg: {s: [] for s in STAGES} for leg in "abc"}
    counts = {}
    for r in range(WARM + REPS):
        rd.TraceLightPaths(tlas, bR, bK, N, DEPTH, 1, sb1, radiance=bA)
        sa = rd.GetTraceStats()
        rd.TracePaths(tlas, bR, bK, N, DEPTH, sb1, radiance=bB)
        sB = rd.GetTraceStats()
        rd.TraceLightPaths(tlas, bR, bK, N, DEPTH, LIGHTS, sb3, radiance=bC)
        sC = rd.GetTraceStats()
        t0 = time.perf_counter()
        readme_loop(tlas, sb3, sf, tR, tK, FRAME, DEPTH, LIGHTS)
        wall = (time.perf_counter() - t0) * 1e3
        if r < WARM:
            continue
        for name, v in zip(legs, (sa.ms_total, sB.ms_total, sC.ms_total, wall)):
            total[name].append(v)
        for leg, st in zip("abc", (sa, sB, sC)):
            for s in STAGES:
                stages[leg][s].append(getattr(st, s))
        counts = {leg: [int(st.rays_primary), int(st.rays_bounce), int(st.rays_shadow), int(st.launches_extend), int(st.launches_shadow)]
                  for leg, st in zip("abc", (sa, sB, sC))}
    rd.SetProfiling(False)
    # the legs computed the same thing
    ra, rb, rc3 = (rd.ReadBuffer(plt, b, N * 16).view(np.uint32).reshape(N, 4).copy() for b in (bA, bB, bC))
    loop = readme_loop(tlas, sb3, sf, tR, tK, FRAME, DEPTH, LIGHTS).cpu().numpy().view(np.uint32)
    a_is_b, c_is_d = bool(np.array_equal(ra, rb)), bool(np.array_equal(rc3[:, :3], loop[:, :3]))
    assert a_is_b and c_is_d and counts["a"][:3] == counts["b"][:3], (a_is_b, c_is_d, counts)
    k = {name: stat(v) for name, v in total.items()}
    for name, v in total.items():
        k[name]["spread"] = round(float(np.max(v) - np.min(v)), 4)
    a, b, c, d = (k[n]["median"] for n in legs)
    med = {leg: {s: round(float(np.median(v)), 4) for s, v in st.items()} for leg, st in stages.items()}
    spread_cd = k["c_light_paths_3"]["spread"] + k["d_readme_loop_3_wall"]["spread"]
    res = {"device": rd.Platform.device_name(), "scene": "c2_atrium (Sponza-class)", "rays": N, "frame": "%d x %d, sample %d, depth %d" % (W, H, FRAME, DEPTH),
           "reps": REPS, "warmup_rounds": WARM, "unit": "ms", "ms": k, "a_over_b": round(a / b, 4), "d_over_c": round(d / c, 2),
           "c_below_d_by_more_than_the_two_spreads": bool(d - c > spread_cd), "stage_ms_median": med,
           "rays_primary_bounce_shadow_launches_extend_shadow": counts, "bytes_per_path_of_a_chunk": {"1 light": 192 + 80, "3 lights": 192 + 80 * LIGHTS},
           "a_equals_trace_paths": a_is_b, "c_equals_readme_loop": c_is_d}
    print("ms: a TraceLightPaths(1) %.3f (spread %.3f) | b TracePaths %.3f (spread %.3f) | a / b %.3f | c TraceLightPaths(3) %.3f (spread %.3f) | "
          "d README loop, 3 lights %.1f (spread %.1f) | d / c %.2f | stages %s"
          % (a, k[legs[0]]["spread"], b, k[legs[1]]["spread"], a / b, c, k[legs[2]]["spread"], d, k[legs[3]]["spread"], d / c, med), flush=True)
    print(json.dumps(res))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

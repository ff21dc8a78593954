#!/usr/bin/env python3
"""env_mis_bench.py -- env.TraceEnvMisPaths (rdx_trace_paths_env_mis) beside env.TraceEnvPaths, on the Sponza-class scene: the 2^21
camera rays of a 2048 x 1024 frame (rays and keys from rd.GenerateRays, sample 1), depth 8, under the 1024 x 512 procedural sky.
After 3 warm-up rounds these legs ALTERNATE in this one process, 20 rounds:
  a   env.TraceEnvPaths with the sky alone: ms_total and its ms_*
  b   env.TraceEnvMisPaths with the sky alone; ms_shade is k_env_mis_shade and k_env_mis_fold over the depths -- the library's stage
      timer brackets a depth's shade and fold kernels together, so the two are reported as one figure beside a's k_env_shade and
      k_lights_fold
  c   env.TraceEnvPaths, three point lights inside the atrium and the sky
  d   env.TraceEnvMisPaths, the same
  h   env.EnvLightHits on the 2^21 material records of the camera rays: ms_shade
  w   env.EnvMisWeights on the shadow rows h wrote (lobe NONE): ms_shade
  w2  env.EnvMisWeights on the next rows of rd.ScatterHits, keys route with src: ms_shade
Medians, min / max per leg, and the ratios b / a and d / c as measured in this run.  No test gates on a time.  GPU only.
    python tools/env_mis_bench.py [out.json]          (default: profiles/env_mis_bench.json)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
torch.zeros(1, device="cuda").cpu()          # torch initialises the GPU first
import rrt_amd  # noqa: F401
from radiance_ray_tracing_amd import env, rd, scenes
from ray_query_bench import stat
import material_cases as mc
import punctual_cases as pu

W, H, DEPTH, REPS, WARM, LIGHTS = 2048, 1024, 8, 20, 3, 3
N = W * H
FRAME = TOTAL = 1
STAGES = ("ms_extend", "ms_shade", "ms_shadow")
POINTS = ((0.0, 6.0, -8.0), (-4.0, 3.0, 2.0), (5.0, 7.0, 10.0))        # inside scenes.c2_atrium (x -12 .. 12, y 0 .. 9, z -20 .. 20)
COLORS = ((300.0, 280.0, 240.0), (120.0, 160.0, 220.0), (260.0, 200.0, 120.0))
SKY, SUN = (1024, 512), (0.3, 0.8, 0.52)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "env_mis_bench.json")
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
    bP = rd.CreateBuffer(plt, points.nbytes)
    rd.WriteBuffer(plt, bP, points.nbytes, points)
    sky = env.CreateEnvironment(plt, env.ProceduralSky(SKY[0], SKY[1], SUN))
    bR, bK = rd.GenerateRays(cam, N, FRAME, TOTAL)
    bH = rd.QueryRays(tlas, bR, N, rd.QUERY_CLOSEST)
    bS, _ = rd.ResolveHits(tlas, bR, bH, N, sf)
    bM, _ = rd.ResolveMaterials(tlas, bR, bH, N, sb3)
    bLit, bSh, bWt = rd.CreateBuffer(plt, N * 16), rd.CreateBuffer(plt, N * 32), rd.CreateBuffer(plt, N * 16)
    _, bNext, bSrc, live = rd.ScatterHits(bR, bM, bS, bK, N, compact=True)
    out = {leg: rd.CreateBuffer(plt, N * 16) for leg in "abcd"}
    rd.SetProfiling(True)
    path_legs = {"a": ("a_env_paths_sky_alone", lambda o: env.TraceEnvPaths(tlas, bR, bK, N, DEPTH, None, 0, None, 0, sky, sb3, radiance=o)),
                 "b": ("b_env_mis_paths_sky_alone", lambda o: env.TraceEnvMisPaths(tlas, bR, bK, N, DEPTH, None, 0, None, 0, sky, sb3, radiance=o)),
                 "c": ("c_env_paths_3_point_and_sky", lambda o: env.TraceEnvPaths(tlas, bR, bK, N, DEPTH, bP, LIGHTS, None, 0, sky, sb3, radiance=o)),
                 "d": ("d_env_mis_paths_3_point_and_sky", lambda o: env.TraceEnvMisPaths(tlas, bR, bK, N, DEPTH, bP, LIGHTS, None, 0, sky, sb3, radiance=o))}
    names = [v[0] for v in path_legs.values()] + ["h_env_light_hits_ms_shade", "w_env_mis_weights_shadow_rows_ms_shade", "w2_env_mis_weights_next_rows_ms_shade"]
    total = {name: [] for name in names}
    stages = {leg: {s: [] for s in STAGES} for leg in path_legs}
    counts = {}
    for r in range(WARM + REPS):
        st = {}
        for leg, (_, call) in path_legs.items():
            call(out[leg])
            st[leg] = rd.GetTraceStats()
        env.EnvLightHits(bR, bM, N, sky, keys=bK, stream=0, lit=bLit, shadow=bSh)
        h = rd.GetTraceStats().ms_shade
        env.EnvMisWeights(bR, bM, bSh, N, sky, out=bWt)
        w = rd.GetTraceStats().ms_shade
        env.EnvMisWeights(bR, bM, bNext, live, sky, keys=bK, src=bSrc, nrecords=N, out=bWt)
        w2 = rd.GetTraceStats().ms_shade
        if r < WARM:
            continue
        for name, v in zip(names, [st[leg].ms_total for leg in path_legs] + [h, w, w2]):
            total[name].append(v)
        for leg in path_legs:
            for s in STAGES:
                stages[leg][s].append(getattr(st[leg], s))
        counts = {leg: [int(st[leg].rays_primary), int(st[leg].rays_bounce), int(st[leg].rays_shadow), int(st[leg].launches_extend), int(st[leg].launches_shadow)]
                  for leg in path_legs}
    rd.SetProfiling(False)
    assert counts["a"] == counts["b"] and counts["c"] == counts["d"], counts       # the same rays are traced: MIS changes colours, not paths
    rad = {leg: rd.ReadBuffer(plt, out[leg], N * 16).view(np.float32).reshape(N, 4)[:, :3].astype(np.float64).mean(0).round(5).tolist() for leg in "abcd"}
    k = {name: stat(v) for name, v in total.items()}
    a, b, c, d, h, w, w2 = (k[n]["median"] for n in names)
    med = {leg: {s: round(float(np.median(v)), 4) for s, v in st.items()} for leg, st in stages.items()}
    res = {"device": rd.Platform.device_name(), "scene": "c2_atrium (Sponza-class)", "rays": N, "frame": "%d x %d, sample %d, depth %d" % (W, H, FRAME, DEPTH),
           "sky": "%d x %d procedural" % SKY, "reps": REPS, "warmup_rounds": WARM, "unit": "ms", "ms": k, "b_over_a": round(b / a, 4), "b_minus_a": round(b - a, 4),
           "d_over_c": round(d / c, 4), "d_minus_c": round(d - c, 4), "shade_and_fold_b_over_a": round(med["b"]["ms_shade"] / med["a"]["ms_shade"], 4),
           "w_over_h": round(w / h, 3), "next_rows": int(live), "stage_ms_median": med, "rays_primary_bounce_shadow_launches_extend_shadow": counts,
           "mean_radiance": rad}
    print("ms: a TraceEnvPaths(sky) %.3f | b TraceEnvMisPaths(sky) %.3f | b / a %.4f | c 3 point + sky %.3f | d MIS %.3f | d / c %.4f | EnvLightHits %.3f, "
          "EnvMisWeights %.3f (shadow rows) %.3f (%d next rows) | stages %s" % (a, b, b / a, c, d, d / c, h, w, w2, live, med), flush=True)
    print(json.dumps(res))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

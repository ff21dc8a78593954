#!/usr/bin/env python3
"""material_bench.py -- rd.ResolveMaterials / rd.LightHits (rdx_resolve_materials, rdx_light_hits) beside the two record calls they
stand next to, on the Sponza-class scene, 2^21 closest-hit records: 2^20 primary rays and 2^20 rays scattered from their hit
points (the rays of tools/ray_query_bench.py).  After a warm-up these legs ALTERNATE in this one process, REPS times each:
  r   rd.ResolveHits on the records of a closest-hit query                -- yardstick: the parent's unchanged kernel
  s   rd.ShadeHits on the same records, next + shadow rays, not compacting -- yardstick: the parent's unchanged kernel
  m   rd.ResolveMaterials on the same records
  l   rd.LightHits(light 0) on the records m wrote, with shadow rays
  l0  the same without shadow rays
Per leg: kernel time (HIP events around the launch: rdx_get_trace_stats().ms_shade), median / min / max.  Written out: m / r,
m / s, (m + l) / s -- the two new calls against the one call whose colour they reproduce -- l0 / l, and GB/s of m and l over
the bytes they stream (m: 32 + 32 in, 64 out per ray; l: 16 + 64 in, 16 + 32 out).  GPU only.
    python tools/material_bench.py [out.json]          (default: profiles/material_bench.json)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np
import rrt_amd  # noqa: F401
from radiance_ray_tracing_amd import rd, scenes
from ray_query_bench import N, SIDE, rays_of, stat

REPS, WARM = 20, 3
M_BYTES, L_BYTES, L0_BYTES = 32 + 32 + 64, 16 + 64 + 16 + 32, 16 + 64 + 16


def measure():
    plt = rd.Platform.GetPlatform()
    dev = scenes.DeviceScene(scenes.CONFIGS["c2_atrium"](SIDE, SIDE, 1, 8))
    o, d, rate = rays_of(dev)
    assert o.shape[0] == N
    rays = np.zeros(N, rd.RAY_DTYPE)
    rays["origin"], rays["direction"], rays["tmin"], rays["tmax"] = o, d, 0.001, 1000.0
    keys = np.zeros(N, rd.SHADE_KEY_DTYPE)
    keys["frameID"], keys["pixel"], keys["depth"] = np.arange(N) % 7, np.arange(N) % (SIDE * SIDE), np.arange(N) // (SIDE * SIDE)
    bR, bH, bK = rd.CreateBuffer(plt, N * 32), rd.CreateBuffer(plt, N * 32), rd.CreateBuffer(plt, N * 16)
    bO, bS, bN, bSh = rd.CreateBuffer(plt, N * 64), rd.CreateBuffer(plt, N * 48), rd.CreateBuffer(plt, N * 32), rd.CreateBuffer(plt, N * 32)
    bM, bL, bLs = rd.CreateBuffer(plt, N * 64), rd.CreateBuffer(plt, N * 16), rd.CreateBuffer(plt, N * 32)
    rd.WriteBuffer(plt, bR, N * 32, rays)
    rd.WriteBuffer(plt, bK, N * 16, keys)
    tl, sb, hb = dev.topAccelStruct, dev.surface_buffers(), dev.shading_buffers()
    rd.QueryRays(tl, bR, N, rd.QUERY_CLOSEST, bH)
    hit_rate = float((rd.ReadBuffer(plt, bH, N * 32).view(rd.RAY_HIT_DTYPE)["hit"] == 1).mean())
    assert rd.ResolveMaterials(tl, bR, bH, N, hb, bM)[1] == 0
    legs = {"r_resolve": lambda: rd.ResolveHits(tl, bR, bH, N, sb, bO),
            "s_shade": lambda: rd.ShadeHits(tl, bR, bH, bK, N, hb, bS, bN, bSh),
            "m_resolve_materials": lambda: rd.ResolveMaterials(tl, bR, bH, N, hb, bM),
            "l_light_hits": lambda: rd.LightHits(bR, bM, N, hb.scene, 0, bL, bLs),
            "l0_light_hits_no_shadow": lambda: rd.LightHits(bR, bM, N, hb.scene, 0, bL, None)}
    kern = {k: [] for k in legs}
    for r in range(WARM + REPS):
        for name, call in legs.items():
            call()
            if r >= WARM:
                kern[name].append(rd.GetTraceStats().ms_shade)
    return {name: stat(v) for name, v in kern.items()}, hit_rate, rate


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "material_bench.json")
    k, hit_rate, rate = measure()
    r, s, m, l, l0 = (k[n]["median"] for n in ("r_resolve", "s_shade", "m_resolve_materials", "l_light_hits", "l0_light_hits_no_shadow"))
    res = {"device": rd.Platform.device_name(), "scene": "c2_atrium (Sponza-class)", "rays": N,
           "rays_note": "2^20 primary rays (%dx%d) + 2^20 scattered from their hit points; %.3f of the primaries hit" % (SIDE, SIDE, rate),
           "hit_rate": round(hit_rate, 4), "reps": REPS, "warmup_rounds": WARM, "unit": "ms", "kernel_ms": k,
           "resolve_materials_over_resolve": round(m / r, 4), "resolve_materials_over_shade": round(m / s, 4),
           "resolve_materials_plus_light_hits_over_shade": round((m + l) / s, 4), "no_shadow_over_light_hits": round(l0 / l, 4),
           "streamed_bytes_per_ray": {"m_resolve_materials": M_BYTES, "l_light_hits": L_BYTES, "l0_light_hits_no_shadow": L0_BYTES},
           "streamed_GBps": {"m_resolve_materials": round(N * M_BYTES / m * 1e-6, 1), "l_light_hits": round(N * L_BYTES / l * 1e-6, 1),
                             "l0_light_hits_no_shadow": round(N * L0_BYTES / l0 * 1e-6, 1)},
           "grays_per_s": {name: round(N / v["median"] * 1e-6, 3) for name, v in k.items()}}
    print("kernel ms: resolve %.3f  shade %.3f  resolve materials %.3f  light hits %.3f  without shadow %.3f | (m + l) / shade %.2f"
          % (r, s, m, l, l0, (m + l) / s), flush=True)
    print(json.dumps(res))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

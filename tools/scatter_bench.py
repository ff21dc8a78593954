#!/usr/bin/env python3
"""scatter_bench.py -- rd.ScatterHits (rdx_scatter_hits) beside the record calls it stands next to, on the Sponza-class scene, 2^21
closest-hit records: 2^20 primary rays and 2^20 rays scattered from their hit points (the rays of tools/ray_query_bench.py).
After a warm-up these legs ALTERNATE in this one process, REPS times each:
  s   rd.ShadeHits on the records of a closest-hit query, next + shadow rays, not compacting -- yardstick: the parent's unchanged kernel
  r   rd.ResolveHits on the same records                                                     -- yardstick: the parent's unchanged kernel
  m   rd.ResolveMaterials on the same records                                                -- yardstick: the parent's unchanged kernel
  l   rd.LightHits(light 0) on the records m wrote, with shadow rays                         -- yardstick: the parent's unchanged kernel
  c   rd.ScatterHits on the records r and m wrote, keys, not compacting
  cs  the same with `src`: survivors packed
Per leg: kernel time (HIP events around the launch: rdx_get_trace_stats().ms_shade), median / min / max.  Written out beside each
other: the one rd.ShadeHits call, and the sum r + m + l + c that replaces it for one light; cs / c; GB/s of c over the bytes it
streams (16 + 64 + 16 + 16 in, 16 + 32 out per ray).  GPU only.
    python tools/scatter_bench.py [out.json]          (default: profiles/scatter_bench.json)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np
import rrt_amd  # noqa: F401
from radiance_ray_tracing_amd import rd, scenes
from ray_query_bench import N, SIDE, rays_of, stat

REPS, WARM = 20, 3
C_BYTES = 16 + 64 + 16 + 16 + 16 + 32


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
    bC, bCn, bSrc = rd.CreateBuffer(plt, N * 16), rd.CreateBuffer(plt, N * 32), rd.CreateBuffer(plt, N * 4)
    rd.WriteBuffer(plt, bR, N * 32, rays)
    rd.WriteBuffer(plt, bK, N * 16, keys)
    tl, sb, hb = dev.topAccelStruct, dev.surface_buffers(), dev.shading_buffers()
    rd.QueryRays(tl, bR, N, rd.QUERY_CLOSEST, bH)
    hit_rate = float((rd.ReadBuffer(plt, bH, N * 32).view(rd.RAY_HIT_DTYPE)["hit"] == 1).mean())
    assert rd.ResolveHits(tl, bR, bH, N, sb, bO)[1] == 0 and rd.ResolveMaterials(tl, bR, bH, N, hb, bM)[1] == 0
    # the records of both routes agree before anything is timed: scatter = bytes 32 .. 47 of shade, and the same next rays
    live_s = rd.ShadeHits(tl, bR, bH, bK, N, hb, bS, bN, bSh)[4]
    live_c = rd.ScatterHits(bR, bM, bO, bK, N, scatter=bC, next=bCn)[3]
    shade = rd.ReadBuffer(plt, bS, N * 48).reshape(N, 48)
    assert live_s == live_c and np.array_equal(shade[:, 32:48].reshape(-1), rd.ReadBuffer(plt, bC, N * 16))
    assert np.array_equal(rd.ReadBuffer(plt, bN, N * 32), rd.ReadBuffer(plt, bCn, N * 32))
    legs = {"s_shade": lambda: rd.ShadeHits(tl, bR, bH, bK, N, hb, bS, bN, bSh),
            "r_resolve": lambda: rd.ResolveHits(tl, bR, bH, N, sb, bO),
            "m_resolve_materials": lambda: rd.ResolveMaterials(tl, bR, bH, N, hb, bM),
            "l_light_hits": lambda: rd.LightHits(bR, bM, N, hb.scene, 0, bL, bLs),
            "c_scatter_hits": lambda: rd.ScatterHits(bR, bM, bO, bK, N, scatter=bC, next=bCn),
            "cs_scatter_hits_src": lambda: rd.ScatterHits(bR, bM, bO, bK, N, scatter=bC, next=bCn, src=bSrc)}
    kern = {k: [] for k in legs}
    for r in range(WARM + REPS):
        for name, call in legs.items():
            call()
            if r >= WARM:
                kern[name].append(rd.GetTraceStats().ms_shade)
    return {name: stat(v) for name, v in kern.items()}, hit_rate, rate


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "scatter_bench.json")
    k, hit_rate, rate = measure()
    s, r, m, l, c, cs = (k[n]["median"] for n in ("s_shade", "r_resolve", "m_resolve_materials", "l_light_hits", "c_scatter_hits", "cs_scatter_hits_src"))
    total = r + m + l + c
    res = {"device": rd.Platform.device_name(), "scene": "c2_atrium (Sponza-class)", "rays": N,
           "rays_note": "2^20 primary rays (%dx%d) + 2^20 scattered from their hit points; %.3f of the primaries hit" % (SIDE, SIDE, rate),
           "hit_rate": round(hit_rate, 4), "reps": REPS, "warmup_rounds": WARM, "unit": "ms", "kernel_ms": k,
           "one_shade_hits_call": round(s, 4), "resolve_plus_materials_plus_one_light_plus_scatter": round(total, 4),
           "split_over_shade": round(total / s, 4), "scatter_over_shade": round(c / s, 4), "src_over_scatter": round(cs / c, 4),
           "streamed_bytes_per_ray": {"c_scatter_hits": C_BYTES}, "streamed_GBps": {"c_scatter_hits": round(N * C_BYTES / c * 1e-6, 1)},
           "grays_per_s": {name: round(N / v["median"] * 1e-6, 3) for name, v in k.items()}}
    print("kernel ms: shade %.3f | resolve %.3f + resolve materials %.3f + light hits %.3f + scatter %.3f = %.3f (%.2f x shade) | scatter with src %.3f"
          % (s, r, m, l, c, total, total / s, cs), flush=True)
    print(json.dumps(res))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

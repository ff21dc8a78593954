#!/usr/bin/env python3
"""surface_bench.py -- rd.ResolveHits (rdx_resolve_hits) beside the query it follows, on the Sponza-class scene, 2^21 closest-hit
queries: 2^20 primary rays and 2^20 rays scattered from their hit points (the rays of tools/ray_query_bench.py).
After a warm-up these legs ALTERNATE in this one process, REPS times each:
  q   rd.QueryRays, closest hit, every ray with (0.001, 1000)            -- the comparand: the parent's unchanged kernel
  r   rd.ResolveHits on the records q wrote
  r0  the same without a uv stream (scene_buffers.uv = None): no uv gathers
  r1  the same on records rewritten to triangle 0 of their instance: the index / normal / uv gathers of a wave fall on a few
      cache lines (the hit flags, the instances and with them the matrix gathers stay as they are)
Per leg: kernel time (HIP events around the launch: rdx_get_trace_stats().ms_extend for q, .ms_shade for the others), median /
min / max.  Written out: the ratio r / q, GB/s of r over the bytes it streams (32 + 32 in, 64 out per ray) and over the nominal
bytes with the gathers of a hit (MeshInfo 32, slot 4, indices 12, normals 36, uv 24, inv + fwd 128), and r0 / r, r1 / r, which
say what the gathers cost.  GPU only.
    python tools/surface_bench.py [out.json]          (default: profiles/surface_bench.json)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np
import rrt_amd  # noqa: F401
from radiance_ray_tracing_amd import rd, scenes
from ray_query_bench import N, SIDE, rays_of, stat

REPS, WARM = 20, 3
STREAM_BYTES, GATHER_BYTES = 32 + 32 + 64, 32 + 4 + 12 + 36 + 24 + 128


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "surface_bench.json")
    plt = rd.Platform.GetPlatform()
    dev = scenes.DeviceScene(scenes.CONFIGS["c2_atrium"](SIDE, SIDE, 1, 8))
    o, d, rate = rays_of(dev)
    assert o.shape[0] == N
    rays = np.zeros(N, rd.RAY_DTYPE)
    rays["origin"], rays["direction"], rays["tmin"], rays["tmax"] = o, d, 0.001, 1000.0
    bR, bH, bH1, bO = rd.CreateBuffer(plt, N * 32), rd.CreateBuffer(plt, N * 32), rd.CreateBuffer(plt, N * 32), rd.CreateBuffer(plt, N * 64)
    rd.WriteBuffer(plt, bR, N * 32, rays)
    tl, sb = dev.topAccelStruct, dev.surface_buffers()
    sb0 = rd.SurfaceBuffers(sb.meshInfo, sb.index, None, sb.normal)
    rd.QueryRays(tl, bR, N, rd.QUERY_CLOSEST, bH)
    rec = rd.ReadBuffer(plt, bH, N * 32).view(rd.RAY_HIT_DTYPE).copy()
    hit_rate = float((rec["hit"] == 1).mean())
    rec["primitiveIndex"] = 0
    rd.WriteBuffer(plt, bH1, N * 32, rec)
    legs = {"q_query": lambda: rd.QueryRays(tl, bR, N, rd.QUERY_CLOSEST, bH),
            "r_resolve": lambda: rd.ResolveHits(tl, bR, bH, N, sb, bO),
            "r0_resolve_no_uv": lambda: rd.ResolveHits(tl, bR, bH, N, sb0, bO),
            "r1_resolve_one_triangle": lambda: rd.ResolveHits(tl, bR, bH1, N, sb, bO)}
    kern = {k: [] for k in legs}
    invalid = {}
    for r in range(WARM + REPS):
        for name, call in legs.items():
            ret = call()
            st = rd.GetTraceStats()
            if r >= WARM:
                kern[name].append(st.ms_extend if name[0] == "q" else st.ms_shade)
            elif name[0] == "r":
                invalid[name] = ret[1]
    assert not any(invalid.values()), invalid
    k = {name: stat(v) for name, v in kern.items()}
    q, r = k["q_query"]["median"], k["r_resolve"]["median"]
    nominal = STREAM_BYTES + GATHER_BYTES * hit_rate
    res = {"device": rd.Platform.device_name(), "scene": "c2_atrium (Sponza-class)", "rays": N,
           "rays_note": "2^20 primary rays (%dx%d) + 2^20 scattered from their hit points; %.3f of the primaries hit" % (SIDE, SIDE, rate),
           "hit_rate": round(hit_rate, 4), "reps": REPS, "warmup_rounds": WARM, "unit": "ms", "kernel_ms": k,
           "q_kernel_spread_ms": round(k["q_query"]["max"] - k["q_query"]["min"], 4),
           "resolve_over_query": round(r / q, 4),
           "resolve_costs_no_more_than_the_query": bool(r <= q),
           "streamed_bytes_per_ray": STREAM_BYTES, "nominal_bytes_per_ray_with_gathers": round(nominal, 1),
           "resolve_streamed_GBps": round(N * STREAM_BYTES / r * 1e-6, 1),
           "resolve_nominal_GBps": round(N * nominal / r * 1e-6, 1),
           "no_uv_over_resolve": round(k["r0_resolve_no_uv"]["median"] / r, 4),
           "one_triangle_over_resolve": round(k["r1_resolve_one_triangle"]["median"] / r, 4),
           "grays_per_s": {name: round(N / v["median"] * 1e-6, 3) for name, v in k.items()}}
    print("kernel ms: query %.3f (spread %.3f)  resolve %.3f  no uv %.3f  one triangle %.3f | resolve / query %.3f | %.0f GB/s streamed, %.0f nominal"
          % (q, res["q_kernel_spread_ms"], r, k["r0_resolve_no_uv"]["median"], k["r1_resolve_one_triangle"]["median"], r / q,
             res["resolve_streamed_GBps"], res["resolve_nominal_GBps"]), flush=True)
    print(json.dumps(res))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

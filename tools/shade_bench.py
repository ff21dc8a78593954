#!/usr/bin/env python3
"""shade_bench.py -- rd.ShadeHits (rdx_shade_hits) beside the two calls it stands next to, on the Sponza-class scene, 2^21
closest-hit records: 2^20 primary rays and 2^20 rays scattered from their hit points (the rays of tools/ray_query_bench.py).
After a warm-up these legs ALTERNATE in this one process, REPS times each:
  q   rd.QueryRays, closest hit, every ray with (0.001, 1000)            -- yardstick: the parent's unchanged kernel
  r   rd.ResolveHits on the records q wrote                              -- yardstick: the parent's unchanged kernel
  s   rd.ShadeHits on the same records, next + shadow rays, not compacting (record k = i)
  sc  the same, compacting (src given: survivors packed, one atomic per wave)
  s0  not compacting, without `next` (the next direction is not sampled: the last bounce)
Per leg: kernel time (HIP events around the launch: rdx_get_trace_stats().ms_extend for q, .ms_shade for the others), median /
min / max.  Written out: s / r, s / q, sc / s, s0 / s, and GB/s of s over the bytes it streams (32 + 32 + 16 in, 48 out per ray,
64 more per hit).
Where the time goes: the timing experiments of csrc/stages.h need libraries of their own (wrong results, timing only), e.g.
    RDX_DEFINES=-DRDX_EXP_SHADE_CHEAP RDX_LIB_NAME=librdx_exp_shade_cheap.so python radiance-ray-tracing_amd/build.py --force
    RDX_DEFINES=-DRDX_EXP_SHADE_NOGATHER RDX_LIB_NAME=librdx_exp_shade_nogather.so python radiance-ray-tracing_amd/build.py --force
Each such library that exists next to librdx.so is measured in a child process of its own (legs q and s only; q shows that the
child's clock is the parent's) and reported as cheap_over_shade (all loads, none of the BRDF arithmetic) / nogather_over_shade
(no dependent index and normal gathers).  GPU only.
    python tools/shade_bench.py [out.json]          (default: profiles/shade_bench.json)"""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np
import rrt_amd  # noqa: F401
from radiance_ray_tracing_amd import rd, scenes
from ray_query_bench import N, SIDE, rays_of, stat

REPS, WARM = 20, 3
STREAM_BYTES, PER_HIT_BYTES = 32 + 32 + 16 + 48, 32 + 32
VARIANTS = {"cheap": "librdx_exp_shade_cheap.so", "nogather": "librdx_exp_shade_nogather.so"}


def measure(only=None):
    plt = rd.Platform.GetPlatform()
    dev = scenes.DeviceScene(scenes.CONFIGS["c2_atrium"](SIDE, SIDE, 1, 8))
    o, d, rate = rays_of(dev)
    assert o.shape[0] == N
    rays = np.zeros(N, rd.RAY_DTYPE)
    rays["origin"], rays["direction"], rays["tmin"], rays["tmax"] = o, d, 0.001, 1000.0
    keys = np.zeros(N, rd.SHADE_KEY_DTYPE)
    keys["frameID"], keys["pixel"], keys["depth"] = np.arange(N) % 7, np.arange(N) % (SIDE * SIDE), np.arange(N) // (SIDE * SIDE)
    bR, bH, bK = rd.CreateBuffer(plt, N * 32), rd.CreateBuffer(plt, N * 32), rd.CreateBuffer(plt, N * 16)
    bO, bS, bN, bSh, bSrc = rd.CreateBuffer(plt, N * 64), rd.CreateBuffer(plt, N * 48), rd.CreateBuffer(plt, N * 32), rd.CreateBuffer(plt, N * 32), rd.CreateBuffer(plt, N * 4)
    rd.WriteBuffer(plt, bR, N * 32, rays)
    rd.WriteBuffer(plt, bK, N * 16, keys)
    tl, sb, hb = dev.topAccelStruct, dev.surface_buffers(), dev.shading_buffers()
    rd.QueryRays(tl, bR, N, rd.QUERY_CLOSEST, bH)
    hit_rate = float((rd.ReadBuffer(plt, bH, N * 32).view(rd.RAY_HIT_DTYPE)["hit"] == 1).mean())
    legs = {"q_query": lambda: rd.QueryRays(tl, bR, N, rd.QUERY_CLOSEST, bH),
            "r_resolve": lambda: rd.ResolveHits(tl, bR, bH, N, sb, bO),
            "s_shade": lambda: rd.ShadeHits(tl, bR, bH, bK, N, hb, bS, bN, bSh),
            "sc_shade_compacting": lambda: rd.ShadeHits(tl, bR, bH, bK, N, hb, bS, bN, bSh, bSrc),
            "s0_shade_no_next": lambda: rd.ShadeHits(tl, bR, bH, bK, N, hb, bS, None, bSh)}
    if only:
        legs = {k: v for k, v in legs.items() if k in only}
    kern = {k: [] for k in legs}
    counts = {}
    for r in range(WARM + REPS):
        for name, call in legs.items():
            ret = call()
            st = rd.GetTraceStats()
            if r >= WARM:
                kern[name].append(st.ms_extend if name[0] == "q" else st.ms_shade)
            elif name[0] == "s":
                counts[name] = ret[4:]
    assert all(c == (round(hit_rate * N), 0) for c in counts.values()), (counts, hit_rate * N)
    return {name: stat(v) for name, v in kern.items()}, hit_rate, rate


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":          # a timing-experiment library (RDX_LIB): legs q and s only
        k, _, _ = measure(only=("q_query", "s_shade"))
        print("CHILD " + json.dumps(k))
        return
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "shade_bench.json")
    k, hit_rate, rate = measure()
    q, r, s = k["q_query"]["median"], k["r_resolve"]["median"], k["s_shade"]["median"]
    nominal = STREAM_BYTES + PER_HIT_BYTES * hit_rate
    res = {"device": rd.Platform.device_name(), "scene": "c2_atrium (Sponza-class)", "rays": N,
           "rays_note": "2^20 primary rays (%dx%d) + 2^20 scattered from their hit points; %.3f of the primaries hit" % (SIDE, SIDE, rate),
           "hit_rate": round(hit_rate, 4), "reps": REPS, "warmup_rounds": WARM, "unit": "ms", "kernel_ms": k,
           "q_kernel_spread_ms": round(k["q_query"]["max"] - k["q_query"]["min"], 4),
           "shade_over_resolve": round(s / r, 4), "shade_over_query": round(s / q, 4),
           "shade_costs_no_more_than_the_query": bool(s <= q),
           "compacting_over_shade": round(k["sc_shade_compacting"]["median"] / s, 4),
           "no_next_over_shade": round(k["s0_shade_no_next"]["median"] / s, 4),
           "streamed_bytes_per_ray": STREAM_BYTES, "streamed_bytes_per_ray_with_the_rays_of_a_hit": round(nominal, 1),
           "shade_streamed_GBps": round(N * nominal / s * 1e-6, 1),
           "grays_per_s": {name: round(N / v["median"] * 1e-6, 3) for name, v in k.items()}}
    for name, lib in VARIANTS.items():
        path = os.path.join(ROOT, "radiance-ray-tracing_amd", lib)
        if not os.path.exists(path):
            continue
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, RDX_LIB=path), capture_output=True, text=True, timeout=900)
        line = [l for l in out.stdout.splitlines() if l.startswith("CHILD ")]
        if out.returncode != 0 or not line:
            res["experiment_" + name] = {"error": (out.stdout + out.stderr)[-500:]}
            continue
        kc = json.loads(line[0][6:])
        res["experiment_" + name] = {"library": lib, "kernel_ms": kc, name + "_over_shade": round(kc["s_shade"]["median"] / s, 4),
                                     "its_query_over_this_query": round(kc["q_query"]["median"] / q, 4)}
    print("kernel ms: query %.3f (spread %.3f)  resolve %.3f  shade %.3f  compacting %.3f  no next %.3f | shade / resolve %.2f | shade / query %.3f | %.0f GB/s streamed"
          % (q, res["q_kernel_spread_ms"], r, s, k["sc_shade_compacting"]["median"], k["s0_shade_no_next"]["median"], s / r, s / q, res["shade_streamed_GBps"]), flush=True)
    print(json.dumps(res))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

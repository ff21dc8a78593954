#!/usr/bin/env python3
"""ray_query_bench.py -- the device-resident ray query (rd.QueryRays) against the test seam (rd.TraceBatch) on the Sponza-class
scene, 2^21 rays: 2^20 primary rays and 2^20 rays scattered from their hit points (the construction of tools/trav_bench.py).
After a warm-up, three legs ALTERNATE in this one process, REPS times each, for closest hit (kind 1) and any hit (kind 2):
  a  rd.TraceBatch, production kernel, interval (0.001, 1000): host arrays in, 112-byte records out
  b  rd.QueryRays, the same rays in a device buffer, every ray with (0.001, 1000)
  c  rd.QueryRays, ray i with interval INTERVALS[i % 13] of tests/ray_edge_cases.py (zero, empty, infinite and NaN bounds among them)
Per leg: kernel time (rdx_get_trace_stats().ms_extend, HIP events around the launch) and wall time of the call, median / min / max;
the margin for "b is slower than a" is the min-to-max spread of a's kernel time in this run.  GPU only.
    python tools/ray_query_bench.py [out.json]          (default: profiles/ray_query_bench.json)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import rrt_amd  # noqa: F401
from radiance_ray_tracing_amd import rd, scenes
import ray_edge_cases as rec

N, SIDE, REPS, WARM = 1 << 21, 1024, 20, 3


def rays_of(dev):
    px = np.arange(SIDE * SIDE, dtype=np.uint32)
    o, d = rd.GenerateBatch(px, np.stack([np.zeros_like(px), np.zeros_like(px), px], 1))
    hits = rd.TraceBatch(dev.topAccelStruct, o, d, reference_order=True)
    ok = hits["hit"] == 1
    hp = (o + d * hits["distance"][:, None])[ok]
    rng = np.random.default_rng(1)
    hp = hp[rng.integers(0, hp.shape[0], N - o.shape[0])]
    d2 = rng.normal(size=hp.shape).astype(np.float32); d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    o2 = (hp + 1e-3 * d2).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([o, o2])), np.ascontiguousarray(np.concatenate([d, d2])), float(ok.mean())


def stat(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ray_query_bench.json")
    plt = rd.Platform.GetPlatform()
    dev = scenes.DeviceScene(scenes.CONFIGS["c2_atrium"](SIDE, SIDE, 1, 8))
    o, d, rate = rays_of(dev)
    assert o.shape[0] == N
    stock = np.zeros(N, rd.RAY_DTYPE)
    stock["origin"], stock["direction"], stock["tmin"], stock["tmax"] = o, d, 0.001, 1000.0
    mixed = stock.copy()
    iv = np.array([(a, b) for _, a, b in rec.INTERVALS], np.float32)
    mixed["tmin"], mixed["tmax"] = iv[np.arange(N) % len(iv), 0], iv[np.arange(N) % len(iv), 1]
    bS, bM, bH = (rd.CreateBuffer(plt, N * 32) for _ in range(3))
    rd.WriteBuffer(plt, bS, N * 32, stock)
    rd.WriteBuffer(plt, bM, N * 32, mixed)
    tl = dev.topAccelStruct
    res = {"device": rd.Platform.device_name(), "scene": "c2_atrium (Sponza-class)", "rays": N,
           "rays_note": "2^20 primary rays (%dx%d) + 2^20 scattered from their hit points; %.3f of the primaries hit" % (SIDE, SIDE, rate),
           "reps": REPS, "warmup_rounds": WARM, "unit": "ms"}
    for kind in (1, 2):
        legs = {"a_trace_batch": lambda: rd.TraceBatch(tl, o, d, 0.001, 1000.0, kind),
                "b_query_stock": lambda: rd.QueryRays(tl, bS, N, kind, bH),
                "c_query_mixed": lambda: rd.QueryRays(tl, bM, N, kind, bH)}
        kern = {k: [] for k in legs}; wall = {k: [] for k in legs}; nhit = {}
        for r in range(WARM + REPS):
            for name, call in legs.items():
                t0 = time.perf_counter()
                ret = call()
                t1 = time.perf_counter()
                if r >= WARM:
                    kern[name].append(rd.GetTraceStats().ms_extend); wall[name].append((t1 - t0) * 1e3)
                elif r == 0:
                    nhit[name] = int(ret["hit"].sum()) if name[0] == "a" else int(rd.ReadBuffer(plt, bH, N * 32).view(rd.RAY_HIT_DTYPE)["hit"].sum())
                ret = None          # (released here: freeing leg a's 235 MB of host records must not fall into the next leg's wall time)
        assert nhit["a_trace_batch"] == nhit["b_query_stock"], nhit
        k = {"hits": nhit}
        for name in legs:
            k[name] = {"kernel_ms": stat(kern[name]), "wall_ms": stat(wall[name])}
        a, b, c = (k[n]["kernel_ms"] for n in legs)
        k["a_kernel_spread_ms"] = round(a["max"] - a["min"], 4)
        k["b_over_a_kernel"] = round(b["median"] / a["median"], 4)
        k["b_minus_a_kernel_ms"] = round(b["median"] - a["median"], 4)
        k["b_slower_than_a_by_more_than_the_spread"] = bool(b["median"] - a["median"] > a["max"] - a["min"])
        k["c_over_b_kernel"] = round(c["median"] / b["median"], 4)
        k["b_over_a_wall"] = round(k["b_query_stock"]["wall_ms"]["median"] / k["a_trace_batch"]["wall_ms"]["median"], 5)
        k["grays_per_s"] = {n: round(N / k[n]["kernel_ms"]["median"] * 1e-6, 3) for n in legs}
        res["closest_hit" if kind == 1 else "any_hit"] = k
        print("kind %d: kernel ms a %.3f (spread %.3f)  b %.3f  c %.3f | wall ms a %.1f  b %.3f  c %.3f | hits %r"
              % (kind, a["median"], k["a_kernel_spread_ms"], b["median"], c["median"], k["a_trace_batch"]["wall_ms"]["median"],
                 k["b_query_stock"]["wall_ms"]["median"], k["c_query_mixed"]["wall_ms"]["median"], nhit), flush=True)
    print(json.dumps(res))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

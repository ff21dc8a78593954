#!/usr/bin/env python3
"""raygen_bench.py -- rd.GenerateRays / rd.Accumulate (rdx_generate_rays, rdx_accumulate) beside the frame path's own generate and
accumulate stages, on the Sponza-class scene at 2048 x 1024 = 2^21 pixels, one ray and one sample per pixel.
After a warm-up these legs ALTERNATE in this one process, REPS times each:
  f   rd.TraceRays of that frame (1 sample, depth 1) with profiling on: its k_generate / k_accumulate launches over 2^21 paths,
      rdx_get_trace_stats().ms_generate / .ms_accumulate        -- yardstick: the frame path, whose kernels this tool does not touch
  g   rd.GenerateRays, 2^21 rays with keys (32 + 16 bytes written per ray; k_generate writes 64)
  g0  the same without keys
  a   rd.Accumulate, 2^21 samples of frame 1 into the scene's imageScratch and image (the traffic of k_accumulate with one sample)
  a0  the same without the image
Per leg: kernel time (HIP events around the launches: .ms_generate / .ms_accumulate of the call; for g that includes the one
thread that prepares the camera), median / min / max.  Once, outside the rounds: the wall time of rd.GenerateBatch for the same
rays (host arrays in and out).  Written out: g / f.generate and a / f.accumulate with the 1.25x margin for launch noise on kernels
this short, and GB/s of g and a over the bytes they stream.  GPU only.
    python tools/raygen_bench.py [out.json]          (default: profiles/raygen_bench.json)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np
import rrt_amd  # noqa: F401
from radiance_ray_tracing_amd import rd, scenes
from ray_query_bench import stat

W, H, REPS, WARM, MARGIN = 2048, 1024, 20, 3, 1.25
N = W * H
GENERATE_BYTES, ACCUMULATE_BYTES = 32 + 16, 16 + 16 + 16 + 4     # ray + key out | colour in, imageScratch in and out, RGBA8 out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "raygen_bench.json")
    plt = rd.Platform.GetPlatform()
    dev = scenes.DeviceScene(scenes.CONFIGS["c2_atrium"](W, H, 1, 1))
    assert dev.width * dev.height == N == 1 << 21
    cam, scratch, image = dev.frame_buffers()
    dev.set_rtprop(totalSamples=1, batchSize=1, depth=1)          # every frame below is sample 1: the running-mean branch
    dev.clear_scratch()
    rd.SetProfiling(True)
    bR, bK, bC = rd.CreateBuffer(plt, N * 32), rd.CreateBuffer(plt, N * 16), rd.CreateBuffer(plt, N * 16)
    rd.WriteBuffer(plt, bC, N * 16, np.random.default_rng(1).uniform(0, 2, (N, 4)).astype(np.float32))
    legs = {"f_trace_rays": lambda: rd.TraceRays(plt, 0, 0, 0, W, H),
            "g_generate": lambda: rd.GenerateRays(cam, N, 1, 1, rays=bR, keys=bK),
            "g0_generate_no_keys": lambda: rd.GenerateRays(cam, N, 1, 1, rays=bR, keys=None),
            "a_accumulate": lambda: rd.Accumulate(bC, N, 1, scratch, image),
            "a0_accumulate_no_image": lambda: rd.Accumulate(bC, N, 1, scratch)}
    kern = {"f_generate": [], "f_accumulate": [], **{k: [] for k in legs if k[0] != "f"}}
    for r in range(WARM + REPS):
        for name, call in legs.items():
            call()
            st = rd.GetTraceStats()
            if r < WARM:
                continue
            if name[0] == "f":
                kern["f_generate"].append(st.ms_generate); kern["f_accumulate"].append(st.ms_accumulate)
            else:
                kern[name].append(st.ms_generate if name[0] == "g" else st.ms_accumulate)
    rd.SetProfiling(False)
    # the test seam on the same rays: host arrays in, host arrays out
    px = np.arange(N, dtype=np.uint32)
    rnd = np.stack([np.ones_like(px), np.ones_like(px), px], 1)
    wall = []
    for r in range(3):
        t0 = time.perf_counter()
        o, d = rd.GenerateBatch(px, rnd)
        wall.append((time.perf_counter() - t0) * 1e3)
    rays = rd.ReadBuffer(plt, bR, N * 32).view(rd.RAY_DTYPE)
    assert np.array_equal(rays["origin"].view(np.uint32), o.view(np.uint32)) and np.array_equal(rays["direction"].view(np.uint32), d.view(np.uint32))
    k = {name: stat(v) for name, v in kern.items()}
    g, a, fg, fa = (k[n]["median"] for n in ("g_generate", "a_accumulate", "f_generate", "f_accumulate"))
    assert fg > 0 and fa > 0, "the frame ran without its staged generate / accumulate launches (option \"pipeline\")"
    res = {"device": rd.Platform.device_name(), "scene": "c2_atrium (Sponza-class)", "rays": N, "frame": "%d x %d, 1 sample, depth 1" % (W, H),
           "reps": REPS, "warmup_rounds": WARM, "unit": "ms", "kernel_ms": k,
           "frame_path_spread_ms": {"generate": round(k["f_generate"]["max"] - k["f_generate"]["min"], 4),
                                    "accumulate": round(k["f_accumulate"]["max"] - k["f_accumulate"]["min"], 4)},
           "generate_over_k_generate": round(g / fg, 4), "accumulate_over_k_accumulate": round(a / fa, 4), "margin": MARGIN,
           "generate_within_margin": bool(g <= MARGIN * fg), "accumulate_within_margin": bool(a <= MARGIN * fa),
           "no_keys_over_generate": round(k["g0_generate_no_keys"]["median"] / g, 4),
           "no_image_over_accumulate": round(k["a0_accumulate_no_image"]["median"] / a, 4),
           "generate_bytes_per_ray": GENERATE_BYTES, "accumulate_bytes_per_sample": ACCUMULATE_BYTES,
           "generate_streamed_GBps": round(N * GENERATE_BYTES / g * 1e-6, 1), "accumulate_streamed_GBps": round(N * ACCUMULATE_BYTES / a * 1e-6, 1),
           "generate_batch_wall_ms": stat(wall), "generate_batch_wall_over_generate_kernel": round(float(np.median(wall)) / g, 1)}
    print("kernel ms: generate %.4f (frame path %.4f, ratio %.2f)  without keys %.4f | accumulate %.4f (frame path %.4f, ratio %.2f)  without image %.4f | GenerateBatch wall %.1f ms"
          % (g, fg, g / fg, k["g0_generate_no_keys"]["median"], a, fa, a / fa, k["a0_accumulate_no_image"]["median"], float(np.median(wall))), flush=True)
    print(json.dumps(res))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""temporal_bench.py -- temporal.TemporalAccumulate (rdx_temporal_accumulate) beside rd.TracePaths, rd.Accumulate and denoise.Denoise
at 5 passes for the same frame, on the Sponza-class scene: the 1920 x 1080 camera rays of sample 0 (rd.GenerateRays), depth 8, one
sample per pixel; guides from rd.ResolveHits / rd.ResolveMaterials on the primary hits; position_tolerance and sigma_position 1 %
of the scene's diagonal, the other settings the defaults.  After 3 warm-up rounds these legs ALTERNATE in this one process, 20
rounds:
  trace          rd.TracePaths: ms_total
  accumulate     rd.Accumulate with the RGBA8 image: ms_accumulate
  denoise        denoise.Denoise with 5 passes, RGBA8 image written: ms_accumulate
  still_v4       TemporalAccumulate as shipped (variance_min_history 4) on a history of length 8 under a still view (previous_view
                 absent), RGBA8 image written: ms_accumulate of both launches; every lane of the variance kernel leaves at once
  still_v0       the same with variance_min_history 0: the reproject kernel alone
  pan_v4, pan_v0 the same under a previous view whose eye is 3.3 pixels to the right: all four bilinear taps of a pixel carry weight, and
                 the pixels that lose their history start again, so that the window runs for them
  young_v4       on a history of length 1, so that N' = 2 < 4 and the 7 x 7 window runs for every valid pixel
  young_v0       the same with variance_min_history 0: young_v4 - young_v0 is the variance kernel at full load, still_v4 - still_v0 idle
Medians, min / max and spread (max - min) per leg.  The reproject kernel must move 196 bytes per pixel under a still view (colour 16,
material record 32 of 64, surface record 16 of 64, one history tap 64, history out 64, image 4) and requests at most 452 (four
taps, previous_positions): both rates are reported as a share of the 8 TB/s an MI355X's HBM delivers at most.  The bytes that reach
HBM, the cache hit rates and the issue rate are not measured here (no counters are collected).  With a second argument, the JSON
line bench.py printed is recorded beside the figure of the commit before this one.  No test gates on a time.  GPU only.
    python tools/temporal_bench.py [out.json [bench.json]]          (default: profiles/temporal_bench.json)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
torch.zeros(1, device="cuda").cpu()          # torch initialises the GPU first
import rrt_amd  # noqa: F401
from radiance_ray_tracing_amd import denoise, rd, scenes, temporal
from ray_query_bench import stat

W, H, DEPTH, REPS, WARM, PASSES = 1920, 1080, 8, 20, 3, 5
N = W * H
HBM_PEAK = 8.0e12
PAN_PIXELS = 3.3
PARENT_FRAME_MS = 20.99          # bench.py, the commit before this one (its message)
MUST, MOST = 196, 452            # bytes per pixel: a still view's minimum, and what four taps and previous_positions request


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "temporal_bench.json")
    plt = rd.Platform.GetPlatform()
    dev = scenes.DeviceScene(scenes.CONFIGS["c2_atrium"](W, H, 1, DEPTH))
    cam, scratch, image = dev.frame_buffers()
    tlas, sb = dev.topAccelStruct, dev.shading_buffers()
    s = rd.DebugAccelLayout(rd.ReadBuffer(plt, tlas, tlas.size).tobytes())[0]
    diagonal = float(np.linalg.norm(np.array(s["sceneHi"], np.float64) - np.array(s["sceneLo"], np.float64)))
    bR, bK = rd.GenerateRays(cam, N, 0, 0)
    bH = rd.QueryRays(tlas, bR, N, rd.QUERY_CLOSEST)
    bS, _ = rd.ResolveHits(tlas, bR, bH, N, dev.surface_buffers())
    bM, _ = rd.ResolveMaterials(tlas, bR, bH, N, sb)
    bC, bO, bW = rd.CreateBuffer(plt, 16 * N), rd.CreateBuffer(plt, 16 * N), rd.CreateBuffer(plt, denoise.WorkSize(W, H))
    rd.TracePaths(tlas, bR, bK, N, DEPTH, sb, radiance=bC)
    dst = denoise.DenoiseSettings(passes=PASSES, sigma_position=0.01 * diagonal)
    st = {v: temporal.TemporalSettings(position_tolerance=0.01 * diagonal, variance_min_history=v) for v in (0, 4)}
    view = temporal.CameraView(cam)
    rec = rd.ReadBuffer(plt, view, 64).view(temporal.VIEW_DTYPE).copy()
    # the previous eye PAN_PIXELS to the right at the depth of the scene's middle: one pixel there is depth / (width * kx) world units
    depth = 0.5 * diagonal
    moved = rec.copy()
    moved["eye"][0] = rec["eye"][0] + rec["right"][0] * np.float32(PAN_PIXELS * depth / (W * float(rec["kx"][0])))
    pview = rd.CreateBuffer(plt, 64)
    rd.WriteBuffer(plt, pview, 64, moved)
    size = temporal.HistorySize(W, H)
    young, old, out = rd.CreateBuffer(plt, size), rd.CreateBuffer(plt, size), rd.CreateBuffer(plt, size)
    temporal.TemporalAccumulate(bC, bM, bS, view, W, H, st[4], None, young)
    a, b = out, old
    temporal.TemporalAccumulate(bC, bM, bS, view, W, H, st[4], young, b)
    for _ in range(6):               # lengths 3 .. 8, ending in `old`
        a, b = b, a
        temporal.TemporalAccumulate(bC, bM, bS, view, W, H, st[4], a, b)
    assert b is old
    lengths = rd.ReadBuffer(plt, old, 16 * N, offset=16 * N).view(np.uint32).reshape(N, 4)[:, 3]
    valid = rd.ReadBuffer(plt, old, 16 * N, offset=48 * N).view(np.uint32).reshape(N, 4)[:, 3] == 1

    def acc(history, v, previous):
        temporal.TemporalAccumulate(bC, bM, bS, view, W, H, st[v], history, out, previous, None, image)
        return rd.GetTraceStats().ms_accumulate

    def trace():
        rd.TracePaths(tlas, bR, bK, N, DEPTH, sb, radiance=bC)
        return rd.GetTraceStats().ms_total

    def accumulate():
        rd.Accumulate(bC, N, 0, scratch, image)
        return rd.GetTraceStats().ms_accumulate

    def den():
        denoise.Denoise(bC, bM, bS, W, H, dst, out=bO, image=image, work=bW)
        return rd.GetTraceStats().ms_accumulate
    legs = {"trace": trace, "accumulate": accumulate, "denoise": den,
            "still_v4": lambda: acc(old, 4, None), "still_v0": lambda: acc(old, 0, None), "pan_v4": lambda: acc(old, 4, pview), "pan_v0": lambda: acc(old, 0, pview),
            "young_v4": lambda: acc(young, 4, None), "young_v0": lambda: acc(young, 0, None)}
    rd.SetProfiling(True)
    ms = {name: [] for name in legs}
    kept = {}
    for r in range(WARM + REPS):
        for name, call in legs.items():
            v = call()
            if r >= WARM:
                ms[name].append(v)
            if r == 0 and name in ("still_v4", "pan_v4", "young_v4"):
                n_out = rd.ReadBuffer(plt, out, 16 * N, offset=16 * N).view(np.uint32).reshape(N, 4)[:, 3]
                kept[name] = {"pixels_with_history": int((n_out[valid] >= 2).sum()), "pixels_in_the_window_kernel": int((valid & (n_out < 4)).sum())}
    rd.SetProfiling(False)
    k = {name: stat(v) for name, v in ms.items()}
    for name, v in ms.items():
        k[name]["spread"] = round(float(np.max(v) - np.min(v)), 4)
    med = {name: k[name]["median"] for name in k}
    rate = {name: {"GB_per_s_at_%d_B_per_pixel" % MUST: round(MUST * N / (med[name] * 1e-3) / 1e9, 1), "share_of_hbm_peak_at_%d_B" % MUST: round(MUST * N / (med[name] * 1e-3) / HBM_PEAK, 4),
                   "share_of_hbm_peak_at_%d_B" % MOST: round(MOST * N / (med[name] * 1e-3) / HBM_PEAK, 4)} for name in ("still_v0", "pan_v0", "young_v0")}
    res = {"device": rd.Platform.device_name(), "scene": "c2_atrium (Sponza-class)", "frame": "%d x %d, sample 0, 1 spp, depth %d" % (W, H, DEPTH), "pixels": N,
           "valid_pixels": int(valid.sum()), "history_lengths_of_the_old_history": {str(v): int(c) for v, c in enumerate(np.bincount(lengths[valid])) if c},
           "settings": repr(st[4]), "denoise_settings": repr(dst), "pan_pixels_at_mid_depth": PAN_PIXELS, "reps": REPS, "warmup_rounds": WARM, "unit": "ms", "ms": k,
           "reproject_kernel_ms": {"still": med["still_v0"], "pan": med["pan_v0"], "young": med["young_v0"]},
           "variance_kernel_ms": {"idle (still_v4 - still_v0)": round(med["still_v4"] - med["still_v0"], 4), "the pixels that lost their history in the pan (pan_v4 - pan_v0)": round(med["pan_v4"] - med["pan_v0"], 4),
                                  "every pixel (young_v4 - young_v0)": round(med["young_v4"] - med["young_v0"], 4)},
           "what_the_legs_did": kept, "temporal_over_trace": round(med["still_v4"] / med["trace"], 4), "temporal_over_denoise": round(med["still_v4"] / med["denoise"], 4),
           "temporal_over_accumulate": round(med["still_v4"] / med["accumulate"], 2), "bytes_per_pixel_a_still_view_must_move": MUST, "bytes_per_pixel_requested_at_most": MOST,
           "hbm_bytes_measured": None, "cache_hit_rates_measured": None, "issue_rate_measured": None, "rate_of_the_reproject_kernel": rate, "history_bytes": size}
    if len(sys.argv) > 2:
        with open(sys.argv[2]) as f:
            line = [ln for ln in f.read().splitlines() if ln.startswith("{")][-1]
        res["bench_py"] = {"this_commit": json.loads(line), "parent_frame_ms": PARENT_FRAME_MS}
    print("ms: TracePaths %.3f | Accumulate %.3f | Denoise 5 passes %.3f | TemporalAccumulate still %.3f (reproject alone %.3f), pan %.3f (%.3f), young %.3f (%.3f)"
          % (med["trace"], med["accumulate"], med["denoise"], med["still_v4"], med["still_v0"], med["pan_v4"], med["pan_v0"], med["young_v4"], med["young_v0"]), flush=True)
    print(json.dumps(res))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""denoise_bench.py -- denoise.Denoise (rdx_denoise) beside rd.TracePaths and rd.Accumulate for the same frame, on the Sponza-class
scene: the 1920 x 1080 camera rays of sample 0 (rd.GenerateRays), depth 8, one sample per pixel; guides from rd.ResolveHits /
rd.ResolveMaterials on the primary hits; sigma_position 1 % of the scene's diagonal, the other settings the defaults.  After 3
warm-up rounds these legs ALTERNATE in this one process, 20 rounds:
  trace        rd.TracePaths: ms_total
  accumulate   rd.Accumulate with the RGBA8 image: ms_accumulate
  s5           denoise.Denoise with 5 passes as the library ships it (steps 1 and 2 from the LDS tile), RGBA8 image written:
               ms_accumulate (prepare, the passes, the finish)
  p0 .. p5     0 .. 5 passes with every pass in the direct form
  t1, t2       1 and 2 passes with every step the tiled form has (1; 1 and 2) taken from the LDS tile
  d2           2 passes, pass 0 direct and pass 1 tiled
Medians, min / max and spread (max - min) per leg.  The time of a direct pass j is p(j+1) - p(j).  Direct against tiled is one
call against the same call with one pass in the other form: p1 against t1 for step 1, p2 against d2 for step 2; the tiled form
is faster "by more than the spread of both" when the difference of the medians exceeds the sum of the two spreads (then the two
ranges of 20 rounds do not touch).  A pass must move 64 bytes per pixel (iterate in, guide in, iterate out); its
25 taps request 25 x 48 bytes per pixel from the caches: the rate at 64 bytes per pixel is reported as a share of the 8 TB/s an
MI355X's HBM delivers at most.  The bytes that reach HBM are not measured here (no counters are collected).  With a second
argument, the JSON line bench.py printed is recorded beside the figure of the commit before this one.  No test gates on a time.
GPU only.
    python tools/denoise_bench.py [out.json [bench.json]]          (default: profiles/denoise_bench.json)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
torch.zeros(1, device="cuda").cpu()          # torch initialises the GPU first
import rrt_amd  # noqa: F401
from radiance_ray_tracing_amd import _lib, denoise, rd, scenes
from ray_query_bench import stat

W, H, DEPTH, REPS, WARM, PASSES = 1920, 1080, 8, 20, 3, 5
N = W * H
HBM_PEAK = 8.0e12
SHIPPED = 3                      # rdx_debug_denoise_tiled: the library's default, steps 1 and 2 tiled
PARENT_FRAME_MS = 20.99          # bench.py, the commit before this one (its message)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "denoise_bench.json")
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
    settings = {k: denoise.DenoiseSettings(passes=k, sigma_position=0.01 * diagonal) for k in range(PASSES + 1)}
    L = _lib.lib()

    def den(passes, tiled):
        L.rdx_debug_denoise_tiled(tiled)
        denoise.Denoise(bC, bM, bS, W, H, settings[passes], out=bO, image=image, work=bW)
        L.rdx_debug_denoise_tiled(SHIPPED)
        return rd.GetTraceStats().ms_accumulate

    def trace():
        rd.TracePaths(tlas, bR, bK, N, DEPTH, sb, radiance=bC)
        return rd.GetTraceStats().ms_total

    def accumulate():
        rd.Accumulate(bC, N, 0, scratch, image)
        return rd.GetTraceStats().ms_accumulate
    legs = {"trace": trace, "accumulate": accumulate, "s5": lambda: den(PASSES, SHIPPED)}
    legs.update({"p%d" % k: (lambda k=k: den(k, 0)) for k in range(PASSES + 1)})
    legs.update({"t1": lambda: den(1, 1), "t2": lambda: den(2, 3), "d2": lambda: den(2, 2)})
    rd.SetProfiling(True)
    ms = {name: [] for name in legs}
    for r in range(WARM + REPS):
        for name, call in legs.items():
            v = call()
            if r >= WARM:
                ms[name].append(v)
    rd.SetProfiling(False)
    # both forms give the same bits on this frame
    den(2, 0)
    direct = rd.ReadBuffer(plt, bO, 16 * N).copy()
    den(2, 3)
    forms_agree = bool(np.array_equal(direct, rd.ReadBuffer(plt, bO, 16 * N)))
    assert forms_agree
    k = {name: stat(v) for name, v in ms.items()}
    for name, v in ms.items():
        k[name]["spread"] = round(float(np.max(v) - np.min(v)), 4)
    med = {name: k[name]["median"] for name in k}
    per_pass = {"step %d" % (1 << j): round(med["p%d" % (j + 1)] - med["p%d" % j], 4) for j in range(PASSES)}
    must = 64 * N
    rate = {name: {"GB_per_s_at_64_B_per_pixel": round(must / (t * 1e-3) / 1e9, 1), "share_of_hbm_peak": round(must / (t * 1e-3) / HBM_PEAK, 4)}
            for name, t in per_pass.items() if t > 0}
    forms = {"step 1": {"legs": "p1 against t1", "direct": med["p1"], "tiled": med["t1"], "spread_direct": k["p1"]["spread"], "spread_tiled": k["t1"]["spread"]},
             "step 2": {"legs": "p2 against d2", "direct": med["p2"], "tiled": med["d2"], "spread_direct": k["p2"]["spread"], "spread_tiled": k["d2"]["spread"]}}
    for f in forms.values():
        f["tiled_faster_by"] = round(f["direct"] - f["tiled"], 4)
        f["tiled_faster_by_more_than_both_spreads"] = bool(f["direct"] - f["tiled"] > f["spread_direct"] + f["spread_tiled"])
    res = {"device": rd.Platform.device_name(), "scene": "c2_atrium (Sponza-class)", "frame": "%d x %d, sample 0, 1 spp, depth %d" % (W, H, DEPTH), "pixels": N,
           "settings": repr(settings[PASSES]), "reps": REPS, "warmup_rounds": WARM, "unit": "ms", "ms": k, "ms_per_direct_pass": per_pass,
           "prepare_and_finish_ms": med["p0"], "denoise_over_trace": round(med["s5"] / med["trace"], 4),
           "denoise_over_accumulate": round(med["s5"] / med["accumulate"], 2), "direct_against_tiled": forms, "forms_agree_bit_for_bit": forms_agree,
           "bytes_per_pixel_a_pass_must_move": 64, "bytes_per_pixel_the_taps_request": 25 * 48 + 48 + 16, "hbm_bytes_measured": None, "rate_per_direct_pass": rate,
           "work_bytes": denoise.WorkSize(W, H)}
    if len(sys.argv) > 2:
        with open(sys.argv[2]) as f:
            line = [ln for ln in f.read().splitlines() if ln.startswith("{")][-1]
        res["bench_py"] = {"this_commit": json.loads(line), "parent_frame_ms": PARENT_FRAME_MS}
    print("ms: TracePaths %.3f | Accumulate %.3f | Denoise 5 passes %.3f as shipped, %.3f all direct (prepare + finish %.3f, per direct pass %s) | direct against tiled %s"
          % (med["trace"], med["accumulate"], med["s5"], med["p%d" % PASSES], med["p0"], per_pass, forms), flush=True)
    print(json.dumps(res))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

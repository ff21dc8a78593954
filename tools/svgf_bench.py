#!/usr/bin/env python3
"""svgf_bench.py -- svgf.Filter (rdx_svgf_filter) beside denoise.Denoise and temporal.TemporalAccumulate, on the Sponza-class scene:
1920 x 1080, one sample per pixel, depth 8; four samples folded into a history under a still view (so that plane 1 carries the
temporal variance), guides from rd.ResolveHits / rd.ResolveMaterials on the primary hits of the last one; sigma_position 1 % of the
scene's diagonal, the other settings the defaults.  After 3 warm-up rounds these legs ALTERNATE in this one process, 20 rounds:
  temporal     temporal.TemporalAccumulate of the last sample onto the history before it, still view: ms_accumulate
  den5         denoise.Denoise with 5 passes on plane 0, as the library ships it (steps 1 and 2 from the LDS tile)
  den5d        the same with every pass in the direct form
  den0         denoise.Denoise with no pass: its prepare fused with its finish
  s5           svgf.Filter with 5 passes on planes 0 and 1 as the library ships it, variance_out and the feedback after pass 1 written
  p0 .. p5     0 .. 5 passes with every pass in the direct form, out alone
  n5           p5 with sigma_luminance = 0: no prefilter, no luminance weight -- the passes of rdx_denoise plus the variance sum
  t1           1 pass from the LDS tile
  d2           2 passes, pass 0 direct and pass 1 tiled
Medians, min / max and spread (max - min) per leg.  The time of a direct pass j is p(j+1) - p(j); the w * w sum of a pass is
((n5 - p0) - (den5d - den0)) / 5: the two calls' passes without their prepare and finish.  Direct against tiled is one call
against the same call with one pass in the other form: p1 against t1 for step 1, p2 against d2 for step 2; the tiled form is faster
"by more than the spread of both" when the difference of the medians exceeds the sum of the two spreads.  The bytes that reach HBM
are not measured here (no counters are collected).  With a second argument, the JSON line bench.py printed is recorded beside the
figure of the commit before this one.  No test gates on a time.  GPU only.
    python tools/svgf_bench.py [out.json [bench.json]]          (default: profiles/svgf_bench.json)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
torch.zeros(1, device="cuda").cpu()          # torch initialises the GPU first
import rrt_amd  # noqa: F401
from radiance_ray_tracing_amd import _lib, denoise, rd, scenes, svgf, temporal
from ray_query_bench import stat

W, H, DEPTH, REPS, WARM, PASSES, FRAMES = 1920, 1080, 8, 20, 3, 5, 4
N = W * H
SHIPPED = 3                      # rdx_debug_svgf_tiled: the library's default
DENOISE_SHIPPED = 3              # rdx_debug_denoise_tiled: the library's default
PARENT_FRAME_MS = 20.99          # bench.py, the commit before this one (its message)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "svgf_bench.json")
    plt = rd.Platform.GetPlatform()
    dev = scenes.DeviceScene(scenes.CONFIGS["c2_atrium"](W, H, 1, DEPTH))
    cam, scratch, image = dev.frame_buffers()
    tlas, sb = dev.topAccelStruct, dev.shading_buffers()
    s = rd.DebugAccelLayout(rd.ReadBuffer(plt, tlas, tlas.size).tobytes())[0]
    diagonal = float(np.linalg.norm(np.array(s["sceneHi"], np.float64) - np.array(s["sceneLo"], np.float64)))
    view = temporal.CameraView(cam)
    tset = temporal.TemporalSettings(position_tolerance=0.01 * diagonal)
    hb = [rd.CreateBuffer(plt, temporal.HistorySize(W, H)) for _ in range(3)]
    bR, bK, bC = rd.CreateBuffer(plt, 32 * N), rd.CreateBuffer(plt, 16 * N), rd.CreateBuffer(plt, 16 * N)
    for f in range(FRAMES):
        rd.GenerateRays(cam, N, f, f, rays=bR, keys=bK)
        bH = rd.QueryRays(tlas, bR, N, rd.QUERY_CLOSEST)
        bS, _ = rd.ResolveHits(tlas, bR, bH, N, dev.surface_buffers())
        bM, _ = rd.ResolveMaterials(tlas, bR, bH, N, sb)
        rd.TracePaths(tlas, bR, bK, N, DEPTH, sb, radiance=bC)
        temporal.TemporalAccumulate(bC, bM, bS, view, W, H, tset, hb[(f + 1) % 2] if f else None, hb[f % 2])
    hist, before = hb[(FRAMES - 1) % 2], hb[FRAMES % 2]
    bO, bV, bF, bW = rd.CreateBuffer(plt, 16 * N), rd.CreateBuffer(plt, 4 * N), rd.CreateBuffer(plt, 16 * N), rd.CreateBuffer(plt, svgf.WorkSize(W, H))
    sigma = 0.01 * diagonal
    plain = {k: svgf.FilterSettings(passes=k, sigma_position=sigma) for k in range(PASSES + 1)}
    shipped = svgf.FilterSettings(passes=PASSES, sigma_position=sigma, feedback_pass=1)
    nolum = svgf.FilterSettings(passes=PASSES, sigma_position=sigma, sigma_luminance=0.0)
    dset = denoise.DenoiseSettings(passes=PASSES, sigma_position=sigma)
    dset0 = denoise.DenoiseSettings(passes=0, sigma_position=sigma)
    L = _lib.lib()

    def flt(settings, tiled, full=False):
        L.rdx_debug_svgf_tiled(tiled)
        svgf.Filter(hist, hist, bM, bS, W, H, settings, out=bO, variance_out=bV if full else None, feedback=bF if settings.feedback_pass else None, work=bW,
                    moments_offset=16 * N)
        L.rdx_debug_svgf_tiled(SHIPPED)
        return rd.GetTraceStats().ms_accumulate

    def den(tiled, settings=None):
        L.rdx_debug_denoise_tiled(tiled)
        denoise.Denoise(hist, bM, bS, W, H, settings or dset, out=bO, work=bW)
        L.rdx_debug_denoise_tiled(DENOISE_SHIPPED)
        return rd.GetTraceStats().ms_accumulate

    def accumulate():
        temporal.TemporalAccumulate(bC, bM, bS, view, W, H, tset, before, hb[2])
        return rd.GetTraceStats().ms_accumulate
    legs = {"temporal": accumulate, "den5": lambda: den(DENOISE_SHIPPED), "den5d": lambda: den(0), "den0": lambda: den(0, dset0), "s5": lambda: flt(shipped, SHIPPED, True)}
    legs.update({"p%d" % k: (lambda k=k: flt(plain[k], 0)) for k in range(PASSES + 1)})
    legs.update({"n5": lambda: flt(nolum, 0), "t1": lambda: flt(plain[1], 1), "d2": lambda: flt(plain[2], 2)})
    rd.SetProfiling(True)
    ms = {name: [] for name in legs}
    for r in range(WARM + REPS):
        for name, call in legs.items():
            v = call()
            if r >= WARM:
                ms[name].append(v)
    rd.SetProfiling(False)
    # both forms give the same bits on this frame
    flt(plain[2], 0)
    direct = rd.ReadBuffer(plt, bO, 16 * N).copy()
    flt(plain[2], 3)
    forms_agree = bool(np.array_equal(direct, rd.ReadBuffer(plt, bO, 16 * N)))
    assert forms_agree
    k = {name: stat(v) for name, v in ms.items()}
    for name, v in ms.items():
        k[name]["spread"] = round(float(np.max(v) - np.min(v)), 4)
    med = {name: k[name]["median"] for name in k}
    per_pass = {"step %d" % (1 << j): round(med["p%d" % (j + 1)] - med["p%d" % j], 4) for j in range(PASSES)}
    forms = {"step 1": {"legs": "p1 against t1", "direct": med["p1"], "tiled": med["t1"], "spread_direct": k["p1"]["spread"], "spread_tiled": k["t1"]["spread"]},
             "step 2": {"legs": "p2 against d2", "direct": med["p2"], "tiled": med["d2"], "spread_direct": k["p2"]["spread"], "spread_tiled": k["d2"]["spread"]}}
    for f in forms.values():
        f["tiled_faster_by"] = round(f["direct"] - f["tiled"], 4)
        f["tiled_faster_by_more_than_both_spreads"] = bool(f["direct"] - f["tiled"] > f["spread_direct"] + f["spread_tiled"])
    res = {"device": rd.Platform.device_name(), "scene": "c2_atrium (Sponza-class)", "frame": "%d x %d, 1 spp, depth %d, a history of %d samples, still view" % (W, H, DEPTH, FRAMES),
           "pixels": N, "settings": repr(shipped), "shipped_tiled_mask": SHIPPED, "reps": REPS, "warmup_rounds": WARM, "unit": "ms", "ms": k, "ms_per_direct_pass": per_pass,
           "prepare_and_finish_ms": med["p0"], "filter_over_denoise": round(med["s5"] / med["den5"], 4), "all_direct_over_denoise_all_direct": round(med["p5"] / med["den5d"], 4),
           "luminance_term_and_prefilter_ms_per_pass": round((med["p5"] - med["n5"]) / PASSES, 4), "variance_sum_ms_per_pass": round(((med["n5"] - med["p0"]) - (med["den5d"] - med["den0"])) / PASSES, 4),
           "prepare_and_finish_over_denoises_ms": round(med["p0"] - med["den0"], 4),
           "direct_against_tiled": forms, "forms_agree_bit_for_bit": forms_agree, "hbm_bytes_measured": None, "work_bytes": svgf.WorkSize(W, H)}
    if len(sys.argv) > 2:
        with open(sys.argv[2]) as f:
            line = [ln for ln in f.read().splitlines() if ln.startswith("{")][-1]
        res["bench_py"] = {"this_commit": json.loads(line), "parent_frame_ms": PARENT_FRAME_MS}
    print("ms: TemporalAccumulate %.3f | Denoise 5 passes %.3f shipped, %.3f direct | svgf.Filter 5 passes %.3f shipped, %.3f direct, %.3f direct without the luminance term "
          "(prepare + finish %.3f, per direct pass %s) | direct against tiled %s"
          % (med["temporal"], med["den5"], med["den5d"], med["s5"], med["p5"], med["n5"], med["p0"], per_pass, forms), flush=True)
    print(json.dumps(res))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

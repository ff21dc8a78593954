#!/usr/bin/env python3
"""user_texture_bench.py -- what a texture read costs.  At 1920x1080 on the Cornell-class scene with texture indices on every
material and a 48x32x3 RGBA8 image array bound (repeat, linear):
  * the stock pipeline with option "textures" 0 and 1 (depth 8, 1 spp);
  * the user stage fixture tests/golden/user_texture_stages.cl with and without its read_imageui (user_stages 2, depth 1, 1 spp);
  * the VGPR count and scratch (private segment) of both stage kernels, from the compile-only seam.
Median of 5 frames after a warm-up frame, ms/frame from the library's own events.  GPU only.
    python tools/user_texture_bench.py [out.json]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import rrt_amd  # noqa: F401
from radiance_ray_tracing_amd import _lib, rd, scenes
import user_texture_ref as tr

W, H, FRAMES = 1920, 1080, 5


def textured(depth):
    s = scenes.c1_cornell(W, H, spp=1, depth=depth, sphere_subdiv=5)
    for k, m in enumerate(s.materials):
        m["albedoTexIdx"] = k % 3
        m["roughnessTexIdx"] = (k + 1) % 3
    return s


def median_ms(dev, ds):
    rd.BindPipeline(dev.plt, dev.pipeline)
    rd.BindDescriptorSet(dev.plt, ds)
    ms = []
    for f in range(FRAMES + 1):
        dev.set_rtprop(totalSamples=0)
        rd.TraceRays(dev.plt, 0, 0, 0, W, H)
        ms.append(rd.GetTraceStats().ms_total)
    return round(float(np.median(ms[1:])), 3)


plt = rd.Platform.GetPlatform()
tex = tr.test_image()
img = rd.CreateImageArray(plt, tex.shape[2], tex.shape[1], tex.shape[0])
for l in range(tex.shape[0]):
    rd.WriteImage(plt, img, tex.shape[2], tex.shape[1], l, tex[l])
smp = rd.CreateSampler(plt, rd.RD_ADDRESS_REPEAT, rd.RD_FILTER_LINEAR)
out = {"frame": "%dx%d, 1 spp" % (W, H), "scene": "c1_cornell, texture indices on every material, 48x32x3 RGBA8, repeat + linear"}

stock = scenes.DeviceScene(textured(8))
ds = list(stock.descSet); ds[11] = img; ds[12] = smp
for t in (0, 1):
    rd.SetOption("textures", t)
    out["stock_depth8_textures%d_ms" % t] = median_ms(stock, ds)
rd.SetOption("textures", 0)

lib = tr.jit_lib(_lib.LIB_PATH)
rd.SetShaderIncludePath("")
for read in (False, True):
    text = tr.stage_program(read=read)
    _, notes = tr.assert_no_image_code(lib, text, 1)
    r = tr.kernel_resources(notes, "rdx_stage_entry")
    rd.SetOption("user_stages", 2)
    try:
        dev = scenes.DeviceScene(textured(1), shader_text=text)
    finally:
        rd.SetOption("user_stages", 1)
    ds = list(dev.descSet); ds[11] = img; ds[12] = smp
    name = "user_stage_%s" % ("read" if read else "no_read")
    out[name + "_depth1_ms"] = median_ms(dev, ds)
    out[name + "_vgpr"] = r[".vgpr_count"]
    out[name + "_sgpr"] = r[".sgpr_count"]
    out[name + "_scratch_bytes"] = r[".private_segment_fixed_size"]
    print(name, out[name + "_depth1_ms"], r[".vgpr_count"], r[".private_segment_fixed_size"], flush=True)
print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)

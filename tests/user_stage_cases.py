"""Shared definitions of the stage-mode parity tests (tests/test_gpu_user_stage_parity.py, tests/test_user_stage_cases_cpu.py):
the variants of tests/golden/user_paths.cl, the frame settings, and the runner that renders one setting with the program's
stage functions on the wavefront pipeline ("user_stages" 2) and with the same text as the megakernel it is ("user_stages" 0).

The comparand needs no reference binary: the megakernel goes through the product's own device library, which
test_gpu_parity.py::test_user_program_traces_rays_with_the_product_library and the ray-edge suite hold to the reference bit
for bit.  Both modes compile the same function text under the same floating-point contract, so RGB of imageScratch is compared
as uint32 -- no tolerance.  Channel 3 is the megakernel's own event mask (see user_paths.cl); the coverage conditions on the
inputs are read from it, so a variant cannot pass by never reaching its branch."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F = np.float32

VARIANTS = {1: "no_query", 2: "query_some", 3: "query_steers", 4: "query_last", 5: "payload_carry", 6: "hit_false",
            7: "miss_continues", 8: "pixel_rng", 9: "reads_interface", 10: "scaled_dirs", 11: "shadow_miss_3"}
NUMBER = {v: k for k, v in VARIANTS.items()}
CROSSING = ("query_steers", "payload_carry", "hit_false", "miss_continues", "pixel_rng")     # state crosses bounces
WALKS = ("query_some", "pixel_rng")                                                          # run under every walk option
QUERYING = ("query_some", "query_steers", "payload_carry", "hit_false", "miss_continues", "pixel_rng", "reads_interface",
            "scaled_dirs", "shadow_miss_3")          # (query_last asks on the payload itself: its answers show as hit = false)

# event mask of user_paths.cl
HIT_RAN, QUERIED, ANSWER_HIT, FALSE_AT_0, FALSE_LATER, MISS_CONTINUED, LAST_DEPTH, MISS_RAN = (1 << k for k in range(8))
W, H = 96, 54
MARKER = 0.2501234                                     # what imageScratch holds before a frame (frame()); no colour of the fixture
BASE = dict(scene="c1_cornell", w=W, h=H, depth=5, batch=1, calls=(0,), debug=0, chunk=None)


def setting(**kw):
    s = dict(BASE)
    s.update(kw)
    return s


# the settings the variants of CROSSING additionally run under (the issue's list), by name
CROSSING_SETTINGS = {
    "depth0": setting(depth=0), "depth1": setting(depth=1), "depth2": setting(depth=2),
    "debug_depth4": setting(depth=4, debug=1),
    "batch3": setting(batch=3),
    "progressive_0_then_3": setting(batch=3, calls=(0, 3)),
    "two_chunks": setting(batch=3, chunk=2 * W * H),          # 3 samples x 5184 paths, 10368 per chunk: chunks of 2 + 1 samples
    "partial_group_97x55": setting(w=97, h=55),
    "edges_inst": setting(scene="edges_inst"),
    "c2_atrium": setting(scene="c2_atrium"),
}
# every option that selects another kernel or another walk for stage mode's extend / shadow launches, one at a time
WALK_DEFAULTS = {"cull": -1, "quad": 1, "group_instances": 1, "group_entry_items": 1, "top_flat": 1, "unified_tree": 1, "inline_leaf_roots": 1}
WALK_OPTIONS = {"c1_cornell": [("cull", 0), ("cull", 1), ("quad", 0), ("quad", 1), ("group_instances", 0), ("group_instances", 1),
                               ("group_entry_items", 0), ("group_entry_items", 1)]}
WALK_OPTIONS["edges_inst"] = WALK_OPTIONS["c1_cornell"] + [("top_flat", 0), ("unified_tree", 0), ("inline_leaf_roots", 0)]


def program(variant):
    """tests/golden/user_paths.cl with `#define VARIANT n` in front"""
    n = NUMBER[variant] if isinstance(variant, str) else int(variant)
    return "#define VARIANT %d\n" % n + open(os.path.join(GOLD, "user_paths.cl")).read()


def make_scene(scenes, name, w, h):
    """scenes the existing megakernel tests trace (the device library's fixed traversal stacks are known to suffice)"""
    if name == "c1_cornell":
        return scenes.c1_cornell(w, h, spp=1, depth=5, sphere_subdiv=2)
    if name == "c2_atrium":
        return scenes.c2_atrium(w, h, spp=1, depth=5, detail=0.2)
    if name == "edges_inst":
        import ray_edge_cases as rec
        s = rec.edges_inst(scenes)
        # the scene's own view at this frame size from closer by, through a longer lens: the primary rays of 69 % of the pixels hit
        # (CPU oracle; from the scene's own camera position it is 30 %)
        s.camera = scenes.blender_camera(w, h, 0.08, 0.036, 9.0, 0.0, (0.3, 4.0, 0.5), (-96.0, 180.0, 0.0))
        return s
    if name == "sbt_offset":
        import accel_layout_cases as alc
        s = alc.scene("sbt_offset")
        s.materials = [scenes.material((0.7, 0.7, 0.7), 0.0, 0.5), scenes.material((0.9, 0.8, 0.5), 0.9, 0.2)]
        s.camera = scenes.blender_camera(w, h, 0.05, 0.036, 9.0, 0.0, (0.5, 7.0, 1.0), (-96.0, 180.0, 0.0))
        s.sceneProps = scenes.blender_dir_light(-45.0, 20.0, 5.0)
        s.rtprop = scenes._rtprop(0, 1, 3)
        return s
    raise KeyError(name)


class Stage:
    """One scene on the device with one variant's two shader modules: the same buffers, descriptor set and RTProp for both."""

    def __init__(self, rd, scenes, variant, scene="c1_cornell", w=W, h=H, texture=None):
        self.rd, self.variant = rd, variant
        text = program(variant)
        rd.SetShaderIncludePath("")
        rd.SetOption("user_stages", 2)
        try:
            self.dev = scenes.DeviceScene(make_scene(scenes, scene, w, h), shader_text=text)
            self.staged = self.dev.pipeline
            rd.SetOption("user_stages", 0)
            layout = rd.CreatePipelineLayout([rd.BUFFER_TYPE, rd.BUFFER_TYPE, rd.IMAGE_TYPE, rd.BUFFER_TYPE, rd.BUFFER_TYPE] +
                                             [rd.BUFFER_TYPE] * 6 + [rd.TEX_ARRAY_TYPE, rd.IMAGE_SAMPLER_TYPE, rd.ACCEL_STRUCT_TYPE])
            shader = rd.CreateShaderModule(self.dev.plt, text, len(text), "user_paths")
            self.mega = rd.CreatePipeline(rd.PipelineCreateInfo(1, layout, [shader], []))
        finally:
            rd.SetOption("user_stages", 1)
        self.n = w * h
        self.w, self.h = w, h
        self.rays = {}
        self.image = self.sampler = None
        if texture is not None:
            layers, th, tw, _ = texture.shape
            self.image = rd.CreateImageArray(self.dev.plt, tw, th, layers)
            for l in range(layers):
                rd.WriteImage(self.dev.plt, self.image, tw, th, l, texture[l])
            self.sampler = rd.CreateSampler(self.dev.plt, rd.RD_ADDRESS_REPEAT, rd.RD_FILTER_LINEAR)

    def _primary(self, total, batch):
        """slot 8 for a call: the frame path's own primary rays (rd.GenerateRays has their bits, tests/test_gpu_raygen.py), every
        sample of the call, sample-major, 8 floats per ray"""
        key = (total, batch)
        if key not in self.rays:
            rd = self.rd
            buf = rd.CreateBuffer(self.dev.plt, max(batch, 1) * self.n * 32)
            for k in range(batch):
                rd.GenerateRays(self.dev.rdCamData, self.n, total + k, total, rays=buf, rays_offset=k * self.n * 32, keys=None)
            self.rays[key] = buf
        return self.rays[key]

    def frame(self, staged, depth=5, batch=1, calls=(0,), debug=0, chunk=None, **_):
        """imageScratch (n, 4) as uint32 after the calls of one setting, and of the last call's statistics the extend and shadow
        launches and the sample groups (the pipeline counts at least one group per chunk, a megakernel launch none)"""
        rd, dev = self.rd, self.dev
        # imageScratch starts from a marker, not from zeros: the first sample of a frame is stored, not folded, so RGB does not
        # depend on it, and a black depth-0 frame or an untouched channel 3 shows that the mode under test wrote, or did not
        marker = np.full(self.n * 4, MARKER, F)
        rd.WriteBuffer(dev.plt, dev.rdImageScratch, marker.nbytes, marker)
        if chunk:
            rd.SetOption("chunk_paths", chunk)
        try:
            for total in calls:
                dev.set_rtprop(totalSamples=total, batchSize=batch, depth=depth, debug=debug)
                ds = list(dev.descSet)
                ds[8] = self._primary(total, batch)
                ds[11], ds[12] = self.image, self.sampler
                rd.BindPipeline(dev.plt, self.staged if staged else self.mega)
                rd.BindDescriptorSet(dev.plt, ds)
                rd.TraceRays(dev.plt, 0, 0, 0, self.w, self.h)
            st = rd.GetTraceStats()
        finally:
            if chunk:
                rd.SetOption("chunk_paths", 16 << 20)
        return dev.read_scratch().reshape(-1, 4).view(np.uint32).copy(), (st.launches_extend, st.launches_shadow, st.groups)


def first_difference(mega, staged):
    """None, or a report of the first pixel whose RGB bits differ: both values and the megakernel's event mask"""
    bad = np.nonzero((mega[:, :3] != staged[:, :3]).any(1))[0]
    if bad.size == 0:
        return None
    p = int(bad[0])
    return ("%d of %d pixels differ; first: pixel %d, megakernel %s (%s), stage mode %s (%s), megakernel events 0x%05x"
            % (bad.size, mega.shape[0], p, mega[p, :3].view(F), [hex(x) for x in mega[p, :3]], staged[p, :3].view(F),
               [hex(x) for x in staged[p, :3]], int(mega[p, 3])))


def coverage(mask):
    """the fractions the coverage conditions are about, from the megakernel's event mask of a 1-spp frame (one path per pixel)"""
    m = np.asarray(mask, np.uint32)
    flag = lambda b: (m & b) != 0
    hits, queries, answers = (int(((m >> s) & 15).astype(np.int64).sum()) for s in (8, 12, 16))
    n = float(m.size)
    return dict(hit_ran=flag(HIT_RAN).sum() / n,
                queried_per_hit=queries / max(hits, 1), answered_hit_per_query=answers / max(queries, 1), queries=int(queries),
                false_at_0=flag(FALSE_AT_0).sum() / n, false_later=flag(FALSE_LATER).sum() / n,
                miss_continued_per_missed=flag(MISS_CONTINUED).sum() / max(flag(MISS_RAN).sum(), 1),
                alive_at_last=flag(LAST_DEPTH).sum() / n)


def coverage_failures(variant, cov, depth):
    """the coverage conditions a megakernel frame misses (conditions on the INPUTS, never tolerances): [] when the frame is one
    the comparison means something on.  Every condition holds on every scene; one that a depth cannot meet says from which
    depth it is asked."""
    bad = []
    need = lambda ok, what: None if ok else bad.append("%s: %s" % (variant, what))
    if depth < 1:
        return bad
    need(cov["hit_ran"] >= 0.5, "a closest-hit shader ran on %.3f of the pixels, less than half" % cov["hit_ran"])
    if depth >= 5:
        need(cov["alive_at_last"] > 0.0, "no path is alive at the last depth")
    if variant == "query_some":
        need(0.2 <= cov["queried_per_hit"] <= 0.8, "%.3f of the closest-hit invocations queried, not 20-80 %%" % cov["queried_per_hit"])
    if variant == "no_query":
        need(cov["queries"] == 0, "the shader queried")
    if variant in QUERYING:
        need(0.05 <= cov["answered_hit_per_query"] <= 0.95, "%.3f of the queries were answered \"hit\", not 5-95 %%" % cov["answered_hit_per_query"])
    if variant == "query_last":          # the query writes the payload: "miss" shows as hit = false, "hit" as a path that goes on
        need(cov["false_at_0"] >= 0.05 and cov["false_at_0"] <= 0.95 * cov["hit_ran"], "%.3f of the paths had the query answer \"miss\" at depth 0" % cov["false_at_0"])
    if variant == "hit_false":
        need(cov["false_at_0"] >= 0.05, "only %.3f of the paths end at depth 0" % cov["false_at_0"])
        if depth >= 2:                   # (a closest-hit shader runs after depth 0 from depth 2 on)
            need(cov["false_later"] >= 0.05, "only %.3f of the paths end later" % cov["false_later"])
    if variant == "miss_continues" and (depth >= 2 or cov["hit_ran"] < 1.0):        # (where every primary ray hits, the miss shader runs from depth 1 on)
        need(cov["miss_continued_per_missed"] >= 0.05, "the miss shader continued only %.3f of the missed paths" % cov["miss_continued_per_missed"])
    return bad

"""GPU suite: a user's stage functions on the wavefront pipeline ("stage mode") against THE SAME PROGRAM run as the
megakernel it is.  tests/golden/user_paths.cl has a complete raygen of its own and eleven variants of its closest-hit / miss
shaders (tests/user_stage_cases.py); every variant x frame setting is rendered under "user_stages" 2 and 0 with the same scene,
descriptor set and RTProp, and RGB of imageScratch must be equal as uint32.  The megakernel also writes an event mask per
pixel; the coverage conditions on it make sure a variant reaches the branch it is named after."""
import numpy as np
import pytest

import user_stage_cases as usc
import user_texture_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(gpu):
    import rrt_amd
    from radiance_ray_tracing_amd import rd, scenes
    return rd, scenes


_STAGES = {}


def _stage(mods, variant, scene="c1_cornell", w=usc.W, h=usc.H):
    """one device scene per (variant, scene, frame size), shared by the tests of this module"""
    key = (variant, scene, w, h)
    if key not in _STAGES:
        rd, scenes = mods
        _STAGES[key] = usc.Stage(rd, scenes, variant, scene, w, h, texture=tr.test_image() if variant == "reads_interface" else None)
    return _STAGES[key]


def _same_frame(mods, variant, s, tag=""):
    """the megakernel first -- its event mask has to meet the coverage conditions before stage mode is looked at -- then stage
    mode: RGB equal bit for bit, and each mode ran where it claims to.  imageScratch holds a marker before either run: the
    megakernel replaces all four channels, the pipeline RGB only, so even a depth-0 frame (black in both modes, no traversal
    launch in either) shows that each mode ran and which one it was."""
    st = _stage(mods, variant, s["scene"], s["w"], s["h"])
    marker = np.array([usc.MARKER], np.float32).view(np.uint32)[0]
    mega, (me, ms, mg) = st.frame(False, **s)
    assert (me, ms, mg) == (0, 0, 0), "the megakernel run went through the pipeline's stages"
    assert not (mega == marker).all(1).any(), "the megakernel left pixels of imageScratch as they were"
    assert mega[:, :3].any() == (s["depth"] > 0), "the megakernel frame is black, or a depth-0 frame is not"
    if s["batch"] == 1 and s["calls"] == (0,) and not s["debug"]:
        cov = usc.coverage(mega[:, 3])
        print("%s %s %s: %s" % (variant, s["scene"], tag, {k: round(float(v), 3) for k, v in cov.items()}))
        missed = usc.coverage_failures(variant, cov, s["depth"])
        assert not missed, missed
    staged, (se, ss, sg) = st.frame(True, **s)
    depth = min(s["depth"], 1) if s["debug"] else s["depth"]
    assert se == ss and se >= depth and sg >= 1, "stage mode did not run on the wavefront pipeline (launches %d / %d, groups %d)" % (se, ss, sg)
    assert (staged[:, 3] == marker).all(), "stage mode wrote channel 3 of imageScratch"
    assert not (staged[:, :3] == marker).all(1).any(), "stage mode left pixels of imageScratch as they were"
    diff = usc.first_difference(mega, staged)
    assert diff is None, "%s %s: %s" % (variant, tag, diff)


@pytest.mark.parametrize("variant", list(usc.VARIANTS.values()))
def test_every_variant_equals_its_own_megakernel(mods, variant):
    """c1_cornell, 96 x 54, depth 5, 1 spp, totalSamples 0.  shadow_miss_3 pins a decision: the stage kernel checks row, Tmin and
    Tmax of the nested query; the miss index stays the shader's own in record and in replay (shader/radiance.cl), so a query
    that names miss 3 runs `environment` on the query payload in both modes and the frame equals the megakernel's."""
    _same_frame(mods, variant, usc.setting())


@pytest.mark.parametrize("name", list(usc.CROSSING_SETTINGS))
@pytest.mark.parametrize("variant", usc.CROSSING)
def test_state_that_crosses_bounces(mods, variant, name):
    """the variants whose state crosses bounces -- the payload carried on, hit = false from either shader, the per-pixel random
    numbers after compaction -- at depth 0, 1, 2; debug; three samples in one call, in two progressive calls, in two chunks; a
    frame whose last work-group is partial; an instanced scene with mirrored and non-uniformly scaled transforms and a transform
    group; a scene with deeper trees"""
    _same_frame(mods, variant, usc.CROSSING_SETTINGS[name], name)


@pytest.mark.parametrize("scene", ["c1_cornell", "edges_inst"])
@pytest.mark.parametrize("variant", usc.WALKS)
def test_every_walk_serves_the_stage_functions(mods, variant, scene):
    """depth 4 under every option that selects another kernel or another walk for stage mode's extend and shadow launches"""
    rd, _ = mods
    try:
        for option, value in usc.WALK_OPTIONS[scene]:
            rd.SetOption(option, value)
            try:
                _same_frame(mods, variant, usc.setting(scene=scene, depth=4), "%s %d" % (option, value))
            finally:
                rd.SetOption(option, usc.WALK_DEFAULTS[option])
    finally:
        for option, value in usc.WALK_DEFAULTS.items():
            rd.SetOption(option, value)

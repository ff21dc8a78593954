"""CPU suite: the fixture of the stage-mode parity tests (tests/golden/user_paths.cl, tests/user_stage_cases.py) up to the
point where a GPU is needed: every variant compiles in both modes, without hardware image instructions; the fixture's raygen
and the stage kernel agree on the interface.  No compute."""
import os
import re

import numpy as np
import pytest

import user_stage_cases as usc
import user_texture_ref as tr

CLANG = "/opt/rocm/lib/llvm/bin/clang"
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang is not installed")


@pytest.fixture(scope="module")
def lib():
    return tr.jit_lib()


@pytest.mark.parametrize("variant", list(usc.VARIANTS.values()))
def test_variant_compiles_in_both_modes_without_image_code(lib, variant):
    """as the stage kernel (record / replay traceRay, the stage-mode get_global_id, raygen blanked) and as the megakernel; the
    code objects hold no hardware image instruction (reads_interface calls read_imageui)"""
    text = usc.program(variant)
    assert text.startswith("#define VARIANT %d\n" % usc.NUMBER[variant])
    for stages in (1, 0):
        tr.assert_no_image_code(lib, text, stages)


def test_variants_are_different_programs():
    """the #define selects: no two variants preprocess to the same stage functions (a typo in an #elif would run one body twice)"""
    import subprocess
    shader = os.path.join(usc.ROOT, "radiance-ray-tracing_amd", "shader")
    seen = {}
    for variant in usc.VARIANTS.values():
        out = subprocess.run([CLANG, "-x", "cl", "-cl-std=CL1.2", "-Xclang", "-finclude-default-header", "-target", "amdgcn-amd-amdhsa",
                              "-nogpulib", "-E", "-P", "-I" + shader, "-"], input=usc.program(variant).encode(), stdout=subprocess.PIPE, check=True).stdout
        body = out[out.index(b"void material("):out.index(b"void shadow(")]
        assert body not in seen, (variant, seen[body])
        seen[body] = variant
    assert len(seen) == len(usc.VARIANTS) == 11


def test_raygen_and_stage_kernel_agree_on_the_interface(lib):
    """The fixture's raygen is the documented loop in the words the stage kernel restates it in: the radiance ray (row 1, miss 3,
    0.001 / 1000), the payload's start values, hit = false after each bounce.  And the get_global_id rule: a stage function that
    asks for its pixel where `sceneData` is not in scope does not compile as a stage kernel but does as a megakernel -- the two
    facts the fall-back of "user_stages" 1 rests on (asserted through the compile seam, no launch)."""
    text = usc.program("pixel_rng")
    raygen = text[text.index("__kernel void raygen"):]
    assert "traceRay(topLevel, 1, 3, payload.nextRayOrigin, payload.nextRayDirection, 0.001f, 1000, &payload, &sd, imageArray, sampler);" in raygen
    for start in ("payload.color = (float3)(0.0f)", "payload.hit = false", "payload.nextFactor = (float3)(1.0f)"):
        assert start in raygen
    assert re.search(r"sd\.depth\+\+;\s*payload\.hit = false;\s*if \(debug\) break;", raygen)
    helper = text.replace("void material(", "uint my_pixel(void) { return (uint)get_global_id(0); }\nvoid material(", 1)
    helper = helper.replace("(uint)get_global_id(0), (uint)sceneData->depth));\n    payload->hit = true;",
                            "my_pixel(), (uint)sceneData->depth));\n    payload->hit = true;")
    assert helper.count("my_pixel()") == 1
    t = helper.encode()
    assert lib.rdx_debug_jit_compiles(t, len(t), b"gfx950", 1) != 0
    assert b"compilation failed" in lib.rdx_last_error() and b"sceneData" in lib.rdx_last_error()
    assert lib.rdx_debug_jit_compiles(t, len(t), b"gfx950", 0) == 0, lib.rdx_last_error().decode()


def test_settings_cover_what_the_issue_lists():
    s = usc.CROSSING_SETTINGS
    assert [s[k]["depth"] for k in ("depth0", "depth1", "depth2")] == [0, 1, 2]
    assert s["debug_depth4"]["debug"] == 1 and s["debug_depth4"]["depth"] == 4
    assert s["batch3"]["batch"] == 3 and s["progressive_0_then_3"]["calls"] == (0, 3)
    c = s["two_chunks"]
    assert c["batch"] * c["w"] * c["h"] > c["chunk"] >= c["w"] * c["h"], "the call does not split into chunks of whole samples"
    assert -(-c["batch"] // (c["chunk"] // (c["w"] * c["h"]))) == 2
    p = s["partial_group_97x55"]
    assert (p["w"] * p["h"]) % 256 != 0 and (p["w"] * p["h"]) % 64 != 0
    assert {s["edges_inst"]["scene"], s["c2_atrium"]["scene"]} == {"edges_inst", "c2_atrium"}
    assert set(usc.CROSSING) == {usc.VARIANTS[k] for k in (3, 5, 6, 7, 8)} and set(usc.WALKS) == {usc.VARIANTS[2], usc.VARIANTS[8]}
    assert {o for o, _ in usc.WALK_OPTIONS["edges_inst"]} == set(usc.WALK_DEFAULTS)


def test_coverage_reads_the_event_mask():
    """the helper the GPU tests trust: counts and flags of a hand-made mask"""
    m = np.array([usc.HIT_RAN | usc.QUERIED | usc.ANSWER_HIT | usc.LAST_DEPTH | (3 << 8) | (2 << 12) | (1 << 16),
                  usc.MISS_RAN | usc.MISS_CONTINUED, usc.MISS_RAN, usc.HIT_RAN | usc.FALSE_AT_0 | (1 << 8)], np.uint32)
    c = usc.coverage(m)
    assert c["hit_ran"] == 0.5 and c["queried_per_hit"] == 0.5 and c["answered_hit_per_query"] == 0.5 and c["queries"] == 2
    assert c["false_at_0"] == 0.25 and c["false_later"] == 0 and c["miss_continued_per_missed"] == 0.5 and c["alive_at_last"] == 0.25
    assert usc.coverage_failures("query_some", c, 5) == []
    assert usc.coverage_failures("hit_false", c, 5) and usc.coverage_failures("no_query", c, 5)
